// emu_reader_cache.cpp -- the reader of byte ranges with its cursor cache (orz_decode_range.h) on the emulation backend (TEST
// INFRASTRUCTURE ONLY): the calls of emu_decode_range.cpp, and the cache calls beside them.
#include "emu_decode_range.cpp"

extern "C" int emu_reader_set_cache(void* h, uint64_t max_bytes, char* err, size_t errcap) {
    try {
        ((EmuReader*)h)->rd->set_cache(max_bytes);
        return 0;
    } catch (const std::exception& e) {
        put_err(e, err, errcap);
        return -22;
    }
}

extern "C" uint64_t emu_reader_cursor_state_bytes() { return orz::RangeReader<EmuBackend>::cursor_state_bytes(); }

// stats8 = of the last read: hits, resumed, fresh, uncached, evicted; now: cursors, bytes, budget
extern "C" void emu_reader_cache_stats(void* h, uint64_t* stats8) {
    const orz::RangeCacheStats c = ((EmuReader*)h)->rd->cache_stats();
    stats8[0] = c.hits; stats8[1] = c.resumed; stats8[2] = c.fresh; stats8[3] = c.uncached; stats8[4] = c.evicted;
    stats8[5] = c.cursors; stats8[6] = c.bytes; stats8[7] = c.budget;
}

// the allocation that many calls from now fails (EmuBackend::fail_alloc_in); -1 = never
extern "C" void emu_reader_fail_alloc_in(void* h, long calls) { ((EmuReader*)h)->be.fail_alloc_in = calls; }
