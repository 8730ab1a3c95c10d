// emu_reader_cache.cpp -- the reader of byte ranges with its cursor cache (orz_decode_range.h) on the emulation backend (TEST
// INFRASTRUCTURE ONLY).  "Device memory" is host memory here: the caller's buffers are handed over as they are.  The calls of
// emu_decode_range.cpp under the same names, and the cache calls beside them.
#include "emu_backend.cpp"
#include "../../orz_amd/csrc/orz_decode_range.h"

namespace {
void put_err(const std::exception& e, char* err, size_t cap) {
    if (err && cap) { std::strncpy(err, e.what(), cap - 1); err[cap - 1] = 0; }
}
struct EmuReader {
    EmuBackend be;
    orz::RangeReader<EmuBackend>* rd = nullptr;
    ~EmuReader() { delete rd; }
};
}  // namespace

extern "C" void* emu_reader_open(const uint8_t* src, size_t n, int src_on_device, const uint64_t* offs, const uint64_t* lens, size_t n_table,
                                 char* err, size_t errcap) {
    EmuReader* r = new EmuReader;
    try {
        r->rd = new orz::RangeReader<EmuBackend>(r->be, src, n, src_on_device != 0, offs != nullptr, offs, lens, n_table);
        return r;
    } catch (const std::exception& e) {
        put_err(e, err, errcap);
        delete r;
        return nullptr;
    }
}

extern "C" void emu_reader_close(void* h) { delete (EmuReader*)h; }

extern "C" void emu_reader_info(void* h, uint64_t* members, uint64_t* total, uint64_t* member_offs, size_t cap) {
    EmuReader* r = (EmuReader*)h;
    *members = r->rd->ix.members;
    *total = r->rd->ix.total;
    if (member_offs) {
        const std::vector<uint64_t>& o = r->rd->member_offsets();
        for (size_t k = 0; k < o.size() && k < cap; k++) member_offs[k] = o[k];
    }
}

// 0, -12 (DecodeCapacityError) or -22 (anything else) with the message in err.  stats6 = ranges, members decoded, decoded bytes,
// out bytes, launches, host waits.
extern "C" int emu_reader_read(void* h, const uint64_t* off, const uint64_t* len, size_t n_ranges, uint8_t* dst, size_t cap, unsigned slots,
                               uint64_t* dst_len, uint64_t* stats6, char* err, size_t errcap) {
    EmuReader* r = (EmuReader*)h;
    orz::RangeReadStats st;
    uint64_t total = 0;
    int rc = 0;
    try {
        r->rd->read(off, len, n_ranges, dst, cap, total, st, slots ? slots : 2048);
    } catch (const orz::DecodeCapacityError& e) {
        put_err(e, err, errcap);
        rc = -12;
    } catch (const std::exception& e) {
        put_err(e, err, errcap);
        rc = -22;
    }
    *dst_len = total;
    if (stats6) {
        stats6[0] = st.ranges; stats6[1] = st.members_decoded; stats6[2] = st.decoded_bytes;
        stats6[3] = st.out_bytes; stats6[4] = st.launches; stats6[5] = st.host_waits;
    }
    return rc;
}

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
