// emu_decode_range.cpp -- the reader of byte ranges (orz_decode_range.h) on the emulation backend (TEST INFRASTRUCTURE ONLY).
// "Device memory" is host memory here: the caller's buffers are handed over as they are.
#include "emu_backend.cpp"
#include "../../orz_amd/csrc/orz_decode_range.h"

namespace {
struct EmuReader {
    EmuBackend be;
    orz::RangeReader<EmuBackend>* rd = nullptr;
    ~EmuReader() { delete rd; }
};
}  // namespace

// a concatenation when offs == nullptr, else the member table offs / lens (n_table entries); nullptr with the message in err
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
