// emu_decode_to_device.cpp -- the device-side framing index and decode_members_to_device (orz_decode_index.h) on the emulation
// backend, next to index_members, the host index they must agree with (TEST INFRASTRUCTURE ONLY).  "Device memory" is host
// memory here: the caller's buffers are handed over as they are.
#include "emu_backend.cpp"
#include "../../orz_amd/csrc/orz_decode_index.h"

namespace {
void copy_index(uint64_t m, const uint64_t* b, const uint64_t* e, const uint64_t* o, const uint32_t* l, size_t cap, uint64_t* begin,
                uint64_t* end, uint64_t* off, uint32_t* len) {
    for (uint64_t k = 0; k < m && k < cap; k++) { begin[k] = b[k]; end[k] = e[k]; off[k] = o[k]; len[k] = l[k]; }
}
}  // namespace

// index_members: 0 and the arrays (first `cap` members), or 1 with its message
extern "C" int emu_index_members(const uint8_t* src, size_t n, uint64_t* begin, uint64_t* end, uint64_t* off, uint32_t* len, size_t cap,
                                 uint64_t* members, uint64_t* total, char* err, size_t errcap) {
    try {
        const orz::MemberIndex ix = orz::index_members(src, n);
        *members = ix.begin.size();
        *total = ix.out_total;
        copy_index(*members, ix.begin.data(), ix.end.data(), ix.out_off.data(), ix.out_len.data(), cap, begin, end, off, len);
        return 0;
    } catch (const std::exception& e) {
        put_err(e, err, errcap);
        return 1;
    }
}

// the device index (DeviceIndex::build): a concatenation when offs == nullptr, else the member table offs / lens (n_table entries)
extern "C" int emu_device_index(const uint8_t* src, size_t n, const uint64_t* offs, const uint64_t* lens, size_t n_table, uint64_t* begin,
                                uint64_t* end, uint64_t* off, uint32_t* len, size_t cap, uint64_t* members, uint64_t* total, char* err,
                                size_t errcap) {
    try {
        EmuBackend be;
        orz::DeviceIndex<EmuBackend> ix(be);
        ix.build(src, n, offs != nullptr, offs, lens, n_table, true);
        *members = ix.members;
        *total = ix.total;
        copy_index(ix.members, ix.begin, ix.end, ix.out_off, ix.out_len, cap, begin, end, off, len);
        return 0;
    } catch (const std::exception& e) {
        put_err(e, err, errcap);
        return 1;
    }
}

// decode_members_to_device: 0, -12 (DecodeCapacityError) or -22 (anything else) with the message in err.  stats3 = launches, host
// waits, members.
extern "C" int emu_decode_to_device(const uint8_t* src, size_t n, int src_on_device, const uint64_t* offs, const uint64_t* lens, size_t n_table,
                                    uint8_t* dst, size_t cap, unsigned slots, uint64_t* dst_len, uint64_t* members, uint64_t* out_offs,
                                    uint64_t* stats3, char* err, size_t errcap) {
    uint64_t len = 0, m = 0;
    int rc = 0;
    orz::DecodeToDeviceStats st;
    try {
        EmuBackend be;
        orz::decode_members_to_device(be, src, n, src_on_device != 0, offs != nullptr, offs, lens, n_table, dst, cap, len, m, out_offs, st,
                                      slots ? slots : 2048);
    } catch (const orz::DecodeCapacityError& e) {
        put_err(e, err, errcap);
        rc = -12;
    } catch (const std::exception& e) {
        put_err(e, err, errcap);
        rc = -22;
    }
    *dst_len = len;
    *members = m;
    if (stats3) { stats3[0] = st.launches; stats3[1] = st.host_waits; stats3[2] = st.members; }
    return rc;
}
