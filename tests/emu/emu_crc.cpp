// emu_crc.cpp -- the CRC-32 kernels (orz_crc.h) and the verified decode (orz_planes.h) on the emulation backend (TEST
// INFRASTRUCTURE ONLY): the three digest launches over buffers that lie where the caller put them, the power function the fold
// kernel uses, the host restatement, and decode_members_planes with a digest check -- every launch counted, not the decode's alone.
#include "emu_plane_pieces.cpp"

#include "../../orz_amd/csrc/orz_crc.h"

namespace {
// the emulation with a count of the launches that have work (a launch of nothing is none on the device either)
struct CountingEmu : EmuBackend {
    uint64_t launched = 0;
    template <class F> void launch(size_t n, const F& f) {
        if (n) launched++;
        EmuBackend::launch(n, f);
    }
    template <class K> void launch_waves(size_t nblocks, const K& k, size_t lds_bytes) {
        if (nblocks) launched++;
        EmuBackend::launch_waves(nblocks, k, lds_bytes);
    }
};
}  // namespace

// the digests of n buffers "on the device": stats2 = launches, host waits
extern "C" int emu_crc_buffers(const uint64_t* addrs, const uint64_t* lens, size_t n, uint32_t* crcs, uint64_t* stats2, char* err, size_t errcap) {
    try {
        CountingEmu be;
        uint64_t waits = 0;
        orz::crc32_device_buffers(be, orz::crc_host_image(), addrs, lens, n, crcs, waits);
        if (stats2) { stats2[0] = be.launched; stats2[1] = waits; }
        return 0;
    } catch (const std::exception& e) {
        put_err(e, err, errcap);
        return -22;
    }
}
extern "C" uint32_t emu_crc_tile_bytes() { return orz::kCrcTileBytes; }
extern "C" uint64_t emu_crc_tiles(uint64_t addr, uint64_t len) { return orz::crc_tiles(addr, len); }
extern "C" uint32_t emu_crc_lds_bytes() { return (uint32_t)orz::CrcTiles::lds_bytes(); }
// x^(8 bytes) mod P by the function CrcFold uses, over the device image's table of powers
extern "C" uint32_t emu_crc_xpow_bytes(uint64_t bytes) { return orz::crc_xpow_bytes(orz::crc_host_image() + orz::kCrcImgPow, bytes); }
extern "C" uint32_t emu_crc_combine(uint32_t a, uint32_t b, uint64_t len_b) { return orz::crc32_combine(a, b, len_b); }
extern "C" uint32_t emu_crc_host(const uint8_t* p, size_t n) { return orz::crc32_host(p, n); }

// decode_members_planes with a digest check: emu_decode_pieces' arguments, elems == nullptr: every element size 1, pieces == nullptr:
// one piece each; crcs: the expected digests, out_crcs: the computed ones (n_dsts entries, untouched unless the digest launches
// ran).  0, -12, -22 as there, -74 (DecodeDigestError: bad3 = the destination, expected, computed).  stats3 = ALL launches, host
// waits, members.
extern "C" int emu_decode_verified(const uint8_t* src, size_t n, int src_on_device, const uint64_t* offs, const uint64_t* lens, size_t n_table,
                                   uint8_t* const* dsts, const uint64_t* caps, const uint32_t* elems, const uint32_t* pieces, size_t n_dsts,
                                   const uint32_t* crcs, int verify, unsigned slots, uint64_t* out_lens, uint32_t* out_crcs, uint64_t* members,
                                   uint64_t* stats3, uint64_t* bad3, char* err, size_t errcap) {
    uint64_t m = 0;
    int rc = 0;
    orz::DecodeScatterStats st;
    CountingEmu be;
    const std::vector<uint32_t> ones(n_dsts + 1, 1);
    const orz::CrcCheck check{orz::crc_host_image(), crcs, out_crcs};
    try {
        orz::decode_members_planes(be, src, n, src_on_device != 0, offs != nullptr, offs, lens, n_table, dsts, caps, elems ? elems : ones.data(),
                                   n_dsts, out_lens, m, st, slots ? slots : 2048, pieces, verify ? &check : nullptr);
    } catch (const orz::DecodeDigestError& e) {
        put_err(e, err, errcap);
        if (bad3) { bad3[0] = e.dst; bad3[1] = e.expected; bad3[2] = e.computed; }
        rc = -74;
    } catch (const orz::DecodeCapacityError& e) {
        put_err(e, err, errcap);
        rc = -12;
    } catch (const std::bad_alloc& e) {
        put_err(e, err, errcap);
        rc = -12;
    } catch (const std::exception& e) {
        put_err(e, err, errcap);
        rc = -22;
    }
    *members = m;
    if (stats3) { stats3[0] = be.launched; stats3[1] = st.host_waits; stats3[2] = st.members; }
    return rc;
}
