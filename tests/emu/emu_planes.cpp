// emu_planes.cpp -- PlaneSplit / PlaneMerge and decode_members_planes (orz_planes.h) on the emulation backend (TEST
// INFRASTRUCTURE ONLY).  "Device memory" is host memory here: the caller's buffers are handed over as they are.
#include "emu_backend.cpp"
#include "../../orz_amd/csrc/orz_planes.h"

// ONE launch over a table of n tensors (element sizes 2, 4, 8): tensor j's count[j] elements of elem[j] bytes at inter[j], its
// planes plane_pitch(count[j]) apart from plane0[j].  merge = 0: PlaneSplit, else PlaneMerge.  Returns the launch's work units.
extern "C" uint64_t emu_plane_move(int merge, size_t n, const uint64_t* inter, const uint64_t* plane0, const uint64_t* count, const uint32_t* elem) {
    EmuBackend be;
    std::vector<orz::PlaneRow> rows(n);
    for (size_t j = 0; j < n; j++) rows[j] = orz::PlaneRow{inter[j], plane0[j], count[j], elem[j]};
    std::vector<uint64_t> image;
    uint64_t units = 0;
    orz::plane_table_image(rows, nullptr, image, units);
    const orz::PlaneTable t = orz::plane_table_at(image.data(), n);
    if (merge) be.launch((size_t)units, orz::PlaneMerge{t, units});
    else be.launch((size_t)units, orz::PlaneSplit{t, units});
    return units;
}

extern "C" uint64_t emu_plane_pitch(uint64_t count) { return orz::plane_pitch(count); }

// decode_members_planes: 0, -12 (DecodeCapacityError, std::bad_alloc) or -22 (anything else) with the message in err.
// dsts == nullptr sizes.  stats3 = launches, host waits, members.
extern "C" int emu_decode_planes(const uint8_t* src, size_t n, int src_on_device, const uint64_t* offs, const uint64_t* lens, size_t n_table,
                                 uint8_t* const* dsts, const uint64_t* caps, const uint32_t* elems, size_t n_dsts, unsigned slots,
                                 uint64_t* out_lens, uint64_t* members, uint64_t* stats3, char* err, size_t errcap) {
    uint64_t m = 0;
    int rc = 0;
    orz::DecodeScatterStats st;
    try {
        EmuBackend be;
        orz::decode_members_planes(be, src, n, src_on_device != 0, offs != nullptr, offs, lens, n_table, dsts, caps, elems, n_dsts, out_lens, m,
                                   st, slots ? slots : 2048);
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
    if (stats3) { stats3[0] = st.launches; stats3[1] = st.host_waits; stats3[2] = st.members; }
    return rc;
}
