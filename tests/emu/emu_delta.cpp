// emu_delta.cpp -- the delta layout (orz_planes.h: PlaneSplitDelta / PlaneMergeDelta, decode_members_planes with bases) on the
// emulation backend (TEST INFRASTRUCTURE ONLY).  "Device memory" is host memory here: the caller's buffers are handed over as
// they are.  The decode counts every launch, as emu_crc.cpp's does.
#include "emu_crc.cpp"

// ONE launch over a table of n tensors (element sizes 1, 2, 4, 8): tensor j's count[j] elements of elem[j] bytes at inter[j], its base
// at base[j] (0: none), its planes plane_pitch(count[j]) apart from plane0[j].  merge = 0: PlaneSplitDelta, else PlaneMergeDelta.
// Returns the launch's work units.
extern "C" uint64_t emu_delta_move(int merge, size_t n, const uint64_t* inter, const uint64_t* base, const uint64_t* plane0, const uint64_t* count,
                                   const uint32_t* elem) {
    EmuBackend be;
    std::vector<orz::PlaneRow> rows(n);
    for (size_t j = 0; j < n; j++) rows[j] = orz::PlaneRow{inter[j], plane0[j], count[j], elem[j]};
    std::vector<uint64_t> image;
    uint64_t units = 0;
    orz::plane_table_image(rows, nullptr, image, units);
    const orz::PlaneTable t = orz::plane_table_at(image.data(), n);
    if (merge) be.launch((size_t)units, orz::PlaneMergeDelta{t, base, units});
    else be.launch((size_t)units, orz::PlaneSplitDelta{t, base, units});
    return units;
}

// decode_members_planes with bases: emu_decode_verified's arguments and answers, and bases[j] = the address of destination j's
// base (0: none); bases == nullptr: the call without the column.
extern "C" int emu_decode_delta(const uint8_t* src, size_t n, int src_on_device, const uint64_t* offs, const uint64_t* lens, size_t n_table,
                                uint8_t* const* dsts, const uint64_t* caps, const uint64_t* bases, const uint32_t* elems, const uint32_t* pieces,
                                size_t n_dsts, const uint32_t* crcs, int verify, unsigned slots, uint64_t* out_lens, uint32_t* out_crcs,
                                uint64_t* members, uint64_t* stats3, uint64_t* bad3, char* err, size_t errcap) {
    uint64_t m = 0;
    int rc = 0;
    orz::DecodeScatterStats st;
    CountingEmu be;
    const std::vector<uint32_t> ones(n_dsts + 1, 1);
    const orz::CrcCheck check{orz::crc_host_image(), crcs, out_crcs};
    try {
        orz::decode_members_planes(be, src, n, src_on_device != 0, offs != nullptr, offs, lens, n_table, dsts, caps, elems ? elems : ones.data(),
                                   n_dsts, out_lens, m, st, slots ? slots : 2048, pieces, verify ? &check : nullptr, bases);
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
