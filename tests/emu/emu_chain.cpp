// emu_chain.cpp -- chains of delta links (orz_chain.h: PlaneMergeChain, ChainPlan, decode_members_chain) on the emulation backend
// (TEST INFRASTRUCTURE ONLY).  "Device memory" is host memory here: the caller's buffers are handed over as they are.  The decode
// counts every launch, as emu_delta.cpp's does.
#include "emu_delta.cpp"

#include "../../orz_amd/csrc/orz_chain.h"

// ONE PlaneMergeChain launch over a table of n tensors (element sizes 1, 2, 4, 8) and `links` plane sets: tensor j's count[j]
// elements of elem[j] bytes go to inter[j], XORed with its base at base[j] (0: none); link k keeps its planes plane_pitch(count[j])
// apart from plane0[k n + j].  Returns the launch's work units.
extern "C" uint64_t emu_chain_move(size_t n, const uint64_t* inter, const uint64_t* base, const uint64_t* plane0, const uint64_t* count,
                                   const uint32_t* elem, uint32_t links) {
    EmuBackend be;
    std::vector<uint64_t> first(n + 1, 0), pitch(n + 1, 0);
    uint64_t units = 0;
    for (size_t j = 0; j < n; j++) {
        first[j] = units;
        pitch[j] = orz::plane_pitch(count[j]);
        units += orz::plane_units(count[j]);
    }
    const orz::PlaneTable t{first.data(), inter, plane0, pitch.data(), count, elem, n};
    be.launch((size_t)units, orz::PlaneMergeChain{t, base, units, links});
    return units;
}

// decode_members_chain: emu_decode_delta's arguments and answers, and `links`
extern "C" int emu_decode_chain(const uint8_t* src, size_t n, int src_on_device, const uint64_t* offs, const uint64_t* lens, size_t n_table,
                                uint8_t* const* dsts, const uint64_t* caps, const uint64_t* bases, const uint32_t* elems, const uint32_t* pieces,
                                size_t n_dsts, const uint32_t* crcs, int verify, unsigned slots, uint32_t links, uint64_t* out_lens, uint32_t* out_crcs,
                                uint64_t* members, uint64_t* stats3, uint64_t* bad3, char* err, size_t errcap) {
    uint64_t m = 0;
    int rc = 0;
    orz::DecodeScatterStats st;
    CountingEmu be;
    const std::vector<uint32_t> ones(n_dsts + 1, 1);
    const orz::CrcCheck check{orz::crc_host_image(), crcs, out_crcs};
    try {
        orz::decode_members_chain(be, src, n, src_on_device != 0, offs != nullptr, offs, lens, n_table, dsts, caps, elems ? elems : ones.data(), n_dsts,
                                  out_lens, m, st, slots ? slots : 2048, pieces, verify ? &check : nullptr, bases, links);
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

// ChainPlan and PlaneScan ALONE over size columns the caller invents, as emu_piece_plan runs PlanePlan: `members` = links x
// sum(elems[j] x pieces[j]) entries of out_len, link-major.  Out: out_off[members]; per destination verdict, units and the merge's
// row (first, inter, pitch, count, elem); plane0[links x n_dsts]; rec3 = the first short destination, the merge's units, the status.
extern "C" void emu_chain_plan(size_t n_dsts, const uint64_t* dsts, const uint64_t* caps, const uint32_t* elems, const uint32_t* pieces,
                               uint32_t links, size_t members, const uint32_t* out_len, uint64_t base, uint64_t stage, uint64_t* out_off,
                               uint32_t* verdict, uint64_t* units, uint64_t* t_first, uint64_t* t_inter, uint64_t* t_plane0, uint64_t* t_pitch,
                               uint64_t* t_count, uint32_t* t_elem, uint64_t* rec3) {
    EmuBackend be;
    std::vector<uint64_t> first_m(n_dsts + 1), ix_off(members + 1);
    uint64_t at = 0;
    for (size_t j = 0; j < n_dsts; j++) { first_m[j] = at; at += (uint64_t)elems[j] * pieces[j]; }
    const uint64_t M1 = at;
    at = 0;
    for (size_t m = 0; m < members; m++) { ix_off[m] = at; at += out_len[m]; }
    std::vector<uint32_t> sizes(members + 1);
    (void)links;
    be.launch(members, orz::ChainPlan{dsts, caps, first_m.data(), elems, pieces, n_dsts, ix_off.data(), out_len, members, M1, base, stage, out_off,
                                      sizes.data(), verdict, units, t_inter, t_pitch, t_count, t_plane0, t_elem});
    orz::PlaneRecord rec{};
    be.launch_waves(1, orz::PlaneScan{units, verdict, t_first, n_dsts, &rec}, orz::PlaneScan::lds_bytes());
    rec3[0] = rec.bad; rec3[1] = rec.units; rec3[2] = rec.status;
}
