// emu_plane_pieces.cpp -- planes cut into pieces (orz_planes.h, orz_read_elements.h) on the emulation backend (TEST
// INFRASTRUCTURE ONLY): the reader's calls of emu_elements.cpp, and beside them the decode driver with pieces, the declaration
// with pieces, and the two kernels alone -- the plan on size columns the caller invents, the gather over planes the caller laid out.
#include "emu_elements.cpp"

// decode_members_planes with pieces: 0, -12 (DecodeCapacityError, std::bad_alloc) or -22 (anything else) with the message in err.
// dsts == nullptr sizes.  stats3 = launches, host waits, members.
extern "C" int emu_decode_pieces(const uint8_t* src, size_t n, int src_on_device, const uint64_t* offs, const uint64_t* lens, size_t n_table,
                                 uint8_t* const* dsts, const uint64_t* caps, const uint32_t* elems, const uint32_t* pieces, size_t n_dsts,
                                 unsigned slots, uint64_t* out_lens, uint64_t* members, uint64_t* stats3, char* err, size_t errcap) {
    uint64_t m = 0;
    int rc = 0;
    orz::DecodeScatterStats st;
    try {
        EmuBackend be;
        orz::decode_members_planes(be, src, n, src_on_device != 0, offs != nullptr, offs, lens, n_table, dsts, caps, elems, n_dsts, out_lens, m,
                                   st, slots ? slots : 2048, pieces);
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

// PlanePlan and PlaneScan ALONE over size columns the caller invents (nothing is decoded, no byte of data exists): destination j
// at dsts[j] with caps[j] bytes takes elems[j] x pieces[j] members, out_len[m] = member m's decoded size; the index's prefix sum
// is made here.  Out: out_off[members]; per destination verdict, units and the merge's row (first, inter, plane0, pitch, count,
// elem); rec3 = the first short destination, the merge's units, the status.
extern "C" void emu_piece_plan(size_t n_dsts, const uint64_t* dsts, const uint64_t* caps, const uint32_t* elems, const uint32_t* pieces,
                               size_t members, const uint32_t* out_len, uint64_t base, uint64_t stage, uint64_t* out_off, uint32_t* verdict,
                               uint64_t* units, uint64_t* t_first, uint64_t* t_inter, uint64_t* t_plane0, uint64_t* t_pitch, uint64_t* t_count,
                               uint32_t* t_elem, uint64_t* rec3) {
    EmuBackend be;
    std::vector<uint64_t> first_m(n_dsts), ix_off(members);
    uint64_t at = 0;
    for (size_t j = 0; j < n_dsts; j++) { first_m[j] = at; at += (uint64_t)elems[j] * pieces[j]; }
    at = 0;
    for (size_t m = 0; m < members; m++) { ix_off[m] = at; at += out_len[m]; }
    std::vector<uint32_t> sizes(members);
    be.launch(members, orz::PlanePlan{dsts, caps, first_m.data(), elems, pieces, n_dsts, ix_off.data(), out_len, members, base, stage, out_off,
                                      sizes.data(), verdict, units, t_inter, t_plane0, t_pitch, t_count, t_elem});
    orz::PlaneRecord rec{};
    be.launch_waves(1, orz::PlaneScan{units, verdict, t_first, n_dsts, &rec}, orz::PlaneScan::lds_bytes());
    rec3[0] = rec.bad; rec3[1] = rec.units; rec3[2] = rec.status;
}

extern "C" uint64_t emu_plane_stage_bound(uint64_t total, uint64_t members) { return orz::plane_stage_bound(total, members); }

extern "C" int emu_reader_set_planes_pieces(void* h, const uint32_t* elems, const uint32_t* pieces, size_t n_tensors, char* err, size_t errcap) {
    try {
        elements_of(h).set_planes(elems, n_tensors, pieces);
        return 0;
    } catch (const std::exception& e) {
        put_err(e, err, errcap);
        return -22;
    }
}

// ONE ElementGatherPieces launch over members that lie where the caller put them: tensor j has elems[j] planes of pieces[j]
// pieces, psize[j] elements each but the last; member_addr / status hold an entry per member, plane-major within a tensor;
// range k = count[k] elements of tensor tensor[k] from first[k] (valid: the caller's duty).  The bytes go back to back in range
// order to dst.  Returns the launch's work units.
extern "C" uint64_t emu_element_gather_pieces(size_t n_ranges, const uint64_t* tensor, const uint64_t* first, const uint64_t* count, size_t n_tensors,
                                              const uint32_t* elems, const uint64_t* pieces, const uint64_t* psize, const uint64_t* member_addr,
                                              const uint32_t* status, uint8_t* dst) {
    EmuBackend be;
    std::vector<uint64_t> first_m(n_tensors);
    uint64_t members = 0;
    for (size_t j = 0; j < n_tensors; j++) { first_m[j] = members; members += elems[j] * pieces[j]; }
    const size_t K = n_ranges;
    std::vector<uint64_t> col(7 * K + 1);
    std::vector<uint32_t> el(K + 1);
    uint64_t units = 0, at = 0;
    for (size_t k = 0; k < K; k++) {
        const uint64_t j = tensor[k];
        col[k] = units; col[K + k] = first[k]; col[2 * K + k] = count[k]; col[3 * K + k] = first_m[j]; col[4 * K + k] = at;
        col[5 * K + k] = psize[j]; col[6 * K + k] = pieces[j];
        el[k] = elems[j];
        units += orz::ElementGather::units_of(first[k], count[k]);
        at += count[k] * el[k];
    }
    const uint64_t* c = col.data();
    const orz::ElementGather g{c, c + K, c + 2 * K, c + 3 * K, c + 4 * K, el.data(), K, units, member_addr, status, nullptr, dst};
    be.launch((size_t)units, orz::ElementGatherPieces{g, c + 5 * K, c + 6 * K});
    return units;
}
