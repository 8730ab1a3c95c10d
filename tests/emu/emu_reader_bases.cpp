// emu_reader_bases.cpp -- element ranges of DELTA containers read against their bases (orz_read_elements.h: set_bases,
// ElementGatherDelta / ElementGatherDeltaPieces) on the emulation backend (TEST INFRASTRUCTURE ONLY): the reader's calls of
// emu_delta.cpp and the twins below it, the new call beside them, and the two kernels alone over planes the caller placed.
#include "emu_delta.cpp"

// 0 or -22 with the message in err; bases[j] = the address of tensor j's base (0: none)
extern "C" int emu_reader_set_bases(void* h, const uint64_t* bases, size_t n_tensors, char* err, size_t errcap) {
    try {
        elements_of(h).set_bases(bases, n_tensors);
        return 0;
    } catch (const std::exception& e) {
        put_err(e, err, errcap);
        return -22;
    }
}

// the bases the reader holds: *n = how many (0: none set), the first `cap` of them to out
extern "C" void emu_reader_bases(void* h, uint64_t* n, uint64_t* out, size_t cap) {
    const orz::ElementReader<EmuBackend>& el = elements_of(h);
    *n = el.bases.size();
    for (size_t j = 0; j < el.bases.size() && j < cap; j++) out[j] = el.bases[j];
}

// ONE ElementGatherDelta launch (pieces == nullptr) or ElementGatherDeltaPieces launch over members that lie where the caller put
// them, as emu_element_gather / emu_element_gather_pieces take them; bslice[k] = where the base's bytes for range k's first
// element lie (0: range k has no base), dst_off[k] = where range k's bytes go behind dst (the kernels take any: back to back is
// the reader's choice).  Returns the launch's work units.
extern "C" uint64_t emu_element_gather_delta(size_t n_ranges, const uint64_t* tensor, const uint64_t* first, const uint64_t* count,
                                             const uint64_t* dst_off, const uint64_t* bslice, size_t n_tensors, const uint32_t* elems,
                                             const uint64_t* pieces, const uint64_t* psize, const uint64_t* member_addr, const uint32_t* status,
                                             uint8_t* dst) {
    EmuBackend be;
    std::vector<uint64_t> first_m(n_tensors);
    uint64_t members = 0;
    for (size_t j = 0; j < n_tensors; j++) { first_m[j] = members; members += elems[j] * (pieces ? pieces[j] : 1); }
    const size_t K = n_ranges;
    std::vector<uint64_t> col(8 * K + 1);
    std::vector<uint32_t> el(K + 1);
    uint64_t units = 0;
    for (size_t k = 0; k < K; k++) {
        const uint64_t j = tensor[k];
        col[k] = units; col[K + k] = first[k]; col[2 * K + k] = count[k]; col[3 * K + k] = first_m[j]; col[4 * K + k] = dst_off[k];
        col[5 * K + k] = pieces ? psize[j] : 0; col[6 * K + k] = pieces ? pieces[j] : 0; col[7 * K + k] = bslice[k];
        el[k] = elems[j];
        units += orz::ElementGather::units_of(first[k], count[k]);
    }
    const uint64_t* c = col.data();
    const orz::ElementGatherDelta g{orz::ElementGather{c, c + K, c + 2 * K, c + 3 * K, c + 4 * K, el.data(), K, units, member_addr, status, nullptr, dst},
                                    c + 7 * K};
    if (pieces) be.launch((size_t)units, orz::ElementGatherDeltaPieces{g, c + 5 * K, c + 6 * K});
    else be.launch((size_t)units, g);
    return units;
}
