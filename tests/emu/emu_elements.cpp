// emu_elements.cpp -- element ranges of plane-encoded tensors (orz_read_elements.h) on the emulation backend (TEST
// INFRASTRUCTURE ONLY): the reader's calls of emu_reader_cache.cpp, the new calls beside them, and ElementGather alone.
#include <map>

#include "emu_reader_cache.cpp"
#include "../../orz_amd/csrc/orz_read_elements.h"

namespace {
std::map<void*, std::unique_ptr<orz::ElementReader<EmuBackend>>> g_elements;  // by reader, made on first use
orz::ElementReader<EmuBackend>& elements_of(void* h) {
    auto& e = g_elements[h];
    if (!e) e.reset(new orz::ElementReader<EmuBackend>(*((EmuReader*)h)->rd));
    return *e;
}
}  // namespace

// closes the reader too
extern "C" void emu_elements_close(void* h) {
    g_elements.erase(h);
    emu_reader_close(h);
}

extern "C" int emu_reader_set_planes(void* h, const uint32_t* elems, size_t n_tensors, char* err, size_t errcap) {
    try {
        elements_of(h).set_planes(elems, n_tensors);
        return 0;
    } catch (const std::exception& e) {
        put_err(e, err, errcap);
        return -22;
    }
}

extern "C" void emu_reader_tensor_info(void* h, uint64_t* n_tensors, uint64_t* counts, uint32_t* elems, size_t cap) {
    const orz::ElementReader<EmuBackend>& el = elements_of(h);
    *n_tensors = el.elems.size();
    for (size_t j = 0; j < el.elems.size() && j < cap; j++) {
        if (counts) counts[j] = el.counts[j];
        if (elems) elems[j] = el.elems[j];
    }
}

// 0, -12 (DecodeCapacityError) or -22 (anything else) with the message in err.  stats6 as emu_reader_read's.
extern "C" int emu_reader_read_elements(void* h, const uint64_t* tensor, const uint64_t* first, const uint64_t* count, size_t n_ranges,
                                        uint8_t* dst, size_t cap, unsigned slots, uint64_t* dst_len, uint64_t* stats6, char* err, size_t errcap) {
    orz::RangeReadStats st;
    uint64_t total = 0;
    int rc = 0;
    try {
        elements_of(h).read(tensor, first, count, n_ranges, dst, cap, total, st, slots ? slots : 2048);
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

// ONE ElementGather launch over planes that lie where the caller put them: tensor j has elems[j] planes, plane_addr / status hold
// an entry per plane in tensor order; range k = count[k] elements of tensor tensor[k] from first[k] (valid: the caller's duty).
// The bytes go back to back in range order to dst.  Returns the launch's work units.
extern "C" uint64_t emu_element_gather(size_t n_ranges, const uint64_t* tensor, const uint64_t* first, const uint64_t* count, size_t n_tensors,
                                       const uint32_t* elems, const uint64_t* plane_addr, const uint32_t* status, uint8_t* dst) {
    EmuBackend be;
    std::vector<uint64_t> first_m(n_tensors);
    uint64_t planes = 0;
    for (size_t j = 0; j < n_tensors; j++) { first_m[j] = planes; planes += elems[j]; }
    const size_t K = n_ranges;
    std::vector<uint64_t> col(5 * K + 1);
    std::vector<uint32_t> el(K + 1);
    uint64_t units = 0, at = 0;
    for (size_t k = 0; k < K; k++) {
        col[k] = units; col[K + k] = first[k]; col[2 * K + k] = count[k]; col[3 * K + k] = first_m[tensor[k]]; col[4 * K + k] = at;
        el[k] = elems[tensor[k]];
        units += orz::ElementGather::units_of(first[k], count[k]);
        at += count[k] * el[k];
    }
    const uint64_t* c = col.data();
    be.launch((size_t)units, orz::ElementGather{c, c + K, c + 2 * K, c + 3 * K, c + 4 * K, el.data(), K, units, plane_addr, status, nullptr, dst});
    return units;
}
