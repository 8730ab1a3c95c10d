// orz_read_elements.h -- element ranges of PLANE-ENCODED tensors, read through a RangeReader and merged on the device.
//
// A container written by orz_members_encode_planes_to_device holds a tensor of e-byte elements as e members, one per byte plane
// (orz_planes.h).  The reader of byte ranges (orz_decode_range.h) serves bytes of single planes; decode_members_planes takes
// whole tensors only.  Here the two meet: the caller declares which members are the planes of which tensor (set_planes) and
// asks for ELEMENTS [first, first + count) of tensors; their interleaved bytes come back to back in range order.
//
// The host expands an element range of tensor j into one byte range per plane -- member_off[first_member + p] + first, length
// count -- and the read is RangeReader's own from there (RangeReader::run: the plan, the arena or the cursors, the decode launches
// with their stops, the verdicts), so it costs what the bytes asked for cost: a plane is decoded only as far as the furthest
// element asked of its tensor, once a call, and a tensor's e planes decode side by side.  The expanded byte ranges and the
// element-range table go up in the read's one upload; the host waits as often as for a byte-range read.
//
// What ends the read is ElementGather instead of RangeGather: one launch, one lane per work unit.  A unit of range k is the part
// of [first, first + count) inside one 16-element block of the PLANE, cut at the plane's multiples of 16 (RangeGather cuts at its
// destination's).  Arena pieces and cursor buffers start at multiples of 16 and all planes of a tensor share `first`, so the e
// plane addresses of a unit are co-aligned: an interior unit over planes at multiples of 16 loads e x 16 bytes (plane_load16),
// interleaves them in registers (plane_merge_shuffle, the shuffles of PlaneMerge) and stores 16 e bytes -- 16 at a time where
// the unit's destination is a multiple of 16, dwords where it is a multiple of 4.  Head and tail units, units over planes at
// other addresses and units whose destination is no multiple of 4 go byte by byte; the checks are made at run time.  An element
// size of 1 is a plain copy through the same kernel.  A unit with a plane whose decode failed writes nothing.  No LDS, no
// scratch, no atomics; the rule of DESIGN 2a holds: a lane writes its own unit's bytes only and reads what earlier launches wrote.
//
// PIECES (orz_planes.h): a declaration may say that tensor j's planes are cut into pieces[j] members each, S elements to a piece,
// S a multiple of 16.  An element range then becomes one byte range per plane PER PIECE IT TOUCHES, so a read decodes only those
// pieces, each as far as the furthest element asked inside it, side by side -- the last rows of a tensor cost its last pieces.
// ElementGatherPieces is ElementGather with the columns S and Q: a unit never straddles two pieces, so it finds its piece
// q = block / S once and takes plane p's bytes from member first + p Q + q at lo - q S.  A declaration without pieces reads
// through ElementGather exactly as before.
#pragma once
#include <string>
#include <vector>

#include "orz_decode_range.h"
#include "orz_planes.h"

namespace orz {

// a dword of device memory at a multiple of 4, stored in the GLOBAL address space (as plane_store16 stores sixteen bytes)
ORZ_HD void element_store4(uint8_t* d, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    *(__attribute__((address_space(1))) uint32_t*)d = v;
#else
    __builtin_memcpy(d, &v, 4);
#endif
}

// One interior unit: 16 bytes of each of the E planes, at multiples of 16 (plane p's at base + place[p Q] + lo, modulo 2^64), into
// 16 E interleaved bytes at d, a multiple of 4.
template <int E>
ORZ_HD void element_unit_merge(uint8_t* d, uint64_t base, const uint64_t* place, uint64_t lo, uint64_t Q) {
    uint32_t w[4 * E], pl[4 * E];
#pragma unroll
    for (int p = 0; p < E; p++) plane_load16(pl + 4 * p, (const uint8_t*)(uintptr_t)(base + place[(uint64_t)p * Q] + lo));
    if constexpr (E == 1) {
#pragma unroll
        for (int q = 0; q < 4; q++) w[q] = pl[q];
    } else {
        plane_merge_shuffle<E>(pl, w);
    }
    if (((uintptr_t)d & 15) == 0) {
#pragma unroll
        for (int q = 0; q < E; q++) plane_store16(d + 16 * q, w + 4 * q);
    } else {
#pragma unroll
        for (int q = 0; q < 4 * E; q++) element_store4(d + 4 * q, w[q]);
    }
}

// One lane per work unit.  The element ranges as columns (device memory, [n_ranges] each): ufirst = the range's first unit (a
// prefix sum of the ranges' unit counts; an empty range repeats its successor's, so the search never lands on it), first / count
// in elements, member = the first member of the range's tensor, dst_off = where the range's bytes go in dst, elem = the element
// size.  place / status as RangeReader::run hands them to a gather.
struct ElementGather {
    const uint64_t *ufirst, *first, *count, *member, *dst_off;
    const uint32_t* elem;
    uint64_t n_ranges, units;
    const uint64_t* place;
    const uint32_t* status;
    const uint8_t* base;
    uint8_t* dst;
    static uint64_t units_of(uint64_t first, uint64_t count) {
        return count ? (first + count + (kPlaneUnit - 1)) / kPlaneUnit - first / kPlaneUnit : 0;
    }
    ORZ_HD void operator()(size_t unit) const { gather_unit<false>((uint64_t)unit, nullptr, nullptr); }
    // unit u; kPieces: the range's tensor has pieces[k] pieces of psize[k] elements to a plane (else one: the columns are not read)
    template <bool kPieces>
    ORZ_HD void gather_unit(uint64_t u, const uint64_t* psize, const uint64_t* pieces) const {
        if (u >= units || !n_ranges) return;
        const uint64_t k = last_at_or_below(ufirst, n_ranges, u);
        const uint64_t f = first[k], end = f + count[k];
        const uint64_t block = (f / kPlaneUnit + (u - ufirst[k])) * kPlaneUnit;
        const uint64_t lo = block > f ? block : f, hi = block + kPlaneUnit < end ? block + kPlaneUnit : end;
        if (lo >= hi) return;
        const uint32_t e = elem[k];
        // the unit's piece (S is a multiple of the unit: [block, block + 16) lies in one), its planes Q members apart
        const uint64_t Q = kPieces ? pieces[k] : 1, q = kPieces ? block / psize[k] : 0;
        const uint64_t in = lo - (kPieces ? q * psize[k] : 0);  // the unit's first byte in its plane's member
        const uint64_t* pl = place + member[k] + q;
        const uint32_t* st = status + member[k] + q;
        const uint64_t b = (uint64_t)(uintptr_t)base;
        uint64_t bits = 0;
        for (uint32_t p = 0; p < e; p++) {
            if (st[(uint64_t)p * Q] != kDecOk) return;
            bits |= b + pl[(uint64_t)p * Q] + in;
        }
        uint8_t* const d = dst + dst_off[k] + (lo - f) * e;
        if (hi - lo == kPlaneUnit && (bits & 15) == 0 && ((uintptr_t)d & 3) == 0 && (e == 1 || e == 2 || e == 4 || e == 8)) {
            if (e == 1) element_unit_merge<1>(d, b, pl, in, Q);
            else if (e == 2) element_unit_merge<2>(d, b, pl, in, Q);
            else if (e == 4) element_unit_merge<4>(d, b, pl, in, Q);
            else element_unit_merge<8>(d, b, pl, in, Q);
            return;
        }
        const uint32_t n = (uint32_t)(hi - lo);
        for (uint32_t p = 0; p < e; p++) {
            const uint8_t* s = (const uint8_t*)(uintptr_t)(b + pl[(uint64_t)p * Q] + in);
            for (uint32_t i = 0; i < n; i++) d[(uint64_t)i * e + p] = s[i];
        }
    }
};

// ElementGather over tensors whose planes are cut into pieces: per range, psize = the elements of a piece (a multiple of 16; of
// a tensor of one piece any number above its last element's) and pieces = the pieces to a plane.
struct ElementGatherPieces {
    ElementGather g;
    const uint64_t *psize, *pieces;  // [n_ranges]
    ORZ_HD void operator()(size_t unit) const { g.gather_unit<true>((uint64_t)unit, psize, pieces); }
};

// ------------------------------------------------------------------------------------------------ deltas against base tensors
// ElementGatherDelta / ElementGatherDeltaPieces are ElementGather / ElementGatherPieces with one more column: bslice[k], the
// address of the BASE's bytes for range k's first element -- base[tensor[k]] + first[k] * elem[k], worked out on the host -- or 0:
// range k has no base.  The members hold the planes of tensor XOR base (orz_planes.h), and a unit of a range with a base writes
// planes XOR base, its base bytes at bslice[k] + (lo - first[k]) e: the gather loads every plane byte and stores every output byte
// once anyway, so that is where the base comes in, as PlaneMergeDelta took it into the merge.  Work units, the search over the
// ranges, the piece arithmetic and the status check are ElementGather's.  A full unit over planes at multiples of 16 whose
// destination and base address are multiples of 4: the e 16-byte plane loads and the 16 e base bytes -- 16 at a time where the
// base address is a multiple of 16, dwords otherwise -- ALL issued before the first store, the XOR on the 4 e interleaved dwords
// behind the shuffle, and the stores of element_unit_merge.  Every other unit goes byte by byte, each base byte read just before
// the byte at the same index is written.  A range without a base moves exactly as ElementGather moves it; a unit with a plane
// whose decode failed writes nothing.  No LDS, no scratch, no atomics, and the rule of DESIGN 2a: a lane reads and writes its own
// unit only -- which makes a read IN PLACE safe, bslice[k] == the range's destination: the lane has loaded its base bytes before
// it stores over them, and no other lane reads them.
// The bodies are their own, not gather_unit with a parameter more: the plain kernels keep their code and registers.

// a dword of device memory at a multiple of 4, loaded from the GLOBAL address space (as plane_load16 loads sixteen bytes)
ORZ_HD uint32_t element_load4(const uint8_t* s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(__attribute__((address_space(1))) const uint32_t*)s;
#else
    uint32_t v;
    __builtin_memcpy(&v, s, 4);
    return v;
#endif
}

// element_unit_merge with a base: the 16 E base bytes at bs, a multiple of 4, XORed into the interleaved dwords
template <int E>
ORZ_HD void element_unit_merge_delta(uint8_t* d, const uint8_t* bs, uint64_t base, const uint64_t* place, uint64_t lo, uint64_t Q) {
    uint32_t w[4 * E], x[4 * E], pl[4 * E];
#pragma unroll
    for (int p = 0; p < E; p++) plane_load16(pl + 4 * p, (const uint8_t*)(uintptr_t)(base + place[(uint64_t)p * Q] + lo));
    if (((uintptr_t)bs & 15) == 0) {
#pragma unroll
        for (int q = 0; q < E; q++) plane_load16(x + 4 * q, bs + 16 * q);
    } else {
#pragma unroll
        for (int q = 0; q < 4 * E; q++) x[q] = element_load4(bs + 4 * q);
    }
    if constexpr (E == 1) {
#pragma unroll
        for (int q = 0; q < 4; q++) w[q] = pl[q];
    } else {
        plane_merge_shuffle<E>(pl, w);
    }
#pragma unroll
    for (int q = 0; q < 4 * E; q++) w[q] ^= x[q];
    if (((uintptr_t)d & 15) == 0) {
#pragma unroll
        for (int q = 0; q < E; q++) plane_store16(d + 16 * q, w + 4 * q);
    } else {
#pragma unroll
        for (int q = 0; q < 4 * E; q++) element_store4(d + 4 * q, w[q]);
    }
}

struct ElementGatherDelta {
    ElementGather g;
    const uint64_t* bslice;  // [n_ranges] where the base's bytes for the range's first element lie (0: no base)
    ORZ_HD void operator()(size_t unit) const { gather_unit<false>((uint64_t)unit, nullptr, nullptr); }
    // unit u; kPieces, psize, pieces as ElementGather::gather_unit takes them
    template <bool kPieces>
    ORZ_HD void gather_unit(uint64_t u, const uint64_t* psize, const uint64_t* pieces) const {
        if (u >= g.units || !g.n_ranges) return;
        const uint64_t k = last_at_or_below(g.ufirst, g.n_ranges, u);
        const uint64_t f = g.first[k], end = f + g.count[k];
        const uint64_t block = (f / kPlaneUnit + (u - g.ufirst[k])) * kPlaneUnit;
        const uint64_t lo = block > f ? block : f, hi = block + kPlaneUnit < end ? block + kPlaneUnit : end;
        if (lo >= hi) return;
        const uint32_t e = g.elem[k];
        const uint64_t Q = kPieces ? pieces[k] : 1, q = kPieces ? block / psize[k] : 0;
        const uint64_t in = lo - (kPieces ? q * psize[k] : 0);
        const uint64_t* pl = g.place + g.member[k] + q;
        const uint32_t* st = g.status + g.member[k] + q;
        const uint64_t b = (uint64_t)(uintptr_t)g.base;
        uint64_t bits = 0;
        for (uint32_t p = 0; p < e; p++) {
            if (st[(uint64_t)p * Q] != kDecOk) return;
            bits |= b + pl[(uint64_t)p * Q] + in;
        }
        uint8_t* const d = g.dst + g.dst_off[k] + (lo - f) * e;
        const bool quads = hi - lo == kPlaneUnit && (bits & 15) == 0 && ((uintptr_t)d & 3) == 0 && (e == 1 || e == 2 || e == 4 || e == 8);
        const uint32_t n = (uint32_t)(hi - lo);
        const uint64_t b0 = bslice[k];
        if (!b0) {  // no base: as ElementGather moves it
            if (quads) {
                if (e == 1) element_unit_merge<1>(d, b, pl, in, Q);
                else if (e == 2) element_unit_merge<2>(d, b, pl, in, Q);
                else if (e == 4) element_unit_merge<4>(d, b, pl, in, Q);
                else element_unit_merge<8>(d, b, pl, in, Q);
                return;
            }
            for (uint32_t p = 0; p < e; p++) {
                const uint8_t* s = (const uint8_t*)(uintptr_t)(b + pl[(uint64_t)p * Q] + in);
                for (uint32_t i = 0; i < n; i++) d[(uint64_t)i * e + p] = s[i];
            }
            return;
        }
        const uint8_t* const bs = (const uint8_t*)(uintptr_t)b0 + (lo - f) * e;
        if (quads && ((uintptr_t)bs & 3) == 0) {
            if (e == 1) element_unit_merge_delta<1>(d, bs, b, pl, in, Q);
            else if (e == 2) element_unit_merge_delta<2>(d, bs, b, pl, in, Q);
            else if (e == 4) element_unit_merge_delta<4>(d, bs, b, pl, in, Q);
            else element_unit_merge_delta<8>(d, bs, b, pl, in, Q);
            return;
        }
        for (uint32_t p = 0; p < e; p++) {
            const uint8_t* s = (const uint8_t*)(uintptr_t)(b + pl[(uint64_t)p * Q] + in);
            for (uint32_t i = 0; i < n; i++) {  // (in place the base byte IS the byte written: read first)
                const uint64_t a = (uint64_t)i * e + p;
                d[a] = (uint8_t)(s[i] ^ bs[a]);
            }
        }
    }
};

struct ElementGatherDeltaPieces {
    ElementGatherDelta g;
    const uint64_t *psize, *pieces;  // [n_ranges], as ElementGatherPieces'
    ORZ_HD void operator()(size_t unit) const { g.gather_unit<true>((uint64_t)unit, psize, pieces); }
};

// The declaration of a reader's container as plane-encoded tensors, and the reads of element ranges it allows.  It borrows the
// reader (declared before it, destroyed after it) and keeps nothing on the device of its own.
template <class BE>
struct ElementReader {
    RangeReader<BE>& rd;
    std::vector<uint32_t> elems;    // [tensors] element sizes; empty = nothing declared
    std::vector<uint64_t> first_m;  // [tensors] a tensor's first member
    std::vector<uint64_t> counts;   // [tensors] its elements = the decoded size of each of its planes, all pieces together
    std::vector<uint64_t> pieces;   // [tensors] pieces to a plane
    std::vector<uint64_t> psize;    // [tensors] elements to a piece (of one piece: the tensor's count, or 1 when it has none)
    bool pieced = false;            // some tensor has more than one piece to a plane
    std::vector<uint64_t> bases;    // [tensors] the address of a tensor's base (0: none); empty = no bases (set_bases)
    explicit ElementReader(RangeReader<BE>& r) : rd(r) {}

    // Tensor j is the next e[j] members, plane 0 first -- with `q`, the next e[j] x q[j] members, q[j] pieces to a plane,
    // plane-major; n_tensors == 0 withdraws the declaration.  Throws RangeArgumentError with nothing changed.  At most one host
    // wait: the member offsets, if the reader has not fetched them yet.
    void set_planes(const uint32_t* e, size_t n_tensors, const uint32_t* q = nullptr) {
        if (n_tensors && !e) throw RangeArgumentError("invalid argument: tensors without element sizes");
        std::vector<uint64_t> fm(n_tensors), cnt(n_tensors), pcs(n_tensors, 1), psz(n_tensors);
        uint64_t planes = 0;
        bool cut = false;
        for (size_t j = 0; j < n_tensors; j++) {
            if (!plane_elem_ok(e[j]))
                throw RangeArgumentError("invalid argument: tensor " + std::to_string(j) + " has elements of " + std::to_string(e[j]) +
                                         " bytes (1, 2, 4 or 8)");
            if (q && !q[j]) throw RangeArgumentError("invalid argument: tensor " + std::to_string(j) + " has no pieces");
            if (q) pcs[j] = q[j];
            cut = cut || pcs[j] > 1;
            fm[j] = planes;
            planes += e[j] * pcs[j];
        }
        const uint64_t M = rd.ix.members;
        if (n_tensors && planes != M)
            throw RangeArgumentError("invalid argument: " + std::to_string(planes) + (q ? " pieces of planes for " : " planes for ") +
                                     std::to_string(M) + " members");
        if (n_tensors) rd.member_offsets();
        for (size_t j = 0; j < n_tensors; j++) {
            try {
                cnt[j] = plane_piece_count("tensor", j, fm[j], e[j], pcs[j], [&](uint64_t m) { return (uint64_t)rd.member_len(m); });
            } catch (const std::runtime_error& err) {
                throw RangeArgumentError(err.what());
            }
            psz[j] = pcs[j] > 1 ? rd.member_len(fm[j]) : cnt[j] ? cnt[j] : 1;
        }
        elems.assign(e, e + n_tensors);
        first_m.swap(fm);
        counts.swap(cnt);
        pieces.swap(pcs);
        psize.swap(psz);
        pieced = cut;
        bases.clear();  // (they were those of the tensors declared before)
    }

    // DELTAS: the members hold the planes of tensor XOR base (orz_members_encode_deltas_to_device), and b[j] is the address of
    // tensor j's base -- counts[j] x elems[j] bytes of device memory on the reader's device -- or 0 for none; reads then return
    // planes XOR base.  n must be the number of tensors declared; n == 0 withdraws the bases, as every successful set_planes
    // does (a refused one leaves them).  The bases are borrowed and only read: one may overlap the container or another base.  A
    // base of a tensor of no elements is not looked at.  Throws RangeArgumentError with nothing changed.  Launches nothing and
    // waits for nothing; cursors are kept: they hold planes and know nothing of bases.
    void set_bases(const uint64_t* b, size_t n) {
        if (n == 0) {
            bases.clear();
            return;
        }
        if (elems.empty()) throw RangeArgumentError("invalid argument: the container is not declared as planes of tensors");
        if (n != elems.size())
            throw RangeArgumentError("invalid argument: " + std::to_string(n) + " bases for " + std::to_string(elems.size()) + " tensors");
        if (!b) throw RangeArgumentError("invalid argument: bases without their array");
        std::vector<uint64_t> bs(n, 0);
        for (size_t j = 0; j < n; j++) {
            const uint64_t len = counts[j] * elems[j];  // (a plane holds less than 2^32 bytes a piece: no overflow)
            if (!len || !b[j]) continue;
            if (len > (uint64_t)0 - b[j])
                throw RangeArgumentError("invalid argument: the base of tensor " + std::to_string(j) + " (" + std::to_string(len) +
                                         " bytes) wraps the address space");
            bs[j] = b[j];
        }
        bases.swap(bs);
    }

    // Elements [first[k], first[k] + count[k]) of tensor tensor[k], their interleaved bytes back to back in range order at d_dst.
    // dst_len = the sum of the bytes whenever the ranges are valid.  Throws what RangeReader::read throws, for the same reasons.
    // With bases (set_bases): when a range that has elements names a tensor with a base, the ranges' base slices go up as one more
    // column of the read's ONE upload and ElementGatherDelta(Pieces) ends the read where the plain gather would, so the ranges of
    // tensors with a base come back as planes XOR base in the same launches and host waits; otherwise the read is the one without
    // bases, kernel and upload.  The base slice of such a range -- its count x e bytes from base + first x e -- must be disjoint
    // from ALL the bytes the read writes, [d_dst, d_dst + dst_len), or begin exactly where the range's own bytes go: the read IN
    // PLACE, after which the slice holds the restored elements.  Any other overlap would be overwritten by, or overwrite, another
    // range: RangeArgumentError naming the range, before anything reaches the device.
    void read(const uint64_t* tensor, const uint64_t* first, const uint64_t* count, size_t n_ranges, uint8_t* d_dst, size_t d_cap,
              uint64_t& dst_len, RangeReadStats& st, uint32_t slots = 2048) {
        BE& be = rd.be;
        const double t0 = be.now();
        st = RangeReadStats{};
        st.ranges = n_ranges;
        dst_len = 0;
        if (elems.empty()) throw RangeArgumentError("invalid argument: the container is not declared as planes of tensors");
        if (n_ranges && (!tensor || !first || !count)) throw RangeArgumentError("invalid argument: ranges without their arrays");
        const size_t K = n_ranges, T = elems.size();
        size_t B = 0;  // byte ranges: one per plane, and per piece touched, of every element range
        uint64_t sum = 0;
        bool delta = false;  // a range that has elements names a tensor with a base
        for (size_t k = 0; k < K; k++) {
            if (tensor[k] >= T)
                throw RangeArgumentError("invalid argument: range " + std::to_string(k) + " names tensor " + std::to_string(tensor[k]) + " of " +
                                         std::to_string(T));
            const uint64_t j = tensor[k];
            if (first[k] > counts[j] || count[k] > counts[j] - first[k])
                throw RangeArgumentError("invalid argument: range " + std::to_string(k) + " (tensor " + std::to_string(j) + ", first " +
                                         std::to_string(first[k]) + ", count " + std::to_string(count[k]) + ") does not lie in the " +
                                         std::to_string(counts[j]) + " elements");
            if (count[k] > ~(uint64_t)0 / elems[j]) throw RangeArgumentError("invalid argument: the ranges' lengths overflow 64 bits");
            const uint64_t bytes = count[k] * elems[j];
            if (sum + bytes < sum) throw RangeArgumentError("invalid argument: the ranges' lengths overflow 64 bits");
            sum += bytes;
            delta = delta || (bytes && !bases.empty() && bases[j]);
            if (!pieced) B += elems[j];
            else if (count[k]) B += elems[j] * (size_t)((first[k] + count[k] - 1) / psize[j] - first[k] / psize[j] + 1);  // (an empty range: none)
        }
        // off | len | prefix of the byte ranges, as RangeReader::run takes them; behind them the element ranges' columns (with
        // pieces: psize and pieces too; of a delta read: bslice last)
        const size_t x = 3 * B + 1, C = (pieced ? 7 : 5) + (delta ? 1 : 0);
        std::vector<uint64_t> up(x + C * K + (K + 1) / 2, 0);
        uint32_t* u_elem = (uint32_t*)(up.data() + x + C * K);
        const std::vector<uint64_t>& m_off = rd.member_offsets();  // (fetched by set_planes: no wait)
        uint64_t units = 0, at = 0, pre = 0;
        size_t b = 0;
        for (size_t k = 0; k < K; k++) {
            const uint64_t j = tensor[k];
            const uint32_t e = elems[j];
            up[x + k] = units;
            up[x + K + k] = first[k];
            up[x + 2 * K + k] = count[k];
            up[x + 3 * K + k] = first_m[j];
            up[x + 4 * K + k] = at;
            u_elem[k] = e;
            if (delta && count[k] && bases[j]) up[x + (C - 1) * K + k] = bases[j] + first[k] * e;
            units += ElementGather::units_of(first[k], count[k]);
            if (!pieced) {
                for (uint32_t p = 0; p < e; p++, b++) {
                    up[b] = m_off[first_m[j] + p] + first[k];
                    up[B + b] = count[k];
                    up[2 * B + b] = at + (uint64_t)p * count[k];
                }
            } else {
                const uint64_t S = psize[j], Q = pieces[j], end = first[k] + count[k];
                up[x + 5 * K + k] = S;
                up[x + 6 * K + k] = Q;
                const uint64_t q0 = first[k] / S, q1 = count[k] ? (end - 1) / S + 1 : q0;
                for (uint32_t p = 0; p < e; p++)
                    for (uint64_t q = q0; q < q1; q++, b++) {  // the range's part of piece q of plane p
                        const uint64_t lo = std::max(first[k], q * S), hi = std::min(end, (q + 1) * S);
                        up[b] = m_off[first_m[j] + p * Q + q] + (lo - q * S);
                        up[B + b] = hi - lo;
                        up[2 * B + b] = pre;
                        pre += hi - lo;
                    }
            }
            at += count[k] * e;
        }
        up[3 * B] = sum;
        dst_len = sum;
        st.out_bytes = sum;
        rd.check_destination(d_dst, d_cap, sum);
        if (sum == 0) {
            st.total_s = be.now() - t0;
            return;
        }
        if (delta) {
            const uint64_t d0 = (uint64_t)(uintptr_t)d_dst;
            for (size_t k = 0; k < K; k++) {
                const uint64_t s = up[x + (C - 1) * K + k], n = count[k] * elems[tensor[k]];
                if (!s || s + n <= d0 || s >= d0 + sum || s == d0 + up[x + 4 * K + k]) continue;
                throw RangeArgumentError("invalid argument: the base slice of range " + std::to_string(k) + " (tensor " + std::to_string(tensor[k]) +
                                         ") overlaps the output buffer other than as the range's own destination");
            }
        }
        rd.run(up, B, st, slots, t0, [&](const uint64_t* d_up, const uint64_t* d_place, const uint8_t* base) {
            const uint64_t* c = d_up + x;
            const ElementGather g{c, c + K, c + 2 * K, c + 3 * K, c + 4 * K, (const uint32_t*)(c + C * K), K, units, d_place, rd.status(), base, d_dst};
            if (delta && pieced) be.launch((size_t)units, ElementGatherDeltaPieces{ElementGatherDelta{g, c + 7 * K}, c + 5 * K, c + 6 * K});
            else if (delta) be.launch((size_t)units, ElementGatherDelta{g, c + 5 * K});
            else if (pieced) be.launch((size_t)units, ElementGatherPieces{g, c + 5 * K, c + 6 * K});
            else be.launch((size_t)units, g);
        });
    }
};

}  // namespace orz
