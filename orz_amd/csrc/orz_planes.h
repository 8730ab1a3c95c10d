// orz_planes.h -- tensors as BYTE PLANES: plane p of a tensor of e-byte elements is byte p of every element.  Each plane is an
// ordinary member (an ordinary orz stream), so nothing in the format changes; what is new is the move between a tensor's
// interleaved bytes and its planes, and a decode driver that ends in that move.
//
// PlaneSplit / PlaneMerge are ONE launch for all tensors of a call, driven by a table on the device (PlaneTable: a column per
// field, one entry per tensor of element size 2, 4 or 8; tensors of single bytes need no move and are not in it).  A work unit
// is 16 consecutive elements of one tensor: 16 e interleaved bytes that are 16 bytes in each of the e planes.  A lane finds its
// tensor with last_at_or_below over the first-unit column (a prefix sum of the tensors' unit counts).  Planes lie `pitch` bytes
// apart, pitch = the element count rounded up to 16, in staging that starts at a multiple of 16: the plane side of every full
// unit is 16-byte aligned.  A full unit of a tensor whose interleaved address is a multiple of 16 too moves as e 16-byte loads,
// a byte shuffle in registers (v_perm_b32 on pairs of dwords: two levels of it transpose 4 x 4 bytes) and e 16-byte stores;
// the last partial unit of a tensor, and every unit of a tensor at another address, goes byte by byte.  No LDS, no scratch, no
// atomics.  The rule of DESIGN 2a holds: a lane writes the bytes of its own unit and no others -- the split the unit's 16 (or
// fewer) bytes of each plane, never the padding behind a plane's count; the merge the unit's 16 e (or fewer) interleaved bytes
// -- and reads only what an earlier launch or the caller wrote.
//
// decode_members_planes is the sixth driver of the device decoder (orz_decode_drive.h): decode_members_scatter's sequence with
// a plan of its own.  Destination j takes the next elems[j] members as its planes.  PlanePlan (one lane per member) points a
// member of a single-byte destination at the destination itself and every other member at its plane in a staging buffer, judges
// the capacities and fills the merge's table on the device; PlaneScan (one wavefront) turns the unit counts into the first-unit
// column and names the first short destination.  The decode launches are DecodeMember's; ONE PlaneMerge launch queued behind
// them writes the destinations, and the statuses are read once, after it.
//
// PIECES.  A member decodes on one lane, so a large tensor's planes may be cut: with a piece size of P elements (a multiple of
// the work unit) plane p of a tensor is Q = ceil(count / P) consecutive members, bytes [q P, min(count, (q + 1) P)) each, and the
// tensor's members are plane-major: plane 0's pieces 0 .. Q - 1, then plane 1's.  The format does not change -- a piece is a
// member -- and neither do split and merge: a plane's pieces lie and decode back to back in the plane's place in staging.  The
// driver takes pieces[j], the pieces per plane of destination j, beside elems[j]; without them every plane is one piece.
//
// DELTAS.  A tensor may be kept as the planes (and pieces) of tensor XOR base, the base being a tensor the reader already holds:
// PlaneSplitDelta / PlaneMergeDelta are the two moves with a column of base addresses, and the driver takes bases[j] beside
// elems[j] and pieces[j].  Nothing in the format says so: which tensors are deltas, and of what, travels beside the container.
#pragma once
#include <algorithm>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "orz_decode_index.h"
#include "orz_decode_drive.h"
#include "orz_decode_range.h"    // (last_at_or_below)
#include "orz_decode_scatter.h"  // (DecodeScatterStats)
#include "orz_crc.h"             // (the digests of a verified decode)

namespace orz {

constexpr uint32_t kPlaneUnit = 16;  // elements in a work unit = bytes of a plane a full unit moves

inline bool plane_elem_ok(uint32_t e) { return e == 1 || e == 2 || e == 4 || e == 8; }
ORZ_HD uint64_t plane_pitch(uint64_t count) { return (count + (kPlaneUnit - 1)) / kPlaneUnit * kPlaneUnit; }
ORZ_HD uint64_t plane_units(uint64_t count) { return (count + (kPlaneUnit - 1)) / kPlaneUnit; }

// The tensors of one launch, a column per field (device memory).  first[] ascends from 0; a tensor of no elements repeats its
// successor's first unit, so the search never lands on it.
struct PlaneTable {
    const uint64_t* first;   // [n] the tensor's first work unit
    const uint64_t* inter;   // [n] address of the interleaved bytes
    const uint64_t* plane0;  // [n] address of plane 0
    const uint64_t* pitch;   // [n] bytes from one plane to the next
    const uint64_t* count;   // [n] elements
    const uint32_t* elem;    // [n] element size: 2, 4 or 8
    uint64_t n;
};
constexpr size_t kPlaneRowBytes = 5 * 8 + 4;  // of one tensor, over all columns

// the columns of a table of n tensors inside one buffer of plane_table_bytes(n) bytes at `mem` (a multiple of 8)
inline size_t plane_table_bytes(uint64_t n) { return ((size_t)n * kPlaneRowBytes + 7) / 8 * 8; }
inline PlaneTable plane_table_at(void* mem, uint64_t n) {
    uint64_t* c = (uint64_t*)mem;
    return PlaneTable{c, c + n, c + 2 * n, c + 3 * n, c + 4 * n, (const uint32_t*)(c + 5 * n), n};
}

// v_perm_b32: byte k of the result is byte sel.k of the eight bytes {hi, lo} (0 .. 3 = lo's, 4 .. 7 = hi's)
ORZ_HD uint32_t plane_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int k = 0; k < 4; k++) r |= (uint32_t)((both >> (8 * ((sel >> (8 * k)) & 7))) & 0xFF) << (8 * k);
    return r;
#endif
}

// sixteen bytes of device memory at a multiple of 16, as four dwords.  On the device one 128-bit access in the GLOBAL address
// space (the table holds addresses as integers: a pointer made of one is generic, and its accesses would be flat ones), the
// value one vector from the shuffle to the store: stored as four scalars, the three element sizes' last stores were merged
// into a common tail of dword stores.
#if defined(__HIP_DEVICE_COMPILE__)
typedef uint32_t PlaneQuad __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) PlaneQuad* PlaneQuadPtr;
typedef __attribute__((address_space(1))) const PlaneQuad* PlaneQuadCPtr;
#endif
ORZ_HD void plane_load16(uint32_t* r, const uint8_t* s) {
#if defined(__HIP_DEVICE_COMPILE__)
    const PlaneQuad v = *(PlaneQuadCPtr)s;
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
#else
    __builtin_memcpy(r, s, 16);
#endif
}
ORZ_HD void plane_store16(uint8_t* d, const uint32_t* r) {
#if defined(__HIP_DEVICE_COMPILE__)
    const PlaneQuad v = {r[0], r[1], r[2], r[3]};
    *(PlaneQuadPtr)d = v;
#else
    __builtin_memcpy(d, r, 16);
#endif
}

// 4 x 4 bytes transposed: byte k of o[p] is byte p of (a, b, c, d)[k].  Its own inverse.
ORZ_HD void plane_transpose4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t& o0, uint32_t& o1, uint32_t& o2, uint32_t& o3) {
    const uint32_t ab_lo = plane_perm(b, a, 0x05010400u), ab_hi = plane_perm(b, a, 0x07030602u);  // a0 b0 a1 b1 | a2 b2 a3 b3
    const uint32_t cd_lo = plane_perm(d, c, 0x05010400u), cd_hi = plane_perm(d, c, 0x07030602u);
    o0 = plane_perm(cd_lo, ab_lo, 0x05040100u);
    o1 = plane_perm(cd_lo, ab_lo, 0x07060302u);
    o2 = plane_perm(cd_hi, ab_hi, 0x05040100u);
    o3 = plane_perm(cd_hi, ab_hi, 0x07060302u);
}

// One full unit, both sides at multiples of 16: w = the 4 E interleaved dwords (element i is dwords i E / 4 ...), pl = the planes'
// dwords, plane p's at pl[4 p .. 4 p + 3].
template <int E>
ORZ_HD void plane_unit_split(const uint8_t* inter, uint8_t* plane, uint64_t pitch) {
    uint32_t w[4 * E], pl[4 * E];
#pragma unroll
    for (int q = 0; q < E; q++) plane_load16(w + 4 * q, inter + 16 * q);
    if constexpr (E == 2) {
#pragma unroll
        for (int k = 0; k < 4; k++) {  // elements 4 k .. 4 k + 3 lie in w[2 k], w[2 k + 1]
            pl[k] = plane_perm(w[2 * k + 1], w[2 * k], 0x06040200u);
            pl[4 + k] = plane_perm(w[2 * k + 1], w[2 * k], 0x07050301u);
        }
    } else {
        constexpr int S = E / 4;  // dwords per element
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int h = 0; h < S; h++)  // dword h of elements 4 k .. 4 k + 3 -> dword k of planes 4 h .. 4 h + 3
                plane_transpose4(w[S * (4 * k) + h], w[S * (4 * k + 1) + h], w[S * (4 * k + 2) + h], w[S * (4 * k + 3) + h], pl[4 * (4 * h) + k],
                                 pl[4 * (4 * h + 1) + k], pl[4 * (4 * h + 2) + k], pl[4 * (4 * h + 3) + k]);
    }
#pragma unroll
    for (int p = 0; p < E; p++) plane_store16(plane + (uint64_t)p * pitch, pl + 4 * p);
}
// the merge's shuffle alone, in registers: 16 bytes of each of E planes (pl) into the 16 E interleaved bytes (w)
template <int E>
ORZ_HD void plane_merge_shuffle(const uint32_t (&pl)[4 * E], uint32_t (&w)[4 * E]) {
    if constexpr (E == 2) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            w[2 * k] = plane_perm(pl[4 + k], pl[k], 0x05010400u);
            w[2 * k + 1] = plane_perm(pl[4 + k], pl[k], 0x07030602u);
        }
    } else {
        constexpr int S = E / 4;
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int h = 0; h < S; h++)
                plane_transpose4(pl[4 * (4 * h) + k], pl[4 * (4 * h + 1) + k], pl[4 * (4 * h + 2) + k], pl[4 * (4 * h + 3) + k], w[S * (4 * k) + h],
                                 w[S * (4 * k + 1) + h], w[S * (4 * k + 2) + h], w[S * (4 * k + 3) + h]);
    }
}
template <int E>
ORZ_HD void plane_unit_merge(uint8_t* inter, const uint8_t* plane, uint64_t pitch) {
    uint32_t w[4 * E], pl[4 * E];
#pragma unroll
    for (int p = 0; p < E; p++) plane_load16(pl + 4 * p, plane + (uint64_t)p * pitch);
    plane_merge_shuffle<E>(pl, w);
#pragma unroll
    for (int q = 0; q < E; q++) plane_store16(inter + 16 * q, w + 4 * q);
}

// work unit u of the table: kMerge = planes -> interleaved, else interleaved -> planes
template <bool kMerge>
ORZ_HD void plane_move_unit(const PlaneTable& t, uint64_t units, uint64_t u) {
    if (u >= units || !t.n) return;
    const uint64_t j = last_at_or_below(t.first, t.n, u);
    const uint64_t at = (u - t.first[j]) * kPlaneUnit, count = t.count[j];  // the unit's first element
    if (at >= count) return;
    const uint32_t e = t.elem[j];
    const uint64_t pitch = t.pitch[j], left = count - at;
    uint8_t* const inter = (uint8_t*)(uintptr_t)t.inter[j] + at * e;
    uint8_t* const plane = (uint8_t*)(uintptr_t)t.plane0[j] + at;
    if (left >= kPlaneUnit && ((t.inter[j] | t.plane0[j] | pitch) & 15) == 0 && (e == 2 || e == 4 || e == 8)) {
        if (kMerge) {
            if (e == 2) plane_unit_merge<2>(inter, plane, pitch);
            else if (e == 4) plane_unit_merge<4>(inter, plane, pitch);
            else plane_unit_merge<8>(inter, plane, pitch);
        } else {
            if (e == 2) plane_unit_split<2>(inter, plane, pitch);
            else if (e == 4) plane_unit_split<4>(inter, plane, pitch);
            else plane_unit_split<8>(inter, plane, pitch);
        }
        return;
    }
    const uint32_t k = left < kPlaneUnit ? (uint32_t)left : kPlaneUnit;
    for (uint32_t p = 0; p < e; p++)
        for (uint32_t i = 0; i < k; i++) {
            if (kMerge) inter[(uint64_t)i * e + p] = plane[(uint64_t)p * pitch + i];
            else plane[(uint64_t)p * pitch + i] = inter[(uint64_t)i * e + p];
        }
}

// One lane per work unit: the tensors' interleaved bytes into their planes / the planes into the interleaved bytes.
struct PlaneSplit {
    PlaneTable t;
    uint64_t units;
    ORZ_HD void operator()(size_t u) const { plane_move_unit<false>(t, units, (uint64_t)u); }
};
struct PlaneMerge {
    PlaneTable t;
    uint64_t units;
    ORZ_HD void operator()(size_t u) const { plane_move_unit<true>(t, units, (uint64_t)u); }
};

// ------------------------------------------------------------------------------------------------ deltas against base tensors
// PlaneSplitDelta / PlaneMergeDelta are PlaneSplit / PlaneMerge with one more column: base[j], the address of a BASE tensor's
// interleaved bytes -- as many bytes as tensor j has, elements of the same size -- or 0 for none.  The split writes the planes of
// tensor XOR base, the merge writes planes XOR base: XOR is its own inverse, works byte by byte and commutes with the move, so the
// move between interleaved bytes and planes, which touches every byte once anyway, is where the base comes in.  An element size
// of 1 is a row here too (with a base its bytes are XORed on their way; the plain kernels have no such rows).  A row without a
// base moves as the plain kernels move it.  A full unit whose interleaved address, base address, plane address and pitch are
// all multiples of 16: e 16-byte loads of the tensor's (merge: the planes') bytes and e of the base's, ALL issued before the
// first store, the XOR on the 4 e dwords of the interleaved side -- before the shuffle in the split, behind it in the merge --
// and e 16-byte stores; every other unit goes byte by byte, each byte read just before it is written.  No LDS, no scratch, no
// atomics, and the rule of DESIGN 2a: a lane reads and writes its own unit only.  That makes the merge safe IN PLACE, base[j] ==
// the interleaved address: the lane has loaded its base bytes before it stores over them, and no other lane reads them.  The
// split never writes the padding behind a plane's count, the source or the base.
// The bodies are their own, not plane_move_unit with a parameter more: the plain kernels keep their code and registers.

// the split's shuffle alone, in registers: the 16 E interleaved bytes (w) into 16 bytes of each of E planes (pl)
template <int E>
ORZ_HD void plane_split_shuffle(const uint32_t (&w)[4 * E], uint32_t (&pl)[4 * E]) {
    if constexpr (E == 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) pl[k] = w[k];
    } else if constexpr (E == 2) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            pl[k] = plane_perm(w[2 * k + 1], w[2 * k], 0x06040200u);
            pl[4 + k] = plane_perm(w[2 * k + 1], w[2 * k], 0x07050301u);
        }
    } else {
        constexpr int S = E / 4;
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int h = 0; h < S; h++)
                plane_transpose4(w[S * (4 * k) + h], w[S * (4 * k + 1) + h], w[S * (4 * k + 2) + h], w[S * (4 * k + 3) + h], pl[4 * (4 * h) + k],
                                 pl[4 * (4 * h + 1) + k], pl[4 * (4 * h + 2) + k], pl[4 * (4 * h + 3) + k]);
    }
}
// One full unit with a base, all three sides at multiples of 16.
template <int E, bool kMerge>
ORZ_HD void plane_unit_delta(uint8_t* inter, const uint8_t* base, uint8_t* plane, uint64_t pitch) {
    uint32_t w[4 * E], b[4 * E], pl[4 * E];
    if constexpr (kMerge) {
#pragma unroll
        for (int p = 0; p < E; p++) plane_load16(pl + 4 * p, plane + (uint64_t)p * pitch);
#pragma unroll
        for (int q = 0; q < E; q++) plane_load16(b + 4 * q, base + 16 * q);
        if constexpr (E == 1) {
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = pl[k];
        } else {
            plane_merge_shuffle<E>(pl, w);
        }
#pragma unroll
        for (int k = 0; k < 4 * E; k++) w[k] ^= b[k];
#pragma unroll
        for (int q = 0; q < E; q++) plane_store16(inter + 16 * q, w + 4 * q);
    } else {
#pragma unroll
        for (int q = 0; q < E; q++) plane_load16(w + 4 * q, inter + 16 * q);
#pragma unroll
        for (int q = 0; q < E; q++) plane_load16(b + 4 * q, base + 16 * q);
#pragma unroll
        for (int k = 0; k < 4 * E; k++) w[k] ^= b[k];
        plane_split_shuffle<E>(w, pl);
#pragma unroll
        for (int p = 0; p < E; p++) plane_store16(plane + (uint64_t)p * pitch, pl + 4 * p);
    }
}

// work unit u of the table with the base column `bases` ([t.n] addresses, 0 = none)
template <bool kMerge>
ORZ_HD void plane_move_unit_delta(const PlaneTable& t, const uint64_t* bases, uint64_t units, uint64_t u) {
    if (u >= units || !t.n) return;
    const uint64_t j = last_at_or_below(t.first, t.n, u);
    const uint64_t at = (u - t.first[j]) * kPlaneUnit, count = t.count[j];  // the unit's first element
    if (at >= count) return;
    const uint32_t e = t.elem[j];
    const uint64_t pitch = t.pitch[j], left = count - at, b0 = bases[j];
    uint8_t* const inter = (uint8_t*)(uintptr_t)t.inter[j] + at * e;
    uint8_t* const plane = (uint8_t*)(uintptr_t)t.plane0[j] + at;
    const bool quads = left >= kPlaneUnit && ((t.inter[j] | t.plane0[j] | pitch | b0) & 15) == 0;
    if (!b0) {  // no base: as the plain kernels move it
        if (quads && (e == 2 || e == 4 || e == 8)) {
            if (kMerge) {
                if (e == 2) plane_unit_merge<2>(inter, plane, pitch);
                else if (e == 4) plane_unit_merge<4>(inter, plane, pitch);
                else plane_unit_merge<8>(inter, plane, pitch);
            } else {
                if (e == 2) plane_unit_split<2>(inter, plane, pitch);
                else if (e == 4) plane_unit_split<4>(inter, plane, pitch);
                else plane_unit_split<8>(inter, plane, pitch);
            }
            return;
        }
        const uint32_t k = left < kPlaneUnit ? (uint32_t)left : kPlaneUnit;
        for (uint32_t p = 0; p < e; p++)
            for (uint32_t i = 0; i < k; i++) {
                if (kMerge) inter[(uint64_t)i * e + p] = plane[(uint64_t)p * pitch + i];
                else plane[(uint64_t)p * pitch + i] = inter[(uint64_t)i * e + p];
            }
        return;
    }
    const uint8_t* const base = (const uint8_t*)(uintptr_t)b0 + at * e;
    if (quads && (e == 1 || e == 2 || e == 4 || e == 8)) {
        if (e == 1) plane_unit_delta<1, kMerge>(inter, base, plane, pitch);
        else if (e == 2) plane_unit_delta<2, kMerge>(inter, base, plane, pitch);
        else if (e == 4) plane_unit_delta<4, kMerge>(inter, base, plane, pitch);
        else plane_unit_delta<8, kMerge>(inter, base, plane, pitch);
        return;
    }
    const uint32_t k = left < kPlaneUnit ? (uint32_t)left : kPlaneUnit;
    for (uint32_t p = 0; p < e; p++)
        for (uint32_t i = 0; i < k; i++) {  // (in place the base byte IS the byte written: read first)
            const uint64_t a = (uint64_t)i * e + p;
            if (kMerge) inter[a] = (uint8_t)(plane[(uint64_t)p * pitch + i] ^ base[a]);
            else plane[(uint64_t)p * pitch + i] = (uint8_t)(inter[a] ^ base[a]);
        }
}

struct PlaneSplitDelta {
    PlaneTable t;
    const uint64_t* base;  // [t.n] the bases' addresses (0: none)
    uint64_t units;
    ORZ_HD void operator()(size_t u) const { plane_move_unit_delta<false>(t, base, units, (uint64_t)u); }
};
struct PlaneMergeDelta {
    PlaneTable t;
    const uint64_t* base;
    uint64_t units;
    ORZ_HD void operator()(size_t u) const { plane_move_unit_delta<true>(t, base, units, (uint64_t)u); }
};

// One tensor of a table the HOST makes (the encode side, where every size is known before anything is launched).
struct PlaneRow {
    uint64_t inter, plane0, count;
    uint32_t elem;
};
// The table of `rows` as one host image for ONE upload to `d_mem` (plane_table_bytes(rows.size()) bytes of device memory):
// returns the table as the kernels take it and sets `units`.
inline PlaneTable plane_table_image(const std::vector<PlaneRow>& rows, void* d_mem, std::vector<uint64_t>& image, uint64_t& units) {
    const uint64_t n = rows.size();
    image.assign(plane_table_bytes(n) / 8, 0);
    uint32_t* elem = (uint32_t*)(image.data() + 5 * n);
    units = 0;
    for (uint64_t j = 0; j < n; j++) {
        image[j] = units;
        image[n + j] = rows[j].inter;
        image[2 * n + j] = rows[j].plane0;
        image[3 * n + j] = plane_pitch(rows[j].count);
        image[4 * n + j] = rows[j].count;
        elem[j] = rows[j].elem;
        units += plane_units(rows[j].count);
    }
    return plane_table_at(d_mem, n);
}

// ------------------------------------------------------------------------------------------------ the decode driver
constexpr uint32_t kPlShortDestination = kIxShortDestination;

struct PlaneRecord {  // what the host reads back of a plan: one record, behind the members' sizes
    uint64_t dsts;
    uint64_t bad;    // first destination that is short (dsts when there is none)
    uint64_t units;  // of the merge
    uint32_t status;  // kIxOk or kIxShortDestination
    uint32_t pad;
};

// where destination j's planes lie in the staging buffer, from the index's prefix sum of the members' sizes (off0 = that of
// the destination's first member, number first_m): a multiple of 16, and far enough behind its predecessor's for e planes of
// whatever pitch -- e (count + 15) <= e count + 32 e - 15
ORZ_HD uint64_t plane_stage_at(uint64_t off0, uint64_t first_m) { return (off0 + 15) / 16 * 16 + 32 * first_m; }
// bytes of staging that always suffice for a container of `members` members that decode to `total` bytes
inline uint64_t plane_stage_bound(uint64_t total, uint64_t members) { return total + 32 * members + 16; }

// What the decoded sizes of the e Q members of one tensor (`what` number j, first member f, plane-major) must satisfy, size_of(m)
// being member m's: with Q > 1 the pieces of a plane are S bytes each, S = the first one's, a multiple of the work unit, but
// for the last, which has 1 .. S; and every plane is cut as plane 0 is.  Returns the tensor's elements, (Q - 1) S + the last
// piece; throws std::runtime_error naming the tensor and the first member that offends.
template <class SizeOf>
uint64_t plane_piece_count(const char* what, uint64_t j, uint64_t f, uint32_t e, uint64_t Q, const SizeOf& size_of) {
    const std::string who = std::string(what) + " " + std::to_string(j);
    const auto says = [&](uint64_t m) { return "member " + std::to_string(m) + " decodes to " + std::to_string(size_of(m)) + " bytes"; };
    const uint64_t S = size_of(f), last = size_of(f + Q - 1);
    if (Q > 1) {
        if (S % kPlaneUnit)
            throw std::runtime_error("invalid argument: the pieces of " + who + " are no multiple of " + std::to_string(kPlaneUnit) + " elements: " + says(f));
        for (uint64_t q = 1; q + 1 < Q; q++)
            if (size_of(f + q) != S)
                throw std::runtime_error("invalid argument: the pieces of " + who + " differ in size: " + says(f + q) + ", member " + std::to_string(f) +
                                         " to " + std::to_string(S));
        if (last == 0 || last > S)
            throw std::runtime_error("invalid argument: the last piece of " + who + " has not 1 .. " + std::to_string(S) + " bytes: " + says(f + Q - 1));
    }
    for (uint64_t r = Q; r < e * Q; r++)
        if (size_of(f + r) != size_of(f + r % Q))
            throw std::runtime_error("invalid argument: the planes of " + who + " differ in size: " + says(f + r) + ", member " + std::to_string(f + r % Q) +
                                     " to " + std::to_string(size_of(f + r % Q)));
    return (Q - 1) * S + last;
}

// One lane per member.  The member's destination j (the last whose first member is at or below m), plane p and piece q -- the
// destination's members are plane-major, Q = pieces[j] to a plane (pieces == nullptr: one) --; where its bytes go as an offset
// from `base` modulo 2^64: q S behind the destination itself for an element size of 1, else q S behind plane p of the
// destination's place in `stage`, S being the size of the destination's first member; its size for the host's one read.  The
// lane of a destination's first member judges the capacity against e x the plane's size, (Q - 1) S + the last piece in 64 bits
// (the host refuses pieces and planes of other sizes before it looks at the verdict) and fills the merge's row.
// plane_stage_at still leaves room when first_m counts pieces: the e Q members of destination j decode to e count bytes, so
// its successor's place lies at least e count + 32 e Q - 15 bytes behind its own, and e planes of pitch <= count + 15 end
// e count + 15 e bytes behind it -- 15 e + 15 <= 32 e Q for every Q >= 1; likewise the last one ends inside plane_stage_bound.
// DELTAS (`bases` not null; null for every other caller, for whom nothing here changes): bases[j] is the address of destination
// j's base, 0 for none.  A single-byte destination that has one cannot be decoded where it lies -- its bytes have to pass the
// merge, which XORs the base in -- so it is staged like the multi-byte ones: its members point at its place in staging, its
// units are plane_units(count) and its row has its count.  The room plane_stage_at leaves still suffices for e = 1: the
// inequality above reads 30 <= 32 Q.
struct PlanePlan {
    const uint64_t* dsts;     // [n_dsts] the destinations' addresses
    const uint64_t* caps;     // [n_dsts] their capacities
    const uint64_t* first_m;  // [n_dsts] their first members: the prefix sum of elems x pieces
    const uint32_t* elems;    // [n_dsts]
    const uint32_t* pieces;   // [n_dsts] pieces per plane (each >= 1), or nullptr: one
    uint64_t n_dsts;
    const uint64_t* ix_off;   // [members] the index's prefix sum of out_len
    const uint32_t* out_len;  // [members]
    uint64_t members;
    uint64_t base, stage;
    uint64_t* out_off;        // [members] out
    uint32_t* sizes;          // [members] out
    uint32_t* verdict;        // [n_dsts] out
    uint64_t* units;          // [n_dsts] out: the merge's units of the destination (0 for an element size of 1)
    uint64_t *t_inter, *t_plane0, *t_pitch, *t_count;  // [n_dsts] out: the merge's table but for its first-unit column
    uint32_t* t_elem;
    const uint64_t* bases = nullptr;  // [n_dsts] the bases' addresses (0: none), or nullptr: no deltas
    ORZ_HD void operator()(size_t m) const {
        if (m >= members) return;
        const uint64_t j = last_at_or_below(first_m, n_dsts, (uint64_t)m);
        const uint64_t f = first_m[j], r = (uint64_t)m - f, Q = pieces ? pieces[j] : 1;
        const uint64_t p = r / Q, q = r % Q;
        const uint32_t e = elems[j], len = out_len[m];
        const uint64_t S = out_len[f], count = (Q - 1) * S + out_len[f + Q - 1], pitch = plane_pitch(count);
        const uint64_t at = stage + plane_stage_at(ix_off[f], f);
        const bool direct = e == 1 && !(bases && bases[j]);  // decoded where it lies, no row in the merge
        out_off[m] = (direct ? dsts[j] : at + p * pitch) + q * S - base;
        sizes[m] = len;
        if (r) return;
        verdict[j] = count > ~(uint64_t)0 / e || caps[j] < count * e ? kPlShortDestination : (uint32_t)kIxOk;
        units[j] = direct ? 0 : plane_units(count);
        t_inter[j] = dsts[j];
        t_plane0[j] = at;
        t_pitch[j] = pitch;
        t_count[j] = direct ? 0 : count;
        t_elem[j] = e;
    }
};

// One wavefront: the exclusive prefix sum of the destinations' units into the merge's first-unit column, their total, and the
// first destination whose verdict is not kIxOk (IndexScan's scan and search).  A launch of its own: it reads what PlanePlan wrote.
struct PlaneScan {
    const uint64_t* units;
    const uint32_t* verdict;
    uint64_t* first;
    uint64_t n_dsts;
    PlaneRecord* rec;
    static size_t lds_bytes() { return 0; }
    template <class W>
    ORZ_D void operator()(W& w) const {
        const uint32_t lane = w.lane();
        uint64_t carry = 0, bad = n_dsts;
        uint32_t why = kIxOk;
        for (uint64_t at = 0; at < n_dsts; at += 64) {
            const uint64_t k = at + lane;
            const uint64_t v = k < n_dsts ? units[k] : 0;
            const uint32_t s = k < n_dsts ? verdict[k] : (uint32_t)kIxOk;
            uint64_t x = v;  // inclusive scan across the wave (Hillis-Steele)
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint64_t y = IndexScan::shfl64(w, x, lane >= d ? lane - d : lane);
                if (lane >= d) x += y;
            }
            if (k < n_dsts) first[k] = carry + x - v;
            carry += IndexScan::shfl64(w, x, 63);
            const uint64_t bm = w.ballot(s != kIxOk);
            const uint32_t lead = bm ? (uint32_t)__builtin_ctzll(bm) : 0;
            const uint32_t s_lead = w.shfl(s, lead);
            if (bm && bad == n_dsts) {  // (wave-uniform; the scan goes on: a refused call launches no merge, but the record is whole)
                bad = at + lead;
                why = s_lead;
            }
        }
        if (lane == 0) *rec = PlaneRecord{n_dsts, bad, carry, why, 0};
    }
};

// The bases of a delta decode may be read while the destinations are written.  `iv`: the destinations that have bytes as
// check_destinations left them, sorted by address and disjoint; bases[j]: the address of destination j's base (0: none), as
// many bytes as the destination's size, counts[j] x elems[j].  Throws std::runtime_error for the first destination, in index
// order, whose base wraps the address space, overlaps its own destination at another address than the destination's own (in
// place), or overlaps another destination's capacity.
inline void check_bases(const std::vector<std::pair<uint64_t, uint64_t>>& iv, const uint64_t* caps, const uint64_t* bases,
                        const std::vector<uint64_t>& counts, const uint32_t* elems) {
    const auto refuse = [](const std::string& what) { return std::runtime_error("invalid argument: " + what); };
    std::vector<uint64_t> dst_of(counts.size(), 0);
    for (const auto& d : iv) dst_of[(size_t)d.second] = d.first;
    for (uint64_t j = 0; j < counts.size(); j++) {
        const uint64_t b = bases[j], len = counts[j] * elems[j];
        if (!b || !len) continue;
        const std::string who = "the base of destination " + std::to_string(j);
        if (len > ~b) throw refuse(who + " wraps the address space");
        if (b == dst_of[(size_t)j]) continue;  // in place: inside its own destination, which overlaps no other
        // the destinations that begin below the base's end, from the last one down: their ends ascend with their addresses
        auto it = std::lower_bound(iv.begin(), iv.end(), std::make_pair(b + len, (uint64_t)0));
        if (it != iv.begin()) {
            const auto& d = *(it - 1);
            if (d.first + caps[d.second] > b)
                throw refuse(who + " overlaps destination " + std::to_string(d.second) + (d.second == j ? " at another address than its own" : ""));
        }
    }
}

// Decodes the members of `src` (n / src_on_device / table / offs / lens / n_table as for decode_members_scatter) into n_dsts
// destinations in device memory: destination j, d_caps[j] bytes at d_dsts[j], takes the next elems[j] members as the byte planes
// of elements of elems[j] bytes (1, 2, 4 or 8) -- with `pieces`, the next elems[j] x pieces[j] members, pieces[j] to a plane,
// plane-major.  out_lens[j] (when not null) = the destination's size, plane size x elems[j] (64 bits: a destination of many
// pieces may exceed 4 GiB though no member does); it is set also when the call fails for a short destination.  d_dsts == nullptr
// sizes only: nothing is decoded.  Sets `members`.
// Staging memory, freed before the call returns: at most the container's decoded size and 32 bytes a member
// (plane_stage_bound); none when every element size is 1.
// Throws, all before any decode launch and so before a byte of any destination is written:
//   std::runtime_error      what decode_members_scatter refuses of a container; an element size other than 1, 2, 4, 8; no pieces
//                           for a destination; the sum of elems x pieces different from the member count; planes of one
//                           destination of different decoded sizes, or pieces that plane_piece_count refuses (naming the
//                           destination and the first member that offends); a null destination that has bytes; two
//                           destinations that have bytes overlap (whole capacities count); one overlaps a device-resident container
//   DecodeCapacityError     a capacity below the destination's size, naming the first such destination
//   std::bad_alloc          no memory for the staging buffer
// and std::runtime_error naming the member after the launches when a member's payload is damaged: the destinations' content is
// unspecified then, but nothing outside [d_dsts[j], d_dsts[j] + out_lens[j]) has been written.
// Host waits (stats.host_waits): decode_members_scatter's for the same container, whatever the number of destinations and pieces -- the
// uploads of a host container and of a table, ONE read of the index record, ONE upload of destinations, capacities, first members,
// element sizes and pieces, ONE read of the plan's record with the sizes, ONE read of the statuses behind the merge: 4, 5 with a table
// or a host container, 6 with both.  A sizing call: the index's waits and one read of the sizes.
// VERIFIED (`check` not null; null for every other caller, for whom nothing here changes): the destinations' decoded bytes are
// held to the CRC-32 digests check->expect[j] (orz_crc.h).  Behind the merge -- behind the decode launches when nothing is merged
// -- ONE CrcPlan launch makes the digest table on the device from what the plan's upload holds, and CrcTiles, CrcFold and CrcSum run
// over the destinations: 4 launches more, whatever the number of destinations.  The digests come back in ONE additional read
// after the statuses (host waits: the above plus 1) and are compared here.  A member whose decode failed is reported first, as
// above; otherwise the first destination whose digest differs throws DecodeDigestError.  check->computed (when not null) is
// filled whenever the digest launches ran.  A sizing call verifies nothing; no digests for destinations is refused before any
// launch, and so is memory for the digests that cannot be had (std::bad_alloc).
// DELTAS (`bases` not null; null for every other caller, for whom nothing here changes): the members hold the planes of tensor XOR
// base, and bases[j] is the address of destination j's base in device memory -- as many bytes as the destination's size -- or 0 for
// none.  The bases go up as one more column of the plan's ONE upload, and that uploaded column is the merge's base column (the
// merge's rows are the destinations): ONE PlaneMergeDelta launch stands where PlaneMerge stood and XORs the bases in.  Launches
// and host waits are those of the same call without bases.  A base may BE its destination (the same address): the destination
// holds the base on entry and the tensor on return.  A destination of single bytes that has a base is staged (PlanePlan).  The
// digests of a verified call are the restored tensors', so a delta applied to another base is a digest mismatch.
// Refused in addition, before any decode launch, each naming the destination: a base that wraps the address space, one that
// overlaps its own destination at another address, one that overlaps another destination (whole capacities count).  Bases are
// only read: one may overlap the container or another base.  A base of a destination of no bytes is not looked at.
// After payload damage or a digest mismatch a base given out of place is untouched; a destination decoded in place holds
// neither its base nor its tensor.
template <class BE>
void decode_members_planes(BE& be, const uint8_t* src, size_t n, bool src_on_device, bool table, const uint64_t* offs, const uint64_t* lens,
                           size_t n_table, uint8_t* const* d_dsts, const uint64_t* d_caps, const uint32_t* elems, size_t n_dsts,
                           uint64_t* out_lens, uint64_t& members, DecodeScatterStats& stats, uint32_t slots = 2048,
                           const uint32_t* pieces = nullptr, const CrcCheck* check = nullptr, const uint64_t* bases = nullptr) {
    const double t0 = be.now();
    const bool sizing = d_dsts == nullptr;
    if (n_dsts && !elems) throw std::runtime_error("invalid argument: destinations without element sizes");
    if (check && !sizing && n_dsts && (!check->expect || !check->d_image)) throw std::runtime_error("invalid argument: destinations without digests");
    if (!sizing && n_dsts && !d_caps) throw std::runtime_error("invalid argument: destinations without capacities");
    const uint64_t J = n_dsts;
    std::vector<uint64_t> first_m((size_t)J + 1, 0);
    bool staged = false;
    for (uint64_t j = 0; j < J; j++) {
        if (!plane_elem_ok(elems[j]))
            throw std::runtime_error("invalid argument: destination " + std::to_string(j) + " has elements of " + std::to_string(elems[j]) +
                                     " bytes (1, 2, 4 or 8)");
        if (pieces && !pieces[j]) throw std::runtime_error("invalid argument: destination " + std::to_string(j) + " has no pieces");
        first_m[j + 1] = first_m[j] + (uint64_t)elems[j] * (pieces ? pieces[j] : 1);
        staged = staged || elems[j] > 1 || (bases && bases[j]);
    }
    DeviceBuffers<BE> own(be);  // the uploaded container, the plan, the staging buffer and the decoder's state
    DeviceIndex<BE> ix(be);
    const uint8_t* d_src = open_container(own, ix, src, n, src_on_device, table, offs, lens, n_table, true, members, stats);
    const uint64_t M = members;
    if (first_m[J] != M)
        throw std::runtime_error("invalid argument: " + std::to_string(first_m[J]) + (pieces ? " pieces of planes for " : " planes for ") +
                                 std::to_string(M) + " members");
    if (!M) {
        stats.total_s = be.now() - t0;
        return;
    }
    // planes of one destination of the same size, cut into pieces the same way, and the destinations' sizes
    std::vector<uint64_t> counts((size_t)J);
    const auto sizes_of = [&](const uint32_t* sizes) {
        for (uint64_t j = 0; j < J; j++)
            counts[j] = plane_piece_count("destination", j, first_m[j], elems[j], pieces ? pieces[j] : 1, [&](uint64_t m) { return (uint64_t)sizes[m]; });
        if (out_lens)
            for (uint64_t j = 0; j < J; j++) out_lens[j] = counts[j] * elems[j];
    };
    if (sizing) {
        std::vector<uint32_t> back((size_t)M);
        be.d2h(back.data(), ix.out_len, (size_t)M * 4);
        stats.host_waits++;
        sizes_of(back.data());
        stats.total_s = be.now() - t0;
        return;
    }
    uint8_t* stage = nullptr;
    if (staged) {
        try {
            stage = own.template alloc<uint8_t>((size_t)plane_stage_bound(ix.total, M), false);
        } catch (const std::exception&) {
            throw std::bad_alloc();
        }
        if (!stage) throw std::bad_alloc();
    }
    // the plan's memory, u64 columns first: dsts | caps | first_m | bases (of a delta call) | (ONE upload up to here, with elems and pieces at its end) out_off[M] |
    // units | table: first, inter, plane0, pitch, count | then u32: elems | table elem | verdict | sizes[M] | the record; sizes
    // and record are read back together
    const size_t up_cols = bases ? 4 : 3;
    const size_t up_words = (size_t)J * up_cols + ((size_t)J * (pieces ? 2 : 1) + 1) / 2;
    std::vector<uint64_t> up(up_words, 0);
    uint64_t base = (uint64_t)(uintptr_t)stage;
    for (uint64_t j = 0; j < J; j++) {
        up[j] = (uint64_t)(uintptr_t)d_dsts[j];
        up[J + j] = d_caps[j];
        up[2 * J + j] = first_m[j];
        if (bases) up[3 * J + j] = bases[j];
        if (!base) base = up[j];
    }
    std::memcpy(up.data() + up_cols * J, elems, (size_t)J * 4);
    if (pieces) std::memcpy((uint32_t*)(up.data() + up_cols * J) + J, pieces, (size_t)J * 4);
    const size_t off_at = up_words * 8, cols_at = off_at + (size_t)M * 8, u32_at = cols_at + (size_t)J * 6 * 8;
    const size_t sizes_at = u32_at + (size_t)J * 8, rec_at = (sizes_at + (size_t)M * 4 + 7) / 8 * 8;
    uint8_t* plan = own.template alloc<uint8_t>(rec_at + sizeof(PlaneRecord), false);
    uint64_t* p_dsts = (uint64_t*)plan;
    uint32_t* p_elems = (uint32_t*)(p_dsts + up_cols * J);
    const uint64_t* p_bases = bases ? p_dsts + 3 * J : nullptr;
    uint64_t* p_off = (uint64_t*)(plan + off_at);
    uint64_t* p_cols = (uint64_t*)(plan + cols_at);  // units | first | inter | plane0 | pitch | count
    uint32_t* p_telem = (uint32_t*)(plan + u32_at);
    uint32_t* p_verdict = p_telem + J;
    uint32_t* p_sizes = (uint32_t*)(plan + sizes_at);
    be.h2d(plan, up.data(), up_words * 8);
    stats.host_waits++;
    be.launch(M, PlanePlan{p_dsts, p_dsts + J, p_dsts + 2 * J, p_elems, pieces ? p_elems + J : nullptr, J, ix.out_off, ix.out_len, M, base, (uint64_t)(uintptr_t)stage, p_off, p_sizes,
                           p_verdict, p_cols, p_cols + 2 * J, p_cols + 3 * J, p_cols + 4 * J, p_cols + 5 * J, p_telem, p_bases});
    be.launch_waves(1, PlaneScan{p_cols, p_verdict, p_cols + J, J, (PlaneRecord*)(plan + rec_at)}, PlaneScan::lds_bytes());
    std::vector<uint8_t> back(rec_at + sizeof(PlaneRecord) - sizes_at);
    be.d2h(back.data(), plan + sizes_at, back.size());
    stats.host_waits++;
    const uint32_t* sizes = (const uint32_t*)back.data();
    PlaneRecord rec;
    std::memcpy(&rec, back.data() + (rec_at - sizes_at), sizeof rec);
    sizes_of(sizes);
    // the destinations that have bytes, by address: none null, none inside another, none inside the container
    std::vector<std::pair<uint64_t, uint64_t>> iv;  // (address, destination)
    for (uint64_t j = 0; j < J; j++)
        if (counts[j]) iv.emplace_back((uint64_t)(uintptr_t)d_dsts[j], j);
    check_destinations(iv, d_caps, src, n, src_on_device, DestinationNames{"no destination ", " for its planes", "destination ", "destinations "});
    if (bases) check_bases(iv, d_caps, bases, counts, elems);
    if (rec.status != kIxOk)
        throw DecodeCapacityError("destination " + std::to_string(rec.bad) + " holds " + std::to_string(d_caps[rec.bad]) + " bytes, too small for " +
                                  std::to_string(counts[rec.bad] * elems[rec.bad]));
    // the digests' memory, made before anything is launched: the table's columns first | addr | len, the tiles' residues, the digests
    uint64_t crc_tiles_all = 0;
    uint64_t* c_cols = nullptr;
    uint32_t *c_residue = nullptr, *c_crcs = nullptr;
    if (check) {
        for (uint64_t j = 0; j < J; j++) crc_tiles_all += crc_tiles((uint64_t)(uintptr_t)d_dsts[j], counts[j] * elems[j]);
        try {
            c_cols = own.template alloc<uint64_t>((size_t)J * 3, false);
            c_residue = own.template alloc<uint32_t>((size_t)crc_tiles_all, false);
            c_crcs = own.template alloc<uint32_t>((size_t)J, false);
        } catch (const std::exception&) {
            throw std::bad_alloc();
        }
    }
    decode_all(be, DecodeArgs{d_src, ix.begin, ix.end, p_off, ix.out_len, (uint8_t*)(uintptr_t)base, nullptr, ix.status, 0, 0}, M, slots, own, stats);
    // the merge, queued behind the decode launches on their stream: a plane whose decode failed is merged as whatever staging
    // holds -- bytes of the destination's own size, inside the destination
    const PlaneTable merge_t{p_cols + J, p_cols + 2 * J, p_cols + 3 * J, p_cols + 4 * J, p_cols + 5 * J, p_telem, J};
    if (rec.units && bases) be.launch((size_t)rec.units, PlaneMergeDelta{merge_t, p_bases, rec.units});
    else if (rec.units) be.launch((size_t)rec.units, PlaneMerge{merge_t, rec.units});
    if (check) {  // (a destination whose decode failed is digested as whatever it holds: bytes of its own size, inside it)
        be.launch_waves(1, CrcPlan{p_dsts, p_dsts + 2 * J, p_elems, pieces ? p_elems + J : nullptr, J, ix.out_len, c_cols, c_cols + J, c_cols + 2 * J},
                        CrcPlan::lds_bytes());
        crc_launches(be, CrcTable{c_cols, c_cols + J, c_cols + 2 * J, J}, crc_tiles_all, check->d_image, c_residue, c_crcs);
    }
    const std::vector<uint32_t> status = read_statuses(be, ix.status, M, stats.host_waits);
    std::vector<uint32_t> got;
    if (check) {
        got.resize((size_t)J);
        be.d2h(got.data(), c_crcs, (size_t)J * 4);
        stats.host_waits++;
        if (check->computed) std::memcpy(check->computed, got.data(), (size_t)J * 4);
    }
    throw_first_bad(status.data(), M);
    for (uint64_t j = 0; j < (check ? J : 0); j++)
        if (got[j] != check->expect[j]) throw DecodeDigestError(j, check->expect[j], got[j]);
    stats.total_s = be.now() - t0;
}

}  // namespace orz
