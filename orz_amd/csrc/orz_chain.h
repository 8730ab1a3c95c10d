// orz_chain.h -- a CHAIN of XOR delta links restored in one decode and one merge launch.
//
// People keep deltas (orz_planes.h) as a chain: a keyframe every N steps and a delta per step against the step before.  A chain
// container is K LINKS one behind the other, each byte for byte a container the plane, piece or delta encode calls wrote for the
// same list of tensors -- the same element sizes and piece size, so the same elems, pieces and number of members M1 -- and so has
// M = K M1 members, link-major.  XOR is associative and commutes with the split into planes and pieces:
//     destination j = bases[j] XOR merge(planes of link 0, tensor j) XOR ... XOR merge(planes of link K - 1, tensor j)
// can be made in the plane domain, in the one launch that touches every byte anyway.  The order of the links does not matter to
// the result.  Without a base the result is the XOR of the links: a chain whose link 0 is a plain keyframe restores without one,
// and a chain of deltas alone yields the composed delta.  Nothing in the format says so: that a container is a chain, and of how
// many links, travels beside it as elems, pieces, bases and digests do.
//
// All links' members decode side by side in the same rounds -- members in flight are the only parallelism the device decoder has
// -- into K plane sets in staging; ONE PlaneMergeChain launch XORs the K plane sets and the base into the destinations; the
// digests of a verified call are those of the final tensors; the host waits are those of one call, whatever K is.
//
// The bodies are their own: PlaneMerge, PlaneMergeDelta, PlanePlan and the others keep their code and registers.
#pragma once
#include "orz_planes.h"

namespace orz {

// One full unit, every side at a multiple of 16: the base's e 16-byte loads FIRST (in place they are the bytes the lane stores
// over, and no other lane reads them), then e 16-byte loads per link, those of one link issued together, XORed into 4 e dwords of
// the PLANE domain; one shuffle, the XOR with the base's interleaved dwords, e 16-byte stores.  plane0 = the tensor's entry of
// link 0 in the plane0 column, whose link k entry lies k x `stride` entries behind it.
template <int E, bool kBase>
ORZ_HD void plane_unit_chain(uint8_t* inter, const uint8_t* base, const uint64_t* plane0, uint64_t stride, uint32_t links, uint64_t at,
                             uint64_t pitch) {
    uint32_t b[kBase ? 4 * E : 1], acc[4 * E], w[4 * E];
    if constexpr (kBase) {
#pragma unroll
        for (int q = 0; q < E; q++) plane_load16(b + 4 * q, base + 16 * q);
    }
#pragma unroll
    for (int i = 0; i < 4 * E; i++) acc[i] = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < links; k++) {
        const uint8_t* const plane = (const uint8_t*)(uintptr_t)plane0[(uint64_t)k * stride] + at;
        uint32_t pl[4 * E];
#pragma unroll
        for (int p = 0; p < E; p++) plane_load16(pl + 4 * p, plane + (uint64_t)p * pitch);
#pragma unroll
        for (int i = 0; i < 4 * E; i++) acc[i] ^= pl[i];
    }
    if constexpr (E == 1) {
#pragma unroll
        for (int i = 0; i < 4; i++) w[i] = acc[i];
    } else {
        plane_merge_shuffle<E>(acc, w);
    }
    if constexpr (kBase) {
#pragma unroll
        for (int i = 0; i < 4 * E; i++) w[i] ^= b[i];
    }
#pragma unroll
    for (int q = 0; q < E; q++) plane_store16(inter + 16 * q, w + 4 * q);
}

// One lane per work unit of 16 elements: PlaneMergeDelta over K plane sets.  The rows of `t` are the J destinations; t.plane0 has
// links x t.n entries, link-major: where link k keeps plane 0 of tensor j; the pitch is shared, every link having the tensor's
// count.  base[j]: the address of destination j's base, 0 for none.  The 16-byte path is taken by a full unit whose destination,
// base (if any), pitch and ALL K plane addresses are multiples of 16, for every element size, single bytes included; any other unit
// -- a partial last one, any address off 16, a single link's plane off 16 -- goes byte by byte, each base byte read just before
// the byte at the same index is written.  No LDS, no scratch, no atomics; a lane writes its own unit's bytes only and reads
// neither the padding behind a plane's count nor another unit's base bytes, so the merge is safe in place.
struct PlaneMergeChain {
    PlaneTable t;
    const uint64_t* base;  // [t.n]
    uint64_t units;
    uint32_t links;
    ORZ_HD void operator()(size_t unit) const {
        const uint64_t u = (uint64_t)unit;
        if (u >= units || !t.n) return;
        const uint64_t j = last_at_or_below(t.first, t.n, u);
        const uint64_t at = (u - t.first[j]) * kPlaneUnit, count = t.count[j];  // the unit's first element
        if (at >= count) return;
        const uint32_t e = t.elem[j];
        const uint64_t pitch = t.pitch[j], left = count - at, b0 = base[j];
        const uint64_t* const plane0 = t.plane0 + j;
        uint8_t* const inter = (uint8_t*)(uintptr_t)t.inter[j] + at * e;
        const uint8_t* const bs = (const uint8_t*)(uintptr_t)(b0 + at * e);  // (looked at only with a base)
        uint64_t low = t.inter[j] | pitch | b0;
        for (uint32_t k = 0; k < links; k++) low |= plane0[(uint64_t)k * t.n];
        if (left >= kPlaneUnit && (low & 15) == 0 && (e == 1 || e == 2 || e == 4 || e == 8)) {
            if (b0) {
                if (e == 1) plane_unit_chain<1, true>(inter, bs, plane0, t.n, links, at, pitch);
                else if (e == 2) plane_unit_chain<2, true>(inter, bs, plane0, t.n, links, at, pitch);
                else if (e == 4) plane_unit_chain<4, true>(inter, bs, plane0, t.n, links, at, pitch);
                else plane_unit_chain<8, true>(inter, bs, plane0, t.n, links, at, pitch);
            } else {
                if (e == 1) plane_unit_chain<1, false>(inter, bs, plane0, t.n, links, at, pitch);
                else if (e == 2) plane_unit_chain<2, false>(inter, bs, plane0, t.n, links, at, pitch);
                else if (e == 4) plane_unit_chain<4, false>(inter, bs, plane0, t.n, links, at, pitch);
                else plane_unit_chain<8, false>(inter, bs, plane0, t.n, links, at, pitch);
            }
            return;
        }
        const uint32_t n = left < kPlaneUnit ? (uint32_t)left : kPlaneUnit;
        for (uint32_t p = 0; p < e; p++)
            for (uint32_t i = 0; i < n; i++) {
                uint8_t v = 0;
                for (uint32_t k = 0; k < links; k++) v ^= ((const uint8_t*)(uintptr_t)plane0[(uint64_t)k * t.n])[at + (uint64_t)p * pitch + i];
                const uint64_t a = (uint64_t)i * e + p;
                if (b0) v ^= bs[a];  // (in place the base byte IS the byte written: read just before)
                inter[a] = v;
            }
    }
};

// PlanePlan's job for the M = K M1 members of K links, one lane per member.  Member m belongs to link k = m / M1; its (j, p, q)
// inside the link is found as PlanePlan finds it, from the destinations' first members WITHIN a link.  The pair (k, j) is a virtual
// destination whose first member is f = k M1 + first_m[j]: the member's place is q S behind plane p of plane_stage_at(ix_off[f], f)
// in staging, S and the pitch being those of (k, j)'s own members.  PlanePlan's disjointness argument holds unchanged: virtual
// destinations are just tensors in member order.  Every destination is staged, single-byte ones too: their bytes must pass the
// merge.  The lane of (k, j)'s first member writes plane0[k J + j]; that of (0, j)'s also judges the capacity and fills row j --
// link 0's sizes define the tensor (the host refuses a link whose tensor has another plane size before it looks at the verdict).
struct ChainPlan {
    const uint64_t* dsts;     // [n_dsts] the destinations' addresses
    const uint64_t* caps;     // [n_dsts] their capacities
    const uint64_t* first_m;  // [n_dsts] their first members within a link: the prefix sum of elems x pieces
    const uint32_t* elems;    // [n_dsts]
    const uint32_t* pieces;   // [n_dsts] pieces per plane (each >= 1)
    uint64_t n_dsts;
    const uint64_t* ix_off;   // [members] the index's prefix sum of out_len
    const uint32_t* out_len;  // [members]
    uint64_t members, link_members;  // M and M1
    uint64_t base, stage;
    uint64_t* out_off;        // [members] out
    uint32_t* sizes;          // [members] out
    uint32_t* verdict;        // [n_dsts] out
    uint64_t* units;          // [n_dsts] out: the merge's units of the destination
    uint64_t *t_inter, *t_pitch, *t_count;  // [n_dsts] out: the merge's rows but for the first-unit column
    uint64_t* t_plane0;       // [links x n_dsts] out, link-major
    uint32_t* t_elem;         // [n_dsts] out
    ORZ_HD void operator()(size_t lane) const {
        const uint64_t m = (uint64_t)lane;
        if (m >= members || !link_members) return;
        const uint64_t k = m / link_members, in_link = m % link_members;
        const uint64_t j = last_at_or_below(first_m, n_dsts, in_link);
        const uint64_t f = k * link_members + first_m[j], r = m - f, Q = pieces[j];
        const uint64_t p = r / Q, q = r % Q;
        const uint32_t e = elems[j];
        const uint64_t S = out_len[f], count = (Q - 1) * S + out_len[f + Q - 1], pitch = plane_pitch(count);
        const uint64_t at = stage + plane_stage_at(ix_off[f], f);
        out_off[m] = at + p * pitch + q * S - base;
        sizes[m] = out_len[m];
        if (r) return;
        t_plane0[k * n_dsts + j] = at;
        if (k) return;
        verdict[j] = count > ~(uint64_t)0 / e || caps[j] < count * e ? kPlShortDestination : (uint32_t)kIxOk;
        units[j] = plane_units(count);
        t_inter[j] = dsts[j];
        t_pitch[j] = pitch;
        t_count[j] = count;
        t_elem[j] = e;
    }
};

// decode_members_planes for a chain of `links` links: the arguments are that call's, `bases` may be null (no bases at all), and
// the M members of `src` are links x M1, M1 = sum(elems[j] x pieces[j]).  links == 1 IS decode_members_planes -- today's path with
// today's kernels.  With more links:
//   open_container; ONE upload (dsts, caps, first members, bases, elems, pieces); ChainPlan; PlaneScan; ONE read of the sizes with
//   the record; the checks; decode_all over all M members; ONE PlaneMergeChain; with digests CrcPlan and the three CRC launches over
//   the destinations, their lengths from link 0; the statuses; the digests.
// Host waits and launches are those of decode_members_planes for a container of the same M members, whatever `links` is.
// Staging memory, freed before the call returns: plane_stage_bound(total, M) -- `links` times the tensors' bytes.
// Throws, all before any decode launch and so before a byte of any destination is written:
//   std::runtime_error      no links; links x M1 different from the member count ("K links of M1 members for M members"); what
//                           decode_members_planes refuses of element sizes and pieces; per link what plane_piece_count refuses,
//                           naming the link and the member; a tensor that decodes to another plane size in link k than in link 0,
//                           naming k, the destination and both sizes; what check_destinations and check_bases refuse
//   DecodeCapacityError     a capacity below the destination's size, naming the first such destination
//   std::bad_alloc          no memory for the staging buffer or the digests
// and after the launches what decode_members_planes throws with bases: a damaged member is named first, then the first destination
// whose digest differs.  After such a failure a base given out of place is untouched; a destination restored in place holds
// neither its base nor its tensor.
template <class BE>
void decode_members_chain(BE& be, const uint8_t* src, size_t n, bool src_on_device, bool table, const uint64_t* offs, const uint64_t* lens,
                          size_t n_table, uint8_t* const* d_dsts, const uint64_t* d_caps, const uint32_t* elems, size_t n_dsts, uint64_t* out_lens,
                          uint64_t& members, DecodeScatterStats& stats, uint32_t slots, const uint32_t* pieces, const CrcCheck* check,
                          const uint64_t* bases, uint32_t links) {
    if (!links) throw std::runtime_error("invalid argument: a chain of 0 links");
    if (links == 1) {
        decode_members_planes(be, src, n, src_on_device, table, offs, lens, n_table, d_dsts, d_caps, elems, n_dsts, out_lens, members, stats, slots,
                              pieces, check, bases);
        return;
    }
    const double t0 = be.now();
    const bool sizing = d_dsts == nullptr;
    if (n_dsts && !elems) throw std::runtime_error("invalid argument: destinations without element sizes");
    if (check && !sizing && n_dsts && (!check->expect || !check->d_image)) throw std::runtime_error("invalid argument: destinations without digests");
    if (!sizing && n_dsts && !d_caps) throw std::runtime_error("invalid argument: destinations without capacities");
    const uint64_t J = n_dsts, K = links;
    std::vector<uint64_t> first_m((size_t)J + 1, 0);
    for (uint64_t j = 0; j < J; j++) {
        if (!plane_elem_ok(elems[j]))
            throw std::runtime_error("invalid argument: destination " + std::to_string(j) + " has elements of " + std::to_string(elems[j]) +
                                     " bytes (1, 2, 4 or 8)");
        if (pieces && !pieces[j]) throw std::runtime_error("invalid argument: destination " + std::to_string(j) + " has no pieces");
        first_m[j + 1] = first_m[j] + (uint64_t)elems[j] * (pieces ? pieces[j] : 1);
    }
    DeviceBuffers<BE> own(be);  // the uploaded container, the plan, the staging buffer and the decoder's state
    DeviceIndex<BE> ix(be);
    const uint8_t* d_src = open_container(own, ix, src, n, src_on_device, table, offs, lens, n_table, true, members, stats);
    const uint64_t M = members, M1 = first_m[J];
    if (M1 ? (M % M1 || M / M1 != K) : M != 0)
        throw std::runtime_error("invalid argument: " + std::to_string(K) + " links of " + std::to_string(M1) + " members for " + std::to_string(M) +
                                 " members");
    if (!M) {
        stats.total_s = be.now() - t0;
        return;
    }
    // every link cut as plane_piece_count asks, every tensor of the plane size it has in link 0, and the destinations' sizes
    std::vector<uint64_t> counts((size_t)J);
    const auto sizes_of = [&](const uint32_t* sizes) {
        for (uint64_t k = 0; k < K; k++) {
            const std::string what = k ? "link " + std::to_string(k) + "'s destination" : std::string("destination");
            for (uint64_t j = 0; j < J; j++) {
                const uint64_t c = plane_piece_count(what.c_str(), j, k * M1 + first_m[j], elems[j], pieces ? pieces[j] : 1,
                                                     [&](uint64_t m) { return (uint64_t)sizes[m]; });
                if (!k) counts[j] = c;
                else if (c != counts[j])
                    throw std::runtime_error("invalid argument: link " + std::to_string(k) + " has planes of " + std::to_string(c) + " bytes for destination " +
                                             std::to_string(j) + ", link 0 of " + std::to_string(counts[j]));
            }
        }
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
    try {
        stage = own.template alloc<uint8_t>((size_t)plane_stage_bound(ix.total, M), false);
    } catch (const std::exception&) {
        throw std::bad_alloc();
    }
    if (!stage) throw std::bad_alloc();
    // the plan's memory, u64 columns first: dsts | caps | first_m | bases | (u32) elems | pieces (ONE upload up to here) | out_off[M] |
    // units | table: first, inter, pitch, count, plane0[K J] | then u32: table elem | verdict | sizes[M] | the record; sizes and
    // record are read back together
    const size_t up_words = (size_t)J * 5;
    std::vector<uint64_t> up(up_words, 0);
    for (uint64_t j = 0; j < J; j++) {
        up[j] = (uint64_t)(uintptr_t)d_dsts[j];
        up[J + j] = d_caps[j];
        up[2 * J + j] = first_m[j];
        up[3 * J + j] = bases ? bases[j] : 0;
        ((uint32_t*)(up.data() + 4 * J))[j] = elems[j];
        ((uint32_t*)(up.data() + 4 * J))[J + j] = pieces ? pieces[j] : 1;
    }
    const uint64_t base = (uint64_t)(uintptr_t)stage;
    const size_t off_at = up_words * 8, cols_at = off_at + (size_t)M * 8, u32_at = cols_at + (size_t)J * (5 + K) * 8;
    const size_t sizes_at = u32_at + (size_t)J * 8, rec_at = (sizes_at + (size_t)M * 4 + 7) / 8 * 8;
    uint8_t* plan = own.template alloc<uint8_t>(rec_at + sizeof(PlaneRecord), false);
    uint64_t* p_dsts = (uint64_t*)plan;
    const uint64_t* p_bases = p_dsts + 3 * J;
    uint32_t* p_elems = (uint32_t*)(p_dsts + 4 * J);
    uint64_t* p_off = (uint64_t*)(plan + off_at);
    uint64_t* p_cols = (uint64_t*)(plan + cols_at);  // units | first | inter | pitch | count | plane0[K J]
    uint32_t* p_telem = (uint32_t*)(plan + u32_at);
    uint32_t* p_verdict = p_telem + J;
    uint32_t* p_sizes = (uint32_t*)(plan + sizes_at);
    be.h2d(plan, up.data(), up_words * 8);
    stats.host_waits++;
    be.launch(M, ChainPlan{p_dsts, p_dsts + J, p_dsts + 2 * J, p_elems, p_elems + J, J, ix.out_off, ix.out_len, M, M1, base, base, p_off, p_sizes, p_verdict,
                           p_cols, p_cols + 2 * J, p_cols + 3 * J, p_cols + 4 * J, p_cols + 5 * J, p_telem});
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
    const PlaneTable merge_t{p_cols + J, p_cols + 2 * J, p_cols + 5 * J, p_cols + 3 * J, p_cols + 4 * J, p_telem, J};
    if (rec.units) be.launch((size_t)rec.units, PlaneMergeChain{merge_t, p_bases, rec.units, links});
    if (check) {  // (the lengths are link 0's: its members are the container's first M1)
        be.launch_waves(1, CrcPlan{p_dsts, p_dsts + 2 * J, p_elems, p_elems + J, J, ix.out_len, c_cols, c_cols + J, c_cols + 2 * J}, CrcPlan::lds_bytes());
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
