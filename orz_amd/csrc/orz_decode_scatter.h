// orz_decode_scatter.h -- members decoded each into a DESTINATION OF ITS OWN: the list-of-buffers twin of decode_members_to_device.
//
// decode_members_to_device (orz_decode_index.h) lays the members' bytes end to end in one buffer.  Here member k's bytes go to
// d_dsts[k], a device buffer of d_caps[k] bytes the caller owns (the tensors of a checkpoint, the pages of a table).  Nothing new
// decodes: the index is DeviceIndex's, the decode launches are DecodeMember's, and the only thing that changes is out_off[m], which
// DecodeArgs already allows to be "the member's address minus `out`, modulo 2^64".  ScatterPlan writes those offsets on the
// device, from ONE upload of the destinations, and holds each capacity against the size the index found; ScatterVerdict reduces
// the verdicts to the first short destination, so the host learns in one read whether it may launch.
#pragma once
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "orz_decode_index.h"
#include "orz_decode_drive.h"

namespace orz {

struct ScatterRecord {  // what the host reads back of a plan: one record, behind the sizes
    uint64_t members;
    uint64_t bad;     // first member whose destination is short (members when there is none)
    uint32_t status;  // kIxOk or kIxShortDestination
    uint32_t pad;
};

// One lane per member: where the member's bytes go, as an offset from `base` modulo 2^64 (base + out_off[m] == dsts[m] in 64-bit
// arithmetic, whichever of the two is the higher address), the verdict on its capacity, and its size next to the record for the
// host's one read.  A member of no bytes is never short and its offset is never used.
struct ScatterPlan {
    const uint64_t* dsts;     // [members] the destinations' addresses
    const uint64_t* caps;     // [members] their capacities
    const uint32_t* out_len;  // [members] the index's sizes
    uint64_t base;
    uint64_t* out_off;
    uint32_t* verdict;
    uint32_t* sizes;
    uint64_t members;
    ORZ_HD void operator()(size_t m) const {
        if (m >= members) return;
        const uint32_t len = out_len[m];
        out_off[m] = dsts[m] - base;
        verdict[m] = caps[m] < len ? (uint32_t)kIxShortDestination : (uint32_t)kIxOk;
        sizes[m] = len;
    }
};

// One wavefront: the first member whose verdict is not kIxOk, by ballot over 64 members at a time (IndexScan's search).  A launch
// of its own: it reads what ScatterPlan's launch wrote.
struct ScatterVerdict {
    const uint32_t* verdict;
    uint64_t members;
    ScatterRecord* rec;
    static size_t lds_bytes() { return 0; }
    template <class W>
    ORZ_D void operator()(W& w) const {
        const uint32_t lane = w.lane();
        uint64_t bad = members;
        uint32_t why = kIxOk;
        for (uint64_t at = 0; at < members; at += 64) {
            const uint64_t k = at + lane;
            const uint32_t s = k < members ? verdict[k] : (uint32_t)kIxOk;
            const uint64_t bm = w.ballot(s != kIxOk);
            const uint32_t lead = bm ? (uint32_t)__builtin_ctzll(bm) : 0;
            const uint32_t s_lead = w.shfl(s, lead);
            if (bm) {  // (wave-uniform)
                bad = at + lead;
                why = s_lead;
                break;
            }
        }
        if (lane == 0) *rec = ScatterRecord{members, bad, why, 0};
    }
};

struct DecodeScatterStats : DecodeStats {
    uint64_t host_waits = 0;
};

// Decodes the members of `src` (n / src_on_device / table / offs / lens / n_table as for decode_members_to_device), member k into
// the d_caps[k] bytes of device memory at d_dsts[k] (host arrays of n_dsts entries).  d_dsts == nullptr sizes only: out_lens
// receives the first min(n_dsts, members) decoded sizes and nothing is decoded.  Otherwise out_lens (when not null) receives all
// n_dsts of them, also when the call fails for a short destination.  Sets `members`.
// Throws, all before any decode launch and so before a byte of any destination is written:
//   std::runtime_error      malformed data (the index's message, naming the first bad member); n_dsts != members; a null
//                           destination of a member that has bytes; two destinations of members that have bytes overlap (their
//                           whole capacities count); a destination overlaps a device-resident container
//   DecodeCapacityError     a destination smaller than its member, naming the first such member
// and std::runtime_error naming the member after the launches when a member's payload is damaged.
// Host waits (stats.host_waits), a constant whatever the number of members: the upload of a host container and of a table as
// uploads always were, ONE read of the index record, ONE upload of destinations and capacities, ONE read of the plan's record
// with the sizes, ONE read of the statuses after the decode launches: 4, 5 with a table or a host container, 6 with both.  A
// sizing call: the index's waits and one read of the sizes.
template <class BE>
void decode_members_scatter(BE& be, const uint8_t* src, size_t n, bool src_on_device, bool table, const uint64_t* offs,
                            const uint64_t* lens, size_t n_table, uint8_t* const* d_dsts, const uint64_t* d_caps, size_t n_dsts,
                            uint64_t* out_lens, uint64_t& members, DecodeScatterStats& stats, uint32_t slots = 2048) {
    const double t0 = be.now();
    const bool sizing = d_dsts == nullptr;
    if (!sizing && n_dsts && !d_caps) throw std::runtime_error("invalid argument: destinations without capacities");
    DeviceBuffers<BE> own(be);  // the uploaded container, the plan and the decoder's state
    DeviceIndex<BE> ix(be);
    const uint8_t* d_src = open_container(own, ix, src, n, src_on_device, table, offs, lens, n_table, true, members, stats);
    const uint64_t M = members;
    if (sizing) {
        const uint64_t k = std::min<uint64_t>(M, out_lens ? n_dsts : 0);
        if (k) {
            std::vector<uint32_t> back((size_t)k);
            be.d2h(back.data(), ix.out_len, (size_t)k * 4);
            stats.host_waits++;
            std::copy(back.begin(), back.end(), out_lens);
        }
        stats.total_s = be.now() - t0;
        return;
    }
    if (n_dsts != M)
        throw std::runtime_error("invalid argument: " + std::to_string(n_dsts) + " destinations for " + std::to_string(M) + " members");
    if (!M) {
        stats.total_s = be.now() - t0;
        return;
    }
    // the plan's memory: dsts | caps (u64, ONE upload) | verdict | sizes (u32) | record, sizes and record read back together
    const size_t rec_at = ((size_t)M * 24 + 7) / 8 * 8;
    uint8_t* plan = own.template alloc<uint8_t>(rec_at + sizeof(ScatterRecord), false);
    uint64_t* p_dsts = (uint64_t*)plan;
    uint64_t* p_caps = p_dsts + M;
    uint32_t* p_verdict = (uint32_t*)(p_caps + M);
    uint32_t* p_sizes = p_verdict + M;
    uint64_t base = 0;
    {
        std::vector<uint64_t> up((size_t)M * 2);
        for (uint64_t m = 0; m < M; m++) {
            up[m] = (uint64_t)(uintptr_t)d_dsts[m];
            up[M + m] = d_caps[m];
            if (!base) base = up[m];
        }
        be.h2d(p_dsts, up.data(), (size_t)M * 16);
        stats.host_waits++;
    }
    uint8_t* const out = (uint8_t*)(uintptr_t)base;
    be.launch(M, ScatterPlan{p_dsts, p_caps, ix.out_len, base, ix.out_off, p_verdict, p_sizes, M});
    be.launch_waves(1, ScatterVerdict{p_verdict, M, (ScatterRecord*)(plan + rec_at)}, ScatterVerdict::lds_bytes());
    std::vector<uint8_t> back(rec_at + sizeof(ScatterRecord) - (size_t)M * 20);
    be.d2h(back.data(), (const uint8_t*)p_sizes, back.size());
    stats.host_waits++;
    const uint32_t* sizes = (const uint32_t*)back.data();
    ScatterRecord rec;
    std::memcpy(&rec, back.data() + (rec_at - (size_t)M * 20), sizeof rec);
    if (out_lens) std::copy(sizes, sizes + M, out_lens);
    // the destinations of members that have bytes, by address: none null, none inside another, none inside the container
    std::vector<std::pair<uint64_t, uint64_t>> iv;  // (address, member)
    for (uint64_t m = 0; m < M; m++)
        if (sizes[m]) iv.emplace_back((uint64_t)(uintptr_t)d_dsts[m], m);
    check_destinations(iv, d_caps, src, n, src_on_device, DestinationNames{"no destination for member ", "", "the destination of member ", "the destinations of members "});
    if (rec.status != kIxOk)
        throw DecodeCapacityError("the destination of member " + std::to_string(rec.bad) + " holds " + std::to_string(d_caps[rec.bad]) +
                                  " bytes, too small for " + std::to_string(sizes[rec.bad]));
    decode_all(be, DecodeArgs{d_src, ix.begin, ix.end, ix.out_off, ix.out_len, out, nullptr, ix.status, 0, 0}, M, slots, own, stats);
    throw_first_bad(read_statuses(be, ix.status, M, stats.host_waits).data(), M);
    stats.total_s = be.now() - t0;
}

}  // namespace orz
