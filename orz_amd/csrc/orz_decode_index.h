// orz_decode_index.h -- members decoded from and into DEVICE memory: the framing index built on the device, and its driver.
//
// decode_members_device (orz_decode_device.h) indexes a host container with index_members and downloads the result.  Here the
// container may already lie in HBM -- as one concatenation, or as a table of (offset, length) entries in any order, which is
// what orz_members_encode_to_device writes -- and the output goes into a device buffer the caller owns.  The index is built by
// kernels that read the framing only (LEB128 chunk lengths, the census, each chunk's end field: the walk of index_members,
// restated for a lane) and must come to exactly what index_members comes to: the same verdict, the same begin / end /
// out_len / out_off.  The decode launches are DecodeMember's, unchanged, with `out` = the caller's buffer.
#pragma once
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "orz_decode_device.h"
#include "orz_decode_drive.h"

namespace orz {

enum : uint32_t {  // verdicts of the device index: one per message of index_members, two for the member table
    kIxOk = 0,
    kIxTruncatedLength,
    kIxChunkLength,
    kIxCensus,
    kIxEndField,
    kIxTooLong,       // a member of 4 GiB or more
    kIxTooDense,      // announces more output than its bits can code
    kIxTableRange,    // a table entry outside [0, n)
    kIxTableEnd,      // a table entry that does not end at its member's EOF byte
    kIxShortDestination  // (orz_decode_scatter.h) a member's own destination is smaller than the member
};

inline const char* index_message(uint32_t s) {
    switch (s) {
        case kIxTruncatedLength: return "invalid orz data: truncated chunk length";
        case kIxChunkLength: return "invalid orz data: chunk length";
        case kIxCensus: return "invalid orz data: census";
        case kIxEndField: return "invalid orz data: end field";
        case kIxTooLong: return "member of 4 GiB or more: use the host decoder";
        case kIxTooDense: return "member announces more output than its bits can code: use the host decoder";
        case kIxTableRange: return "invalid orz data: member table entry out of range";
        case kIxTableEnd: return "invalid orz data: member table entry does not end at its member's EOF byte";
        case kIxShortDestination: return "a member's destination is too small";
        default: return "invalid orz data: unknown index verdict";
    }
}

struct MemberWalk {
    uint64_t end;   // one past the member's EOF byte
    uint32_t len;   // decoded size its end fields announce
    uint32_t status;
};

// The framing of the member that starts at `at`, reading no byte at or past `lim`: index_members' loop body, verdict for verdict.
ORZ_HD MemberWalk walk_member(const uint8_t* src, uint64_t at, uint64_t lim) {
    const uint64_t begin = at;
    uint32_t spos_end = kPre;
    uint64_t slid = 0;
    bool first = true;
    for (;;) {
        uint64_t t = 0;
        for (uint32_t sh = 0;; sh += 7) {
            if (at >= lim || sh > 56) return MemberWalk{at, 0, kIxTruncatedLength};
            const uint8_t b = src[at++];
            t |= (uint64_t)(b & 0x7f) << sh;
            if (!(b & 0x80)) break;
        }
        if (t == 0) break;
        if (t >= (uint64_t)kPre * 3 || t > lim - at) return MemberWalk{at, 0, kIxChunkLength};
        DecodeMember::Bits br{src + at, (uint32_t)t, 0, 0, 0};
        bool bad = false;
        if (first) {
            const uint32_t k = br.varint(bad);
            if (bad || k > kSyms) return MemberWalk{at, 0, kIxCensus};
            for (uint32_t i = 0; i < k; i++) br.bits(9);
            first = false;
        }
        const uint32_t end_field = br.varint(bad);
        if (bad || end_field < spos_end || end_field > kBlock) return MemberWalk{at, 0, kIxEndField};
        spos_end = end_field;
        if (spos_end >= kBlock) {  // the decoder slides here (src/lib.rs:119-124)
            slid += kNewMax;
            spos_end = kPre;
            if (slid > 0xffffffffull - 2 * kNewMax) return MemberWalk{at, 0, kIxTooLong};
        }
        at += t;
    }
    const uint64_t mlen = (uint64_t)(spos_end - kPre) + slid;
    if (mlen > (at - begin) * 4096 + 4096) return MemberWalk{at, 0, kIxTooDense};
    return MemberWalk{at, (uint32_t)mlen, kIxOk};
}

struct IndexRecord {  // what the host reads back of an index: one record
    uint64_t members, total;
    uint64_t bad;     // first member whose verdict is not kIxOk
    uint32_t status;  // its verdict
    uint32_t pad;
};

// Concatenation: member boundaries are a serial chain, so ONE lane walks the framing.  Pass 1 (begin == nullptr) counts,
// sums and validates; pass 2 fills the arrays of the `cap` members pass 1 counted, out_off accumulating as it goes.
struct IndexConcat {
    const uint8_t* src;
    uint64_t n;
    uint64_t *begin, *end, *out_off;
    uint32_t *out_len, *status;
    uint64_t cap;
    IndexRecord* rec;
    ORZ_HD void operator()(size_t tid) const {
        if (tid != 0) return;
        uint64_t at = 0, m = 0, total = 0;
        while (at < n) {
            const MemberWalk w = walk_member(src, at, n);
            if (w.status != kIxOk) {
                *rec = IndexRecord{m, total, m, w.status, 0};
                return;
            }
            if (begin && m < cap) {
                begin[m] = at; end[m] = w.end; out_off[m] = total; out_len[m] = w.len; status[m] = kIxOk;
            }
            total += w.len;
            at = w.end;
            m++;
        }
        *rec = IndexRecord{m, total, m, kIxOk, 0};
    }
};

// Member table: one lane per member.  begin[] holds the entries' offsets and end[] their lengths on entry; the lane turns the
// length into the end and checks that the member's framing, read inside its entry, ends exactly there.
struct IndexTable {
    const uint8_t* src;
    uint64_t n;
    uint64_t *begin, *end;
    uint32_t *out_len, *status;
    uint64_t members;
    ORZ_HD void operator()(size_t k) const {
        if (k >= members) return;
        const uint64_t off = begin[k], len = end[k];
        out_len[k] = 0;
        if (off >= n || len > n - off) {
            end[k] = off;
            status[k] = kIxTableRange;
            return;
        }
        end[k] = off + len;
        const MemberWalk w = walk_member(src, off, off + len);
        status[k] = w.status != kIxOk ? w.status : (w.end != off + len ? (uint32_t)kIxTableEnd : (uint32_t)kIxOk);
        if (status[k] == kIxOk) out_len[k] = w.len;
    }
};

// One wavefront: the exclusive 64-bit prefix sum of out_len (totals exceed 4 GiB) into out_off, the total, and the first member
// whose verdict is not kIxOk, into the record.
struct IndexScan {
    const uint32_t* out_len;
    const uint32_t* status;
    uint64_t* out_off;
    uint64_t members;
    IndexRecord* rec;
    template <class W>
    ORZ_D static uint64_t shfl64(W& w, uint64_t v, uint32_t src) {
        return (uint64_t)w.shfl((uint32_t)v, src) | ((uint64_t)w.shfl((uint32_t)(v >> 32), src) << 32);
    }
    static size_t lds_bytes() { return 0; }
    template <class W>
    ORZ_D void operator()(W& w) const {
        const uint32_t lane = w.lane();
        uint64_t carry = 0, bad = members;
        uint32_t why = kIxOk;
        for (uint64_t base = 0; base < members; base += 64) {
            const uint64_t k = base + lane;
            const uint64_t v = k < members ? out_len[k] : 0;
            const uint32_t s = k < members ? status[k] : kIxOk;
            uint64_t x = v;  // inclusive scan across the wave (Hillis-Steele)
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint64_t y = shfl64(w, x, lane >= d ? lane - d : lane);
                if (lane >= d) x += y;
            }
            if (k < members) out_off[k] = carry + x - v;
            carry += shfl64(w, x, 63);
            const uint64_t bm = w.ballot(s != kIxOk);
            const uint32_t lead = bm ? (uint32_t)__builtin_ctzll(bm) : 0;
            const uint32_t s_lead = w.shfl(s, lead);
            if (bm) {  // (wave-uniform)
                bad = base + lead;
                why = s_lead;
                break;
            }
        }
        if (lane == 0) *rec = IndexRecord{members, carry, bad, why, 0};
    }
};

// Thrown when the caller's buffer is smaller than the decoded size (ORZ_ENOMEM at the C boundary).
struct DecodeCapacityError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// The device-built index of a container: one allocation holding begin | end | out_off (u64) | status | out_len (u32), so that
// out_off and status come back in one read.  Freed with the object.
template <class BE>
struct DeviceIndex {
    BE& be;
    uint64_t members = 0, total = 0;
    uint8_t* mem = nullptr;
    IndexRecord* rec = nullptr;
    uint64_t *begin = nullptr, *end = nullptr, *out_off = nullptr;
    uint32_t *status = nullptr, *out_len = nullptr;
    uint32_t host_waits = 0;
    explicit DeviceIndex(BE& b) : be(b) {}
    DeviceIndex(const DeviceIndex&) = delete;
    DeviceIndex& operator=(const DeviceIndex&) = delete;
    ~DeviceIndex() {
        if (mem) be.free(mem);
        if (rec) be.free(rec);
    }
    void arrays(uint64_t m) {
        mem = be.template alloc<uint8_t>((size_t)m * 32, false);
        begin = (uint64_t*)mem;
        end = begin + m;
        out_off = end + m;
        status = (uint32_t*)(out_off + m);
        out_len = status + m;
    }
    IndexRecord read_record() {
        IndexRecord r;
        be.d2h(&r, rec, sizeof r);
        host_waits++;
        return r;
    }
    static void check(const IndexRecord& r) {
        if (r.status != kIxOk) throw std::runtime_error(std::string(index_message(r.status)) + " (member " + std::to_string(r.bad) + ")");
    }

    // Concatenation (table == false) or member table (offs / lens: host arrays of `n_table` entries).  `want_arrays` = false:
    // a concatenation is counted and validated only (the sizing call without offsets).  Throws std::runtime_error naming the first
    // bad member.  Host waits: one read of the record, plus the upload of the table.
    void build(const uint8_t* d_src, size_t n, bool table, const uint64_t* offs, const uint64_t* lens, size_t n_table, bool want_arrays) {
        rec = be.template alloc<IndexRecord>(1);
        if (!table) {
            be.launch(1, IndexConcat{d_src, n, nullptr, nullptr, nullptr, nullptr, nullptr, 0, rec});
            const IndexRecord r = read_record();
            check(r);
            members = r.members;
            total = r.total;
            if (want_arrays && members) {
                arrays(members);
                be.launch(1, IndexConcat{d_src, n, begin, end, out_off, out_len, status, members, rec});
            }
            return;
        }
        members = n_table;
        arrays(members);
        if (members) {
            std::vector<uint64_t> up((size_t)members * 2);  // offsets into begin[], lengths into end[]: one upload
            std::copy(offs, offs + members, up.begin());
            std::copy(lens, lens + members, up.begin() + members);
            be.h2d(begin, up.data(), (size_t)members * 16);
            host_waits++;
            be.launch(members, IndexTable{d_src, n, begin, end, out_len, status, members});
        }
        be.launch_waves(1, IndexScan{out_len, status, out_off, members, rec}, IndexScan::lds_bytes());
        const IndexRecord r = read_record();
        check(r);
        total = r.total;
    }
};

// Decodes the members of `src` (n bytes: device memory when src_on_device, host memory otherwise, which is uploaded) into
// d_dst (d_cap bytes of device memory) in member order.  table: member k is the lens[k] bytes at src + offs[k]; otherwise src is
// one concatenation.  d_dst == nullptr with d_cap == 0 sizes only.  Sets dst_len / members, and out_offs (host, one entry a
// member) when not null.  Throws DecodeCapacityError when d_cap is short and std::runtime_error for malformed data, both before any
// decode launch when the index finds them.  Host waits (stats.host_waits): the upload of a host container and of a table as
// uploads always were, then ONE read of the index record and ONE read of the statuses (and offsets) after the decode launches;
// a sizing call that wants offsets of a concatenation reads them instead of the statuses.
struct DecodeToDeviceStats : DecodeStats {
    uint64_t host_waits = 0;
};
template <class BE>
void decode_members_to_device(BE& be, const uint8_t* src, size_t n, bool src_on_device, bool table, const uint64_t* offs,
                              const uint64_t* lens, size_t n_table, uint8_t* d_dst, size_t d_cap, uint64_t& dst_len,
                              uint64_t& members, uint64_t* out_offs, DecodeToDeviceStats& stats, uint32_t slots = 2048) {
    const double t0 = be.now();
    const bool sizing = d_dst == nullptr && d_cap == 0;
    if (src_on_device && n && d_cap && (const uint8_t*)d_dst < src + n && src < (const uint8_t*)d_dst + d_cap)
        throw std::runtime_error("invalid argument: the container and the output buffer overlap");
    DeviceBuffers<BE> own(be);  // the uploaded container and the decoder's state
    DeviceIndex<BE> ix(be);
    const uint8_t* d_src = open_container(own, ix, src, n, src_on_device, table, offs, lens, n_table, !sizing || out_offs != nullptr, members, stats);
    const uint64_t M = members;
    dst_len = ix.total;
    if (!sizing && d_cap < ix.total)
        throw DecodeCapacityError("output buffer of " + std::to_string(d_cap) + " bytes is too small for " + std::to_string(ix.total));
    if (!sizing && M)
        decode_all(be, DecodeArgs{d_src, ix.begin, ix.end, ix.out_off, ix.out_len, d_dst, nullptr, ix.status, 0, 0}, M, slots, own, stats);
    const bool want_status = !sizing && M;
    if (want_status || (out_offs && M)) {
        // out_off and status lie side by side: one read for either or both
        std::vector<uint8_t> back((size_t)M * 12);
        const size_t from = out_offs ? 0 : (size_t)M * 8, to = want_status ? (size_t)M * 12 : (size_t)M * 8;
        be.d2h(back.data() + from, (const uint8_t*)ix.out_off + from, to - from);
        stats.host_waits++;
        if (out_offs) std::memcpy(out_offs, back.data(), (size_t)M * 8);
        if (want_status) throw_first_bad((const uint32_t*)(back.data() + (size_t)M * 8), M);
    }
    stats.total_s = be.now() - t0;
}

}  // namespace orz
