// orz_decode_range.h -- byte ranges of the DECODED data of a members container that lies in device memory.
//
// decode_members_to_device (orz_decode_index.h) can do one thing with a container: decode all of it, at one lane's speed per
// member.  Members are independent, the device index knows every member's decoded offset and length from the framing alone,
// and decoding is causal: the first k bytes of a member need only the items that start before k.  So a reader indexes a
// container once (DeviceIndex, unchanged) and a read costs what the bytes asked for cost: only the members a range touches are
// decoded, each once a call and only as far as the furthest byte asked of it (DecodeArgs::stop), into a scratch arena, and
// one kernel over the DESTINATION bytes copies the ranges out of the arena, back to back in range order.
//
// One read is  upload of the ranges -> clear -> RangePlan -> RangeCompact -> [host reads one record] -> DecodeMember launches ->
// RangeGather -> [host reads stops, statuses and what was produced]: the upload and two reads, however many ranges.  The rule of
// DESIGN.md 2a holds: a thread acts only on state that an earlier launch wrote (stop[] is cleared before RangePlan raises it,
// with atomic maxima, whose result does not depend on the order of the lanes).
#pragma once
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "orz_decode_index.h"
#include "orz_kernels.h"  // (ORZ_ATOMIC_MAX)

namespace orz {

// the last k with a[k] <= x in the ascending a[0 .. n), n >= 1 and a[0] <= x.  Entries of length zero repeat their successor's
// offset, so the last of equals is the one that holds bytes.
ORZ_HD uint64_t last_at_or_below(const uint64_t* a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;  // a[lo] <= x < a[hi] (a[n] = infinity)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// sixteen bytes at addresses that are multiples of 16
ORZ_HD void copy16(uint8_t* d, const uint8_t* s) {
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
#else
    __builtin_memcpy(d, s, 16);
#endif
}

// One lane per range: every member the range touches must be decoded up to the range's end, or to its own.
struct RangePlan {
    const uint64_t *off, *len;  // [n_ranges], validated by the host: off + len <= total
    uint64_t n_ranges;
    const uint64_t* out_off;    // [members]
    const uint32_t* out_len;
    uint64_t members;
    uint32_t* stop;             // [members], zero on entry
    ORZ_HD void operator()(size_t k) const {
        if (k >= n_ranges || len[k] == 0) return;
        const uint64_t from = off[k], to = from + len[k];
        for (uint64_t m = last_at_or_below(out_off, members, from); m < members && out_off[m] < to; m++) {
            if (out_len[m] == 0) continue;
            const uint64_t mend = out_off[m] + out_len[m];
            ORZ_ATOMIC_MAX(&stop[m], (uint32_t)((to < mend ? to : mend) - out_off[m]));
        }
    }
};

struct RangeRecord {  // what the host reads back of a plan
    uint64_t needed;         // members with a stop
    uint64_t scratch_bytes;  // of the arena that holds their prefixes
};

// One wavefront: the members with a stop in member order, and each one's place in the scratch arena (its stop rounded up to 16:
// the arena's pieces start at multiples of 16).  Ballots for the list, a 64-bit prefix sum in the style of IndexScan for the places.
struct RangeCompact {
    const uint32_t* stop;
    uint64_t members;
    uint32_t* list;       // [members] out: the needed members
    uint64_t* arena_off;  // [members] out: where a needed member's bytes go in the arena
    RangeRecord* rec;
    static size_t lds_bytes() { return 0; }
    template <class W>
    ORZ_D void operator()(W& w) const {
        const uint32_t lane = w.lane();
        uint64_t count = 0, bytes = 0;
        for (uint64_t base = 0; base < members; base += 64) {
            const uint64_t k = base + lane;
            const uint32_t s = k < members ? stop[k] : 0;
            const uint64_t v = ((uint64_t)s + 15) & ~(uint64_t)15;
            uint64_t x = v;  // inclusive scan across the wave (Hillis-Steele)
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint64_t y = IndexScan::shfl64(w, x, lane >= d ? lane - d : lane);
                if (lane >= d) x += y;
            }
            const uint64_t need = w.ballot(s != 0);
            if (s != 0) {
                list[count + (uint64_t)__builtin_popcountll(need & (((uint64_t)1 << lane) - 1))] = (uint32_t)k;
                arena_off[k] = bytes + x - v;
            }
            bytes += IndexScan::shfl64(w, x, 63);
            count += (uint64_t)__builtin_popcountll(need);
        }
        if (lane == 0) *rec = RangeRecord{count, bytes};
    }
};

// One lane per sixteen bytes of the destination, cut at the destination's multiples of 16: the lane finds its range in the
// prefix of the lengths and its member in out_off, and copies from the arena -- sixteen bytes a load and a store where the piece
// covers the lane's unit and source and destination are co-aligned, bytes otherwise.  A range that spans members is several
// pieces; pieces of a member whose decode failed are skipped.
struct RangeGather {
    const uint64_t *off, *prefix;  // [n_ranges], [n_ranges + 1]: prefix[k] = sum of len[0 .. k)
    uint64_t n_ranges;
    const uint64_t *out_off, *arena_off;
    const uint32_t *out_len, *status;
    uint64_t members;
    const uint8_t* arena;
    uint8_t* dst;
    uint64_t dst_len;  // prefix[n_ranges]
    uint32_t head;     // dst's address modulo 16
    static uint64_t units(uint64_t dst_len, uint32_t head) { return (dst_len + head + 15) / 16; }
    ORZ_HD void operator()(size_t u) const {
        const uint64_t u0 = (uint64_t)u * 16;
        uint64_t pos = u0 > head ? u0 - head : 0;
        const uint64_t hi = u0 + 16 - head < dst_len ? u0 + 16 - head : dst_len;
        if (pos >= hi) return;
        uint64_t r = last_at_or_below(prefix, n_ranges, pos);
        while (pos < hi) {
            const uint64_t g = off[r] + (pos - prefix[r]);  // offset in the decoded data
            const uint64_t m = last_at_or_below(out_off, members, g);
            const uint64_t in_m = g - out_off[m];
            uint64_t end = prefix[r + 1] < hi ? prefix[r + 1] : hi;
            if (out_len[m] - in_m < end - pos) end = pos + (out_len[m] - in_m);
            if (status[m] == kDecOk) {
                const uint8_t* s = arena + arena_off[m] + in_m;
                uint8_t* d = dst + pos;
                if (end - pos == 16 && (((uintptr_t)s | (uintptr_t)d) & 15) == 0) copy16(d, s);
                else for (uint64_t i = 0; i < end - pos; i++) d[i] = s[i];
            }
            pos = end;
            while (r + 1 < n_ranges && prefix[r + 1] <= pos) r++;
        }
    }
};

struct RangeReadStats {
    uint64_t ranges = 0, members_decoded = 0, decoded_bytes = 0, out_bytes = 0, launches = 0, host_waits = 0;
    double kernel_ms = 0, gather_ms = 0, total_s = 0;
};

// Thrown for what the caller got wrong (ORZ_EINVAL before anything reaches the device).
struct RangeArgumentError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// A container, indexed once, that serves reads of byte ranges of its decoded data.  A host container is uploaded and owned; a
// device container is borrowed.  Everything a read needs on the device is kept and only ever grows; a growth that fails leaves
// the reader as it was (all or nothing, one buffer at a time: each is replaced only after its successor exists).  Reads are
// serial: NOT thread-safe.
template <class BE>
struct RangeReader {
    BE& be;
    DeviceIndex<BE> ix;
    const uint8_t* d_src = nullptr;
    size_t n = 0;
    uint8_t* owned_src = nullptr;
    uint64_t open_waits = 0;
    // per member: stop | status | produced (u32 each, side by side: one clear, one read), list (u32), arena_off (u64)
    uint8_t* plan = nullptr;
    RangeRecord* rec = nullptr;
    uint64_t* d_ranges = nullptr;  // off | len | prefix
    size_t ranges_cap = 0;
    uint8_t* arena = nullptr;
    size_t arena_cap = 0;
    uint8_t* state = nullptr;
    uint32_t state_slots = 0;
    std::vector<uint64_t> h_off;  // (orz_reader_info: read once, on demand)

    RangeReader(BE& b, const uint8_t* src, size_t n_, bool src_on_device, bool table, const uint64_t* offs, const uint64_t* lens,
                size_t n_table)
        : be(b), ix(b), n(n_) {
        try {
            d_src = src;
            if (!src_on_device) {
                owned_src = be.template alloc<uint8_t>(n, false);
                be.h2d(owned_src, src, n);
                open_waits++;
                d_src = owned_src;
            }
            ix.build(d_src, n, table, offs, lens, n_table, true);
            open_waits += ix.host_waits;
            if (ix.members) {
                plan = be.template alloc<uint8_t>((size_t)ix.members * 24);
                rec = be.template alloc<RangeRecord>(1);
            }
        } catch (...) {
            release();
            throw;
        }
    }
    RangeReader(const RangeReader&) = delete;
    RangeReader& operator=(const RangeReader&) = delete;
    ~RangeReader() { release(); }
    void release() {
        for (void* p : {(void*)owned_src, (void*)plan, (void*)rec, (void*)d_ranges, (void*)arena, (void*)state})
            if (p) be.free(p);
        owned_src = plan = arena = state = nullptr;
        rec = nullptr;
        d_ranges = nullptr;
    }
    uint32_t* stop() const { return (uint32_t*)plan; }
    uint32_t* status() const { return stop() + ix.members; }
    uint32_t* produced() const { return status() + ix.members; }
    uint32_t* list() const { return produced() + ix.members; }
    uint64_t* arena_off() const { return (uint64_t*)(list() + ix.members); }  // (16 M bytes in: a multiple of 8)

    const std::vector<uint64_t>& member_offsets() {
        if (h_off.size() != ix.members) {
            h_off.resize(ix.members);
            if (ix.members) be.d2h(h_off.data(), ix.out_off, (size_t)ix.members * 8);
        }
        return h_off;
    }

    template <class T>
    void grow(T*& p, size_t& cap, size_t want, bool zero) {
        if (want <= cap) return;
        T* q = be.template alloc<T>(want, zero);  // (throws: the old buffer stands)
        if (!q) throw std::bad_alloc();
        if (p) be.free(p);
        p = q;
        cap = want;
    }

    // Ranges [off[k], off[k] + len[k]) of the decoded data, written back to back in range order at d_dst.  dst_len = the sum of the
    // lengths whenever the ranges are valid.  Throws RangeArgumentError (bad ranges, overlap: nothing has reached the device),
    // DecodeCapacityError (d_cap short: nothing written) and std::runtime_error naming the first member whose payload is damaged
    // before its stop.
    void read(const uint64_t* off, const uint64_t* len, size_t n_ranges, uint8_t* d_dst, size_t d_cap, uint64_t& dst_len,
              RangeReadStats& st, uint32_t slots = 2048) {
        const double t0 = be.now();
        st = RangeReadStats{};
        st.ranges = n_ranges;
        dst_len = 0;
        if (n_ranges && (!off || !len)) throw RangeArgumentError("invalid argument: ranges without their arrays");
        std::vector<uint64_t> up(n_ranges * 3 + 1);  // off | len | prefix
        uint64_t sum = 0;
        for (size_t k = 0; k < n_ranges; k++) {
            if (off[k] > ix.total || len[k] > ix.total - off[k])
                throw RangeArgumentError("invalid argument: range " + std::to_string(k) + " (offset " + std::to_string(off[k]) + ", length " +
                                         std::to_string(len[k]) + ") does not lie in the " + std::to_string(ix.total) + " decoded bytes");
            if (sum + len[k] < sum) throw RangeArgumentError("invalid argument: the ranges' lengths overflow 64 bits");
            up[k] = off[k];
            up[n_ranges + k] = len[k];
            up[2 * n_ranges + k] = sum;
            sum += len[k];
        }
        up[3 * n_ranges] = sum;
        dst_len = sum;
        st.out_bytes = sum;
        if (d_cap && !d_dst) throw RangeArgumentError("invalid argument: a capacity without a buffer");
        if (!owned_src && n && d_cap && (const uint8_t*)d_dst < d_src + n && d_src < (const uint8_t*)d_dst + d_cap)
            throw RangeArgumentError("invalid argument: the container and the output buffer overlap");
        if (d_cap < sum)
            throw DecodeCapacityError("output buffer of " + std::to_string(d_cap) + " bytes is too small for " + std::to_string(sum));
        if (sum == 0) {
            st.total_s = be.now() - t0;
            return;
        }
        const uint64_t M = ix.members;  // (sum > 0: the container has members)
        grow(d_ranges, ranges_cap, up.size(), false);
        be.h2d(d_ranges, up.data(), up.size() * 8);
        st.host_waits++;
        const uint64_t *d_off = d_ranges, *d_len = d_ranges + n_ranges, *d_prefix = d_ranges + 2 * n_ranges;
        be.memset(plan, 0, (size_t)M * 12);  // stop, status (kDecOk = 0), produced
        be.launch(n_ranges, RangePlan{d_off, d_len, n_ranges, ix.out_off, ix.out_len, M, stop()});
        be.launch_waves(1, RangeCompact{stop(), M, list(), arena_off(), rec}, RangeCompact::lds_bytes());
        RangeRecord r;
        be.d2h(&r, rec, sizeof r);
        st.host_waits++;
        if (r.needed == 0 || r.needed > M || r.scratch_bytes < 16 * r.needed)
            throw std::runtime_error("range plan: inconsistent record");
        if (slots == 0) slots = 1;
        if (slots > r.needed) slots = (uint32_t)r.needed;
        grow(arena, arena_cap, (size_t)r.scratch_bytes, false);
        bool fresh = state_slots < slots;
        if (fresh) {
            size_t cap = (size_t)state_slots * DecodeLayout::kBytes;
            grow(state, cap, (size_t)slots * DecodeLayout::kBytes, true);
            state_slots = slots;
        }
        st.members_decoded = r.needed;
        be.set_timing(true);
        uint64_t nl = 0, nby[4];
        double msby[4];
        be.collect_timed(&nl);
        for (uint64_t first = 0; first < r.needed; first += slots) {
            const uint32_t count = r.needed - first < slots ? (uint32_t)(r.needed - first) : slots;
            if (!fresh) be.memset(state, 0, (size_t)count * DecodeLayout::kBytes);  // (alloc zeroed a new one)
            fresh = false;
            be.timed_begin(2);
            DecodeArgs a{d_src, ix.begin, ix.end, arena_off(), ix.out_len, arena, state, status(), (uint32_t)first, count};
            a.list = list();
            a.stop = stop();
            a.produced = produced();
            be.launch_waves(count, DecodeMember{a}, DecodeMember::lds_bytes());
            be.timed_end(2);
            st.launches++;
        }
        const uint32_t head = (uint32_t)((uintptr_t)d_dst & 15);
        be.timed_begin(1);
        be.launch((size_t)RangeGather::units(sum, head),
                  RangeGather{d_off, d_prefix, n_ranges, ix.out_off, arena_off(), ix.out_len, status(), M, arena, d_dst, sum, head});
        be.timed_end(1);
        std::vector<uint32_t> back((size_t)M * 3);
        be.d2h(back.data(), plan, (size_t)M * 12);
        st.host_waits++;
        be.collect_timed(&nl, msby, nby);  // (the stream has drained: no further wait)
        be.set_timing(false);
        st.kernel_ms = msby[2];
        st.gather_ms = msby[1];
        const uint32_t *h_stop = back.data(), *h_status = h_stop + M, *h_produced = h_status + M;
        for (uint64_t m = 0; m < M; m++) {
            if (!h_stop[m]) continue;
            if (h_status[m] != kDecOk) {
                st.total_s = be.now() - t0;
                throw std::runtime_error(h_status[m] == kDecDeepTable ? "member with a 16-bit Huffman table: use the host decoder"
                                                                      : "invalid orz data (member " + std::to_string(m) + ", status " + std::to_string(h_status[m]) + ")");
            }
            st.decoded_bytes += h_produced[m];
        }
        st.total_s = be.now() - t0;
    }
};

}  // namespace orz
