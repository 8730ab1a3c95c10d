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
//
// CURSORS (opt-in: set_cache).  Every read above starts every member it touches at byte 0, so walking through a member window by
// window is quadratic.  The decoder is causal and its whole state is explicit (the blob, the LDS, a handful of registers:
// DecodeResume), so a reader may keep, under a byte budget, a member's decoded prefix together with the decoder state at its
// end, and a later read costs the bytes not yet decoded.  With the cache on a read is planned on the HOST from the member offsets
// the reader has: upload (ranges and the per-member plan in one copy) -> clear -> DecodeMember launches over the members that
// fall short -> RangeGather -> [host reads statuses and what was produced]: two host waits.  With the cache off a read is what it
// was, launch for launch.
//
// ELEMENT RANGES of plane-encoded tensors (orz_read_elements.h) are this read with another last launch: RangeReader::run is the
// part of a read from the upload to the verdicts, and takes the gather that ends it.
#pragma once
#include <algorithm>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "orz_decode_index.h"
#include "orz_decode_drive.h"
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
    const uint64_t *out_off, *arena_off;  // (arena_off[m]: where a touched member's bytes lie, relative to `arena`, modulo 2^64: cursors' are buffers of their own)
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

struct RangeCacheStats {
    uint64_t hits = 0, resumed = 0, fresh = 0, uncached = 0, evicted = 0;  // of the last read (all zero while the cache is off)
    uint64_t cursors = 0, bytes = 0, budget = 0;                           // now
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
    // the cursor cache (set_cache): off while budget == 0
    struct Cursor {
        uint32_t m;
        uint8_t* mem;       // the member's bytes (out_len rounded up to 256), then a DecodeCursor
        uint64_t cost;
        uint32_t produced;  // valid bytes at mem
        uint64_t touched;   // the read that touched it last
    };
    std::vector<Cursor> cursors;  // ascending in m
    uint64_t budget = 0, held = 0, reads = 0;
    RangeCacheStats last;
    uint8_t* d_up = nullptr;  // one upload a read: off | len | prefix | place[M] | cursor[M] (u64), stop[M] | list[M] (u32)
    size_t up_cap = 0;

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
        for (void* p : {(void*)owned_src, (void*)plan, (void*)rec, (void*)d_ranges, (void*)arena, (void*)state, (void*)d_up})
            if (p) be.free(p);
        for (Cursor& c : cursors) be.free(c.mem);
        cursors.clear();
        held = 0;
        owned_src = plan = arena = state = d_up = nullptr;
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

    // ---- cursors
    // What a cursor costs beyond its member's bytes: the blob, the copy of the LDS, the record.
    static uint64_t cursor_state_bytes() { return DecodeCursor::kBytes; }
    static uint64_t cursor_cost(uint32_t out_len) { return ((uint64_t)out_len + 255) / 256 * 256 + cursor_state_bytes(); }
    uint32_t member_len(uint64_t m) const { return (uint32_t)((m + 1 < ix.members ? h_off[m + 1] : ix.total) - h_off[m]); }
    Cursor* find_cursor(uint32_t m) {
        auto it = std::lower_bound(cursors.begin(), cursors.end(), m, [](const Cursor& c, uint32_t x) { return c.m < x; });
        return it != cursors.end() && it->m == m ? &*it : nullptr;
    }
    void drop_cursor(uint32_t m) {
        Cursor* c = find_cursor(m);
        if (!c) return;
        be.free(c->mem);
        held -= c->cost;
        cursors.erase(cursors.begin() + (c - cursors.data()));
    }
    // the least recently touched cursor that read `now` does not touch (ties: the lower member), or nullptr
    Cursor* oldest(uint64_t now) {
        Cursor* best = nullptr;
        for (Cursor& c : cursors)
            if (c.touched < now && (!best || c.touched < best->touched)) best = &c;
        return best;
    }
    // The budget for cursors in bytes; 0 = off (the default): every cursor is freed and a read is what it was without the cache.
    // A smaller budget evicts least recently touched cursors until the rest fits.  One host wait the first time (the member
    // offsets), none after.
    void set_cache(uint64_t max_bytes) {
        if (max_bytes) member_offsets();
        budget = max_bytes;
        while (held > budget) drop_cursor(oldest(reads + 1)->m);
        last = RangeCacheStats{};
    }
    RangeCacheStats cache_stats() const {
        RangeCacheStats c = last;
        c.cursors = cursors.size(); c.bytes = held; c.budget = budget;
        return c;
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
        check_destination(d_dst, d_cap, sum);
        if (sum == 0) {
            st.total_s = be.now() - t0;
            return;
        }
        const uint32_t head = (uint32_t)((uintptr_t)d_dst & 15);
        run(up, n_ranges, st, slots, t0, [&](const uint64_t* d_up, const uint64_t* d_place, const uint8_t* base) {
            be.launch((size_t)RangeGather::units(sum, head), RangeGather{d_up, d_up + 2 * n_ranges, n_ranges, ix.out_off, d_place, ix.out_len, status(),
                                                                         ix.members, base, d_dst, sum, head});
        });
    }

    // what every read refuses of its output buffer, `sum` being the bytes the ranges ask for
    void check_destination(const uint8_t* d_dst, size_t d_cap, uint64_t sum) const {
        if (d_cap && !d_dst) throw RangeArgumentError("invalid argument: a capacity without a buffer");
        if (!owned_src && n && d_cap && d_dst < d_src + n && d_src < d_dst + d_cap)
            throw RangeArgumentError("invalid argument: the container and the output buffer overlap");
        if (d_cap < sum)
            throw DecodeCapacityError("output buffer of " + std::to_string(d_cap) + " bytes is too small for " + std::to_string(sum));
    }

    // A read from its one upload to the members' verdicts.  `up` = off | len | prefix of n_ranges valid byte ranges that ask for at
    // least one byte, then whatever else the gather wants uploaded with them.  gather(d_up, d_place, base) queues the launch that
    // ends the read behind the decode launches: d_up = `up` on the device, a touched member m's bytes lie at base + d_place[m]
    // (modulo 2^64) as far as the furthest byte asked of it, and status()[m] tells whether they are good.
    template <class Gather>
    void run(std::vector<uint64_t>& up, size_t n_ranges, RangeReadStats& st, uint32_t slots, double t0, const Gather& gather) {
        const uint64_t M = ix.members;  // (bytes are asked for: the container has members)
        if (budget) return read_cached(up, n_ranges, st, slots, t0, gather);
        grow(d_ranges, ranges_cap, up.size(), false);
        be.h2d(d_ranges, up.data(), up.size() * 8);
        st.host_waits++;
        const uint64_t *d_off = d_ranges, *d_len = d_ranges + n_ranges;
        be.memset(plan, 0, (size_t)M * 12);  // stop, status (kDecOk = 0), produced
        be.launch(n_ranges, RangePlan{d_off, d_len, n_ranges, ix.out_off, ix.out_len, M, stop()});
        be.launch_waves(1, RangeCompact{stop(), M, list(), arena_off(), rec}, RangeCompact::lds_bytes());
        RangeRecord r;
        be.d2h(&r, rec, sizeof r);
        st.host_waits++;
        if (r.needed == 0 || r.needed > M || r.scratch_bytes < 16 * r.needed)
            throw std::runtime_error("range plan: inconsistent record");
        slots = clamp_slots(r.needed, slots);
        grow(arena, arena_cap, (size_t)r.scratch_bytes, false);
        bool fresh = state_slots < slots;
        if (fresh) {
            size_t cap = (size_t)state_slots * DecodeLayout::kBytes;
            grow(state, cap, (size_t)slots * DecodeLayout::kBytes, true);
            state_slots = slots;
        }
        st.members_decoded = r.needed;
        TimedBracket<BE> timed(be);
        decode_rounds(r.needed, slots, [&](uint32_t first, uint32_t count) {
            if (!fresh) be.memset(state, 0, (size_t)count * DecodeLayout::kBytes);  // (alloc zeroed a new one)
            fresh = false;
            DecodeArgs a{d_src, ix.begin, ix.end, arena_off(), ix.out_len, arena, state, status(), first, count};
            a.list = list();
            a.stop = stop();
            a.produced = produced();
            launch_decode<DecodeMember>(be, a, st.launches);
        });
        be.timed_begin(1);
        gather(d_ranges, arena_off(), arena);
        be.timed_end(1);
        std::vector<uint32_t> back((size_t)M * 3);
        be.d2h(back.data(), plan, (size_t)M * 12);
        st.host_waits++;
        const std::array<double, 4> ms = timed.finish();  // (the stream has drained: no further wait)
        st.kernel_ms = ms[2];
        st.gather_ms = ms[1];
        const uint32_t *h_stop = back.data(), *h_status = h_stop + M, *h_produced = h_status + M;
        for (uint64_t m = 0; m < M; m++) {
            if (!h_stop[m]) continue;
            if (h_status[m] != kDecOk) {
                st.total_s = be.now() - t0;
                throw decode_status_error(m, h_status[m]);
            }
            st.decoded_bytes += h_produced[m];
        }
        st.total_s = be.now() - t0;
    }

    // A read with the cache on (the ranges are valid, sum > 0).  The policy, in ascending member order over the members the call
    // touches: a cursor whose valid bytes cover the member's stop is a HIT (no decode); one that falls short is RESUMED; a member
    // without a cursor gets a FRESH one if its cost fits the budget, after evicting least recently touched cursors that this call
    // does not touch (ties: the lower member; nothing is evicted when even all of them would not make room); otherwise, or when
    // the allocation fails, it is decoded into the transient arena and nothing is kept (UNCACHED).  A member whose decode fails
    // loses its cursor.
    template <class Gather>
    void read_cached(std::vector<uint64_t>& up, size_t n_ranges, RangeReadStats& st, uint32_t slots, double t0, const Gather& gather) {
        const uint64_t M = ix.members, now = ++reads;
        last = RangeCacheStats{};
        // the plan: RangePlan on the host
        std::vector<uint32_t> h_stop(M, 0), todo, tmembers;
        for (size_t k = 0; k < n_ranges; k++) {
            const uint64_t from = up[k], to = from + up[n_ranges + k];
            if (to == from) continue;
            for (uint64_t m = last_at_or_below(h_off.data(), M, from); m < M && h_off[m] < to; m++) {
                const uint32_t ml = member_len(m);
                if (!ml) continue;
                const uint32_t s = (uint32_t)(std::min(to, h_off[m] + ml) - h_off[m]);
                if (!h_stop[m]) tmembers.push_back((uint32_t)m);
                h_stop[m] = std::max(h_stop[m], s);
            }
        }
        std::sort(tmembers.begin(), tmembers.end());
        for (uint32_t m : tmembers)
            if (Cursor* c = find_cursor(m)) c->touched = now;
        // addr | cursor | stop | list behind the ranges
        const size_t r8 = up.size();
        up.resize(r8 + 2 * M + M);  // (stop and list: M u32 each = M u64 together)
        uint64_t* h_addr = up.data() + r8;
        uint64_t* h_cur = h_addr + M;  // indexed as the list is
        uint32_t* u_stop = (uint32_t*)(h_cur + M);
        uint32_t* u_list = u_stop + M;
        std::fill(h_addr, h_addr + 3 * M, 0);
        std::vector<uint32_t> was(M, 0);      // valid bytes before this read, of a member that is decoded into a cursor
        std::vector<uint8_t> kind(M, 0);      // 1 = decoded into a cursor, 2 = decoded into the arena
        // a member's bytes lie in its cursor or in the arena: h_addr[m] is their address minus the container's, modulo 2^64, so that
        // decoder and gather find them as `base + offset[m]` like every other caller's
        const uint64_t base = (uint64_t)(uintptr_t)d_src;
        uint64_t arena_bytes = 0;
        for (uint32_t m : tmembers) {
            Cursor* c = find_cursor(m);
            if (c && c->produced >= h_stop[m]) {
                last.hits++;
                h_addr[m] = (uint64_t)(uintptr_t)c->mem - base;
                continue;
            }
            if (c) last.resumed++;
            else {
                const uint64_t cost = cursor_cost(member_len(m));
                uint64_t spare = 0;
                for (const Cursor& o : cursors)
                    if (o.touched < now) spare += o.cost;
                if (cost <= budget && held - spare + cost <= budget) {
                    while (held + cost > budget) {
                        drop_cursor(oldest(now)->m);
                        last.evicted++;
                    }
                    uint8_t* mem = nullptr;
                    const size_t data = (size_t)(cost - cursor_state_bytes());
                    try { mem = be.template alloc<uint8_t>((size_t)cost, false); } catch (const std::bad_alloc&) {} catch (const std::runtime_error&) {}
                    if (mem) {
                        be.memset(mem + data, 0, (size_t)cursor_state_bytes());  // a zeroed blob, as a transient slot's; a record that is not live
                        auto at = std::lower_bound(cursors.begin(), cursors.end(), m, [](const Cursor& x, uint32_t y) { return x.m < y; });
                        c = &*cursors.insert(at, Cursor{m, mem, cost, 0, now});
                        held += cost;
                        last.fresh++;
                    }
                }
            }
            if (c) {
                kind[m] = 1;
                was[m] = c->produced;
                h_addr[m] = (uint64_t)(uintptr_t)c->mem - base;
                h_cur[todo.size()] = (uint64_t)(uintptr_t)(c->mem + (c->cost - cursor_state_bytes()));
            } else {
                kind[m] = 2;
                last.uncached++;
                h_addr[m] = arena_bytes;  // (the arena may still move: its address is added below)
                arena_bytes += ((uint64_t)h_stop[m] + 15) & ~(uint64_t)15;
            }
            u_list[todo.size()] = m;
            todo.push_back(m);
        }
        std::copy(h_stop.begin(), h_stop.end(), u_stop);
        const uint64_t need = todo.size();
        slots = clamp_slots(need, slots);
        bool fresh = false;
        if (last.uncached) {
            grow(arena, arena_cap, (size_t)arena_bytes, false);
            for (uint32_t m : todo)
                if (kind[m] == 2) h_addr[m] += (uint64_t)(uintptr_t)arena - base;
            fresh = state_slots < slots;
            if (fresh) {
                size_t cap = (size_t)state_slots * DecodeLayout::kBytes;
                grow(state, cap, (size_t)slots * DecodeLayout::kBytes, true);
                state_slots = slots;
            }
        }
        grow(d_up, up_cap, up.size() * 8, false);
        be.h2d(d_up, up.data(), up.size() * 8);
        st.host_waits++;
        const uint64_t *d_off = (const uint64_t*)d_up, *d_addr = d_off + r8, *d_cur = d_addr + M;
        const uint32_t *d_stop = (const uint32_t*)(d_cur + M), *d_list = d_stop + M;
        be.memset(status(), 0, (size_t)M * 8);  // status (kDecOk = 0), produced
        st.members_decoded = need;
        TimedBracket<BE> timed(be);
        decode_rounds(need, slots, [&](uint32_t first, uint32_t count) {
            bool transient = false;
            for (uint32_t k = 0; k < count; k++) transient |= kind[todo[first + k]] == 2;
            if (transient && !fresh) be.memset(state, 0, (size_t)count * DecodeLayout::kBytes);  // (alloc zeroed a new one)
            if (transient) fresh = false;
            DecodeArgs a{d_src, ix.begin, ix.end, d_addr, ix.out_len, const_cast<uint8_t*>(d_src), state, status(), first, count};
            a.list = d_list;
            a.stop = d_stop;
            a.produced = produced();
            a.cursor = d_cur;
            launch_decode<DecodeMemberCursor>(be, a, st.launches);
        });
        be.timed_begin(1);
        gather(d_off, d_addr, d_src);
        be.timed_end(1);
        std::vector<uint32_t> back((size_t)M * 2);
        be.d2h(back.data(), status(), (size_t)M * 8);
        st.host_waits++;
        const std::array<double, 4> ms = timed.finish();  // (the stream has drained: no further wait)
        st.kernel_ms = ms[2];
        st.gather_ms = ms[1];
        const uint32_t *h_status = back.data(), *h_produced = h_status + M;
        int64_t failed = -1;
        for (uint32_t m : todo) {
            if (h_status[m] != kDecOk) {
                if (failed < 0) failed = m;
                if (kind[m] == 1) drop_cursor(m);
                continue;
            }
            st.decoded_bytes += h_produced[m] - was[m];
            if (kind[m] == 1) find_cursor(m)->produced = h_produced[m];
        }
        st.total_s = be.now() - t0;
        if (failed >= 0) throw decode_status_error((uint64_t)failed, h_status[failed]);
    }
};

}  // namespace orz
