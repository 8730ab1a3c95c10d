// orz_fast_step.h -- FOR TESTS: the step machinery of the fast parse's round loop (orz_fast.h) run ONCE on host arrays, without
// a stream object and without an encode: the path stage (decisions, exit maps, entries, marks), the counts / prefixes / ordinals
// built from a path, and the ring horizons.  Every launch is the product's own (the path stage through fast_path_stage, the
// function the round loop calls); the backend is a template parameter, so the host emulation (tests/emu/emu_fast_step.cpp) runs
// the same lines as the library (orz_capi.hip).  Arrays the kernels write are handed in pre-filled by the caller and handed
// back whole: what a kernel leaves alone comes back as it went in.
#pragma once
#include <stdexcept>
#include <vector>

#include "orz_fast.h"

namespace orz {

struct FastStepInvalid : std::invalid_argument {
    using std::invalid_argument::invalid_argument;
};

// device buffers of one call, freed on every path out
template <class BE>
struct StepBufs {
    BE& be;
    std::vector<void*> all;
    explicit StepBufs(BE& b) : be(b) {}
    ~StepBufs() { for (void* p : all) be.free(p); }
    template <class T> T* zeroed(size_t n) { T* p = be.template alloc<T>(n); all.push_back(p); return p; }
    template <class T> T* from(const T* src, size_t n) {  // a copy of the caller's array
        T* p = be.template alloc<T>(n, false);
        all.push_back(p);
        be.h2d(p, src, n * sizeof(T));
        return p;
    }
};
// The kernels index by window offset: a buffer that stands for the offsets from `first` on is handed to them as a pointer
// `first` elements in front of it (never dereferenced below `first`).
template <class T> T* biased(T* p, size_t first) { return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) - first * sizeof(T)); }

// sizes of the arrays of a call, in entries (the stream's own buffers are sized by the same rules for a full block)
struct FastStepSizes {
    size_t nsub, ntile, pos, x1, x2, centry, tentry, sbits, cm, win, ev;
    FastStepSizes(uint32_t n, uint32_t tile) {
        nsub = ((size_t)n + kSub - 1) / kSub;
        ntile = tile ? ((size_t)n + tile - 1) / tile : 0;
        pos = (size_t)n + kSub + 512;      // ty, nl, x0, pt (a chunk more than the block: a store past a short last chunk stays inside, and shows)
        x1 = (nsub + 2) * kEntries;
        x2 = (ntile + 2) * kEntries;
        centry = nsub + 2;
        tentry = ntile + 2;
        sbits = (size_t)n / 64 + 16;
        cm = (nsub + 2) * 256;             // cm, cp
        win = 2 + (nsub + 1) * kSub + 16;  // window bytes from kPre - 2 on (the kernels read whole chunks and a word more)
        ev = (size_t)n + 8 + 512;
    }
};

// The window the kernels see: the caller's n + 2 bytes (offsets kPre - 2 .. len), zeros behind them.
template <class BE>
const uint8_t* step_window(StepBufs<BE>& b, const uint8_t* wbytes, uint32_t n, const FastStepSizes& z) {
    uint8_t* w = b.template zeroed<uint8_t>(z.win);
    b.be.h2d(w, wbytes, (size_t)n + 2);
    return biased(w, kPre - 2);
}

// the refusals of (a): thrown before anything reaches the device
inline void fast_step_path_check(uint32_t form, uint32_t n, uint32_t tile, uint32_t t_lo, uint32_t t_hi, uint32_t entry, const uint8_t* wbytes,
                                 const uint32_t* ev, const uint8_t* ty, const uint8_t* nl, const uint8_t* x0, const uint8_t* x1, const uint8_t* x2,
                                 const uint32_t* centry, const uint32_t* tentry, const uint64_t* sbits, const uint8_t* pt, const uint32_t* cm) {
    if (!wbytes || !ev || !ty || !nl || !x0 || !x1 || !x2 || !centry || !tentry || !sbits || !pt || !cm) throw FastStepInvalid("null array");
    if (form > kPathPlain) throw FastStepInvalid("no such form");
    if (!n || n > kNewMax) throw FastStepInvalid("n outside 1 .. 2^24");
    if (!tile || tile % kSub || tile > kNewMax) throw FastStepInvalid("the tile is not a multiple of 4096");
    if (t_lo > t_hi || (uint64_t)t_hi * tile >= n) throw FastStepInvalid("tiles outside the block");
    const uint32_t lo = kPre + t_lo * tile;
    if (entry < lo || entry >= lo + kEntries) throw FastStepInvalid("the entry lies outside the first 240 positions of the range");
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t sh = 0; sh < 24; sh += 8) {
            const uint32_t l = (ev[i] >> sh) & 0xff;
            if (l && (l < kMinLen || l > kMaxLen)) throw FastStepInvalid("a length in ev that is neither 0 nor 4 .. 240");
        }
}
// (a) the path stage of one step over the tiles t_lo .. t_hi of `tile` positions, the path entering at window offset `entry`.
// form: PathForm.  lds_used receives PathTileDown::lds_bytes() of the range (0 = its walk ran on global memory).
template <class BE>
void fast_step_path(BE& be, uint32_t form, uint32_t n, uint32_t tile, uint32_t t_lo, uint32_t t_hi, uint32_t entry, const uint8_t* wbytes,
                    const uint32_t* ev, uint8_t* ty, uint8_t* nl, uint8_t* x0, uint8_t* x1, uint8_t* x2, uint32_t* centry, uint32_t* tentry,
                    uint64_t* sbits, uint8_t* pt, uint32_t* cm, uint64_t* lds_used) {
    fast_step_path_check(form, n, tile, t_lo, t_hi, entry, wbytes, ev, ty, nl, x0, x1, x2, centry, tentry, sbits, pt, cm);
    const FastStepSizes z(n, tile);
    StepBufs<BE> b(be);
    FastArgs a{};
    a.win = step_window(b, wbytes, n, z);
    a.n = n; a.len = kPre + n; a.tile = tile;
    a.ev = b.from(ev, z.ev);
    a.ty = b.from(ty, z.pos); a.nl = b.from(nl, z.pos); a.x0 = b.from(x0, z.pos); a.pt = b.from(pt, z.pos);
    a.x1 = b.from(x1, z.x1); a.x2 = b.from(x2, z.x2);
    a.centry = b.from(centry, z.centry); a.tentry = b.from(tentry, z.tentry);
    a.sbits = b.from(sbits, z.sbits); a.cm = b.from(cm, z.cm);
    be.h2d(a.tentry + t_lo, &entry, 4);
    const PathTileDown td{a, t_lo, t_hi - t_lo + 1};
    if (lds_used) *lds_used = td.lds_bytes();
    fast_path_stage(be, a, t_lo, t_hi, (PathForm)form, FastRetireDone{a, kPre, kPre, nullptr});
    be.d2h(ty, a.ty, z.pos); be.d2h(nl, a.nl, z.pos); be.d2h(x0, a.x0, z.pos); be.d2h(pt, a.pt, z.pos);
    be.d2h(x1, a.x1, z.x1); be.d2h(x2, a.x2, z.x2);
    be.d2h(centry, a.centry, z.centry * 4); be.d2h(tentry, a.tentry, z.tentry * 4);
    be.d2h(sbits, a.sbits, z.sbits * 8); be.d2h(cm, a.cm, z.cm * 4);
}

inline void fast_step_counts_check(uint32_t n, const uint8_t* wbytes, const uint64_t* sbits, uint32_t s0, uint32_t s1, uint32_t ext, uint32_t cpt,
                                   uint32_t live_end, uint32_t rows, const uint32_t* cm, const uint32_t* cp, const uint32_t* cp2, const uint32_t* ord,
                                   const uint32_t* ord2, const uint32_t* acc2) {
    if (!wbytes || !sbits || !cm || !cp || !cp2 || !ord || !ord2 || !acc2) throw FastStepInvalid("null array");
    if (!n || n > kNewMax) throw FastStepInvalid("n outside 1 .. 2^24");
    const FastStepSizes z(n, 0);
    // rows: subtile rows of cm (and of cp, which has one more): every subtile the launches touch
    if (!cpt || s0 > s1 || (uint64_t)s1 + ext > rows || rows < z.nsub || rows > kNSub + 2 || live_end < s0 || live_end > s1)
        throw FastStepInvalid("subtile range");
}
// (b) counts, prefixes, ordinals.  count != 0: CountWave over every subtile first (cm from sbits); else cm as given.  Then
// FastPrefix{s0, s1, ext, cpt, live_end} alone -> cp, and as the prefix half of FlipPrefixWave with a flip part of zero
// positions -> cp2 (both start from the caller's cp / cp2); FastItemTotal over cp -> acc2[0] = acc, acc2[1] = hotacc; OrdWave
// with cp -> ord, OrdWave2 -> ord2 (n entries each, entry i = the ordinal of window offset kPre + i).
template <class BE>
void fast_step_counts(BE& be, uint32_t n, const uint8_t* wbytes, const uint64_t* sbits, int count, uint32_t s0, uint32_t s1, uint32_t ext,
                      uint32_t cpt, uint32_t live_end, uint32_t rows, uint32_t* cm, uint32_t* cp, uint32_t* cp2, uint32_t* ord, uint32_t* ord2,
                      uint32_t* acc2) {
    fast_step_counts_check(n, wbytes, sbits, s0, s1, ext, cpt, live_end, rows, cm, cp, cp2, ord, ord2, acc2);
    const FastStepSizes z(n, 0);
    StepBufs<BE> b(be);
    FastArgs a{};
    a.win = step_window(b, wbytes, n, z);
    a.n = n; a.len = kPre + n;
    a.sbits = b.from(const_cast<uint64_t*>(sbits), z.sbits);
    const size_t ncm = (size_t)rows * 256, ncp = ((size_t)rows + 1) * 256;
    a.cm = b.from(cm, ncm);
    uint32_t* d_cp = b.from(cp, ncp);
    uint32_t* d_cp2 = b.from(cp2, ncp);
    uint32_t* d_ord = b.from(ord, n);
    uint32_t* d_ord2 = b.from(ord2, n);
    FastCtl* ctl = b.template zeroed<FastCtl>(1);
    if (count) be.launch_waves(z.nsub, CountWave{a, 0}, CountWave::lds_bytes());
    a.cp = d_cp;
    be.launch_waves(256, FastPrefix{a, s0, s1, ext, cpt, live_end}, FastPrefix::lds_bytes());
    a.cp = d_cp2;
    be.launch_waves(flip_blocks(0) + 256, FlipPrefixWave{FastFlip{}, FastPrefix{a, s0, s1, ext, cpt, live_end}, 0}, FlipPrefixWave::lds_bytes());
    be.launch(256, FastItemTotal{d_cp, (uint32_t)z.nsub, ctl});
    be.launch_waves(z.nsub, OrdWave{a.win, a.sbits, d_cp, n, biased(d_ord, kPre), ctl}, OrdWave::lds_bytes());
    be.launch_waves(z.nsub, OrdWave2{a.win, a.sbits, d_cp, n, biased(d_ord2, kPre), ctl}, OrdWave2::lds_bytes());
    FastCtl h{};
    be.d2h(&h, ctl, sizeof h);
    acc2[0] = h.acc; acc2[1] = h.hotacc;
    be.d2h(cm, a.cm, ncm * 4); be.d2h(cp, d_cp, ncp * 4); be.d2h(cp2, d_cp2, ncp * 4);
    be.d2h(ord, d_ord, (size_t)n * 4); be.d2h(ord2, d_ord2, (size_t)n * 4);
}

inline void fast_step_horizon_check(const uint32_t* cp, uint32_t rows, const uint32_t* hpre, uint32_t s0, uint32_t s1, const uint32_t* hz, const uint32_t* hz2) {
    if (!cp || !hpre || !hz || !hz2) throw FastStepInvalid("null array");
    if (s0 > s1 || s1 + 2 > rows || rows > kNSub + 2) throw FastStepInvalid("subtile range");
}
// (c) ring horizons of the subtiles s0 .. s1 from cp ([rows][256], rows >= s1 + 2) and hpre ([kHistSub + 1][256]): FastHorizon
// alone -> hz, and as the horizon half of RetireHorizonWave with no retiring positions -> hz2 ([s1 + 1][256][4] each).
template <class BE>
void fast_step_horizon(BE& be, const uint32_t* cp, uint32_t rows, const uint32_t* hpre, uint32_t s0, uint32_t s1, uint32_t* hz, uint32_t* hz2) {
    fast_step_horizon_check(cp, rows, hpre, s0, s1, hz, hz2);
    StepBufs<BE> b(be);
    FastArgs a{};
    a.cp = b.from(const_cast<uint32_t*>(cp), (size_t)rows * 256);
    a.hpre = b.from(const_cast<uint32_t*>(hpre), (size_t)(kHistSub + 1) * 256);
    const size_t nhz = ((size_t)s1 + 1) * 256 * 4;
    uint32_t* d_hz = b.from(hz, nhz);
    uint32_t* d_hz2 = b.from(hz2, nhz);
    a.hz = d_hz;
    { const FastHorizon fh{a, s0, s1}; be.launch(fh.threads(), fh); }
    a.hz = d_hz2;
    { const FastHorizon fh{a, s0, s1}; be.launch_waves((fh.threads() + 63) / 64, RetireHorizonWave{FastRetire{}, fh, 0}, 0); }
    be.d2h(hz, d_hz, nhz * 4); be.d2h(hz2, d_hz2, nhz * 4);
}

}  // namespace orz
