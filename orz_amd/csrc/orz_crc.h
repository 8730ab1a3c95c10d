// orz_crc.h -- CRC-32 digests of device buffers, computed where the buffers lie, and the check of decoded tensors against them.
//
// The digest is zlib's: reflected polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF, crc32("") == 0.  A register
// value is a polynomial over GF(2) modulo P with bit 31 the coefficient of x^0, so a step "one zero bit further" is a shift right
// (crc_times_x) and everything below is linear: the raw residue of a message (no initial value, no final xor) is
//     raw(A || B) = raw(A) x^(8 |B|) + raw(B),        crc(M) = raw(M) + 0xFFFFFFFF x^(8 |M|) + 0xFFFFFFFF.
//
// J buffers, given as a table on the device (a column per field: first tile, address, length), cost THREE launches whatever J is:
//
// CrcTiles, one wavefront per tile (launch_waves).  A buffer's first (-address) mod 16 bytes are its head; what follows, the
// body, starts at a multiple of 16 and is cut into tiles of kCrcTileBytes; a buffer with bytes has at least one tile, and its first
// tile takes the head.  A wavefront finds its buffer with last_at_or_below over the first-tile column.  Lane L takes the 16-byte
// words L, L + 64, ... of the tile's full rows of 1,024 bytes -- every load of the wavefront is one coalesced kilobyte, a
// global_load_dwordx4 in the global address space -- and steps  s = xor_i T[i][byte i of (word ^ s in its first four bytes)]
// over 16 tables of 256 words in LDS: T[i][b] is the residue of byte b followed by 15 - i + 1,008 zero bytes, so a step carries
// the state a whole row further.  After R rows the lane holds the residue of its words as if each stood at the START of its row
// and the block ended behind the last row: 16 L bytes too far from the end.  x is invertible modulo P (P has a constant term), so
// the lane multiplies by x^(-128 L), a constant from a 64-entry table.  What does not fill a row goes beside that: the up to 63
// full words behind the last row one to a lane, bit by bit; the head and the up to 15 bytes behind the last full word byte by
// byte on lane 63; each is multiplied by x^(8 x the bytes of the tile behind it) (crc_shift: square-and-multiply over a table of
// x^(2^k)).  No lane loads a byte outside [address, address + length): a word that straddles an edge is never loaded.  The 64
// values are xor-reduced with shuffles, and lane 0 writes the tile's raw residue to residue[tile].
// LDS: 16 KiB a wavefront (the tables, copied from one device-resident image of kCrcImageWords words the host computes once per
// device: crc_image); the reduction needs none.  No scratch, no atomics; a wavefront writes its own tile's word only.
//
// CrcFold, one lane per tile, a launch of its own because it reads what CrcTiles wrote: residue[tile] *= x^(8 x the
// bytes of the buffer behind the tile), in place.  The byte count has 64 bits -- a destination of pieces may exceed 4 GiB -- so the
// table of powers has 67 entries.
// CrcSum, one wavefront per buffer, again a launch of its own: the xor over the buffer's tiles, plus the initial value carried
// over the whole length, plus the final xor, into crcs[buffer].
//
// crc32_host restates the digest for host-resident buffers (slicing by 8); crc32_combine is zlib's crc32_combine on crc_shift,
// the function CrcFold uses.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "orz_decode_index.h"  // (IndexScan::shfl64; DeviceBuffers through orz_decode_device.h)
#include "orz_decode_range.h"  // (last_at_or_below)

namespace orz {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcOne = 0x80000000u;        // the polynomial 1
constexpr uint32_t kCrcRowBytes = 1024;          // what the 64 lanes load at once
constexpr uint32_t kCrcTileBytes = 64 * 1024;    // a multiple of kCrcRowBytes
constexpr uint32_t kCrcPowers = 67;              // x^(2^k), k < 67: 8 x a 64-bit byte count
// the device-resident image, in words: the 16 tables | x^(-128 L) for the 64 lanes | x^(2^k)
constexpr size_t kCrcImgLane = 16 * 256, kCrcImgPow = kCrcImgLane + 64, kCrcImageWords = kCrcImgPow + kCrcPowers + 1;
static_assert(kCrcTileBytes % kCrcRowBytes == 0 && kCrcImageWords % 4 == 0, "tiles are whole rows; the image is copied 16 bytes at a time");

ORZ_HD uint32_t crc_times_x(uint32_t s) { return (s >> 1) ^ (kCrcPoly & (0u - (s & 1))); }
// a b mod P
ORZ_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        p ^= b & (0u - ((a >> i) & 1));
        b = crc_times_x(b);
    }
    return p;
}
// s x^(8 bytes) mod P: the register `bytes` zero bytes further (x2k[k] = x^(2^k) mod P, kCrcPowers entries)
ORZ_HD uint32_t crc_shift(const uint32_t* x2k, uint32_t s, uint64_t bytes) {
    for (uint32_t k = 3; bytes; k++, bytes >>= 1)
        if (bytes & 1) s = crc_mul(s, x2k[k]);
    return s;
}
ORZ_HD uint32_t crc_xpow_bytes(const uint32_t* x2k, uint64_t bytes) { return crc_shift(x2k, kCrcOne, bytes); }

// the raw residue of one byte behind state s, and of a 32-bit little-endian word
ORZ_HD uint32_t crc_byte(uint32_t s, uint32_t b) {
    s ^= b;
    for (int i = 0; i < 8; i++) s = crc_times_x(s);
    return s;
}
ORZ_HD uint32_t crc_word(uint32_t s, uint32_t v) {
    s ^= v;
    for (int i = 0; i < 32; i++) s = crc_times_x(s);
    return s;
}

// What the host computes once per device: kCrcImageWords words at `img`.
inline void crc_image(uint32_t* img) {
    uint32_t t0[256], z[256];
    for (uint32_t b = 0; b < 256; b++) t0[b] = z[b] = crc_byte(0, b);
    for (uint32_t k = 1; k <= 1023; k++) {  // z = the byte followed by k zero bytes
        for (uint32_t b = 0; b < 256; b++) z[b] = (z[b] >> 8) ^ t0[z[b] & 255];
        if (k >= 1008) std::memcpy(img + (size_t)(1023 - k) * 256, z, sizeof z);
    }
    uint32_t inv = kCrcOne;  // x^-128: 128 steps against crc_times_x
    for (int i = 0; i < 128; i++) inv = inv & 0x80000000u ? ((inv ^ kCrcPoly) << 1) | 1u : inv << 1;
    img[kCrcImgLane] = kCrcOne;
    for (uint32_t L = 1; L < 64; L++) img[kCrcImgLane + L] = crc_mul(img[kCrcImgLane + L - 1], inv);
    img[kCrcImgPow] = kCrcOne >> 1;  // x
    for (uint32_t k = 1; k < kCrcPowers; k++) img[kCrcImgPow + k] = crc_mul(img[kCrcImgPow + k - 1], img[kCrcImgPow + k - 1]);
    for (size_t k = kCrcImgPow + kCrcPowers; k < kCrcImageWords; k++) img[k] = 0;
}
inline const uint32_t* crc_host_image() {
    static const std::vector<uint32_t> img = [] {
        std::vector<uint32_t> v(kCrcImageWords);
        crc_image(v.data());
        return v;
    }();
    return img.data();
}

// zlib's crc32 of n host bytes, slicing by 8
inline uint32_t crc32_host(const uint8_t* p, size_t n) {
    struct Tables {
        uint32_t t[8][256];
        Tables() {
            for (uint32_t b = 0; b < 256; b++) t[0][b] = crc_byte(0, b);
            for (int k = 1; k < 8; k++)
                for (uint32_t b = 0; b < 256; b++) t[k][b] = (t[k - 1][b] >> 8) ^ t[0][t[k - 1][b] & 255];
        }
    };
    static const Tables tb;
    uint32_t c = 0xFFFFFFFFu;
    for (; n >= 8; n -= 8, p += 8) {
        uint32_t a, b;
        std::memcpy(&a, p, 4);
        std::memcpy(&b, p + 4, 4);
        a ^= c;
        c = tb.t[7][a & 255] ^ tb.t[6][(a >> 8) & 255] ^ tb.t[5][(a >> 16) & 255] ^ tb.t[4][a >> 24] ^ tb.t[3][b & 255] ^ tb.t[2][(b >> 8) & 255] ^
            tb.t[1][(b >> 16) & 255] ^ tb.t[0][b >> 24];
    }
    for (; n; n--, p++) c = (c >> 8) ^ tb.t[0][(c ^ *p) & 255];
    return ~c;
}
// crc32(A || B) from crc32(A), crc32(B) and |B|
inline uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc_shift(crc_host_image() + kCrcImgPow, crc_a, len_b) ^ crc_b; }

// ------------------------------------------------------------------------------------------------ tiles
ORZ_HD uint64_t crc_head(uint64_t addr, uint64_t len) {
    const uint64_t h = (0 - addr) & 15;
    return h < len ? h : len;
}
ORZ_HD uint64_t crc_tiles(uint64_t addr, uint64_t len) {
    if (!len) return 0;
    const uint64_t body = len - crc_head(addr, len);
    return body ? (body + (kCrcTileBytes - 1)) / kCrcTileBytes : 1;
}

// The buffers of one launch, a column per field (device memory).  first[] ascends from 0; a buffer of no bytes has no tile and
// repeats its successor's first tile, so the search never lands on it.
struct CrcTable {
    const uint64_t* first;  // [n] the buffer's first tile
    const uint64_t* addr;   // [n]
    const uint64_t* len;    // [n] bytes
    uint64_t n;
};

#if defined(__HIP_DEVICE_COMPILE__)
typedef uint32_t CrcQuad __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const CrcQuad* CrcQuadCPtr;
typedef __attribute__((address_space(1))) const uint8_t* CrcByteCPtr;
#endif
// sixteen bytes at a multiple of 16 / one byte, in the GLOBAL address space (the table holds addresses as integers)
ORZ_HD void crc_load16(uint32_t* r, const uint8_t* s) {
#if defined(__HIP_DEVICE_COMPILE__)
    const CrcQuad v = *(CrcQuadCPtr)s;
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
#else
    __builtin_memcpy(r, s, 16);
#endif
}
ORZ_HD uint32_t crc_load8(const uint8_t* s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(CrcByteCPtr)s;
#else
    return *s;
#endif
}
// the raw residue of k bytes, one after the other
ORZ_HD uint32_t crc_bytes(const uint8_t* p, uint32_t k) {
    uint32_t s = 0;
    for (uint32_t i = 0; i < k; i++) s = crc_byte(s, crc_load8(p + i));
    return s;
}
// one step of a lane: the word behind state s, and 1,008 zero bytes (T: the 16 tables)
ORZ_HD uint32_t crc_step(const uint32_t* T, const uint32_t* q, uint32_t s) {
    uint32_t o = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const uint32_t v = d ? q[d] : q[0] ^ s;
#pragma unroll
        for (int b = 0; b < 4; b++) o ^= T[(4 * d + b) * 256 + ((v >> (8 * b)) & 255)];
    }
    return o;
}

struct CrcTiles {
    CrcTable t;
    uint64_t tiles;
    const uint32_t* image;  // crc_image, device-resident
    uint32_t* residue;      // [tiles] out
    static size_t lds_bytes() { return kCrcImgLane * 4; }
    template <class W>
    ORZ_D void operator()(W& w) const {
        const uint32_t lane = w.lane();
        const uint64_t tile = w.block();
        if (tile >= tiles || !t.n) return;  // (wave-uniform)
        uint32_t* const T = (uint32_t*)w.lds();
        for (uint32_t i = lane; i < kCrcImgLane / 4; i += 64) {
            uint32_t q[4];
            crc_load16(q, (const uint8_t*)(image + 4 * i));
            T[4 * i] = q[0]; T[4 * i + 1] = q[1]; T[4 * i + 2] = q[2]; T[4 * i + 3] = q[3];
        }
        w.sync();
        const uint32_t* const x2k = image + kCrcImgPow;
        const uint64_t j = last_at_or_below(t.first, t.n, tile);
        const uint64_t a = t.addr[j], len = t.len[j], k = tile - t.first[j];
        const uint64_t head = crc_head(a, len), body = len - head, lo = k * kCrcTileBytes;
        const uint32_t nb = body - lo < kCrcTileBytes ? (uint32_t)(body - lo) : kCrcTileBytes;  // the tile's bytes of the body
        const uint8_t* const p = (const uint8_t*)(uintptr_t)(a + head + lo);                      // (a multiple of 16)
        const uint32_t W16 = nb / 16, R = W16 / 64, Wr = W16 % 64, r = nb % 16;
        uint32_t s = 0;
#pragma unroll 4
        for (uint32_t row = 0; row < R; row++) {
            uint32_t q[4];
            crc_load16(q, p + (size_t)row * kCrcRowBytes + 16 * lane);
            s = crc_step(T, q, s);
        }
        const uint32_t loose = 16 * Wr + r;  // bytes behind the rows
        uint32_t v = 0;
        if (R) {
            v = crc_mul(s, image[kCrcImgLane + lane]);
            if (loose) v = crc_shift(x2k, v, loose);
        }
        if (lane < Wr) {
            uint32_t q[4];
            crc_load16(q, p + (size_t)R * kCrcRowBytes + 16 * lane);
            const uint32_t c = crc_word(crc_word(crc_word(crc_word(0, q[0]), q[1]), q[2]), q[3]);
            v ^= crc_shift(x2k, c, 16 * (Wr - 1 - lane) + r);
        }
        if (lane == 63) {
            if (k == 0 && head) v ^= crc_shift(x2k, crc_bytes((const uint8_t*)(uintptr_t)a, (uint32_t)head), nb);
            if (r) v ^= crc_bytes(p + 16 * (size_t)W16, r);
        }
        for (uint32_t d = 32; d; d >>= 1) v ^= w.shfl(v, lane ^ d);
        if (lane == 0) residue[tile] = v;
    }
};

// One lane per tile: the tile's residue carried over the bytes of its buffer behind it.
struct CrcFold {
    CrcTable t;
    uint64_t tiles;
    const uint32_t* image;
    uint32_t* residue;  // [tiles] in place
    ORZ_HD void operator()(size_t u) const {
        const uint64_t tile = u;
        if (tile >= tiles || !t.n) return;
        const uint64_t j = last_at_or_below(t.first, t.n, tile);
        const uint64_t len = t.len[j], body = len - crc_head(t.addr[j], len), end = (tile - t.first[j] + 1) * kCrcTileBytes;
        if (end < body) residue[tile] = crc_shift(image + kCrcImgPow, residue[tile], body - end);
    }
};

// One wavefront per buffer: the xor over its tiles, the initial value over its length, the final xor.
struct CrcSum {
    CrcTable t;
    const uint32_t* image;
    const uint32_t* residue;
    uint32_t* crcs;  // [n] out
    static size_t lds_bytes() { return 0; }
    template <class W>
    ORZ_D void operator()(W& w) const {
        const uint32_t lane = w.lane();
        const uint64_t j = w.block();
        if (j >= t.n) return;
        const uint64_t len = t.len[j], first = t.first[j], cnt = crc_tiles(t.addr[j], len);
        uint32_t v = 0;
        for (uint64_t i = lane; i < cnt; i += 64) v ^= residue[first + i];
        for (uint32_t d = 32; d; d >>= 1) v ^= w.shfl(v, lane ^ d);
        if (lane == 0) crcs[j] = v ^ crc_shift(image + kCrcImgPow, 0xFFFFFFFFu, len) ^ 0xFFFFFFFFu;
    }
};

// the three launches over a table on the device; residue: `tiles` words, crcs: t.n words
template <class BE>
void crc_launches(BE& be, const CrcTable& t, uint64_t tiles, const uint32_t* d_image, uint32_t* d_residue, uint32_t* d_crcs) {
    be.launch_waves((size_t)tiles, CrcTiles{t, tiles, d_image, d_residue}, CrcTiles::lds_bytes());
    be.launch((size_t)tiles, CrcFold{t, tiles, d_image, d_residue});
    be.launch_waves((size_t)t.n, CrcSum{t, d_image, d_residue, d_crcs}, CrcSum::lds_bytes());
}
constexpr uint64_t kCrcLaunches = 3;

// The digests of n buffers in device memory (host arrays of addresses and lengths): ONE upload of the table, the three launches,
// ONE read of the digests -- 2 host waits for any n > 0.  d_image: crc_image on the device.
template <class BE>
void crc32_device_buffers(BE& be, const uint32_t* d_image, const uint64_t* addrs, const uint64_t* lens, size_t n, uint32_t* crcs,
                          uint64_t& host_waits) {
    if (!n) return;
    std::vector<uint64_t> up(3 * n);
    uint64_t tiles = 0;
    for (size_t j = 0; j < n; j++) {
        up[j] = tiles;
        up[n + j] = addrs[j];
        up[2 * n + j] = lens[j];
        tiles += crc_tiles(addrs[j], lens[j]);
    }
    DeviceBuffers<BE> own(be);
    uint64_t* d_table = own.template alloc<uint64_t>(3 * n, false);
    uint32_t* d_residue = own.template alloc<uint32_t>((size_t)tiles, false);
    uint32_t* d_crcs = own.template alloc<uint32_t>(n, false);
    be.h2d(d_table, up.data(), up.size() * 8);
    host_waits++;
    crc_launches(be, CrcTable{d_table, d_table + n, d_table + 2 * n, n}, tiles, d_image, d_residue, d_crcs);
    be.d2h(crcs, d_crcs, n * 4);
    host_waits++;
}

// ------------------------------------------------------------------------------------------------ the verified decode
// What decode_members_planes (orz_planes.h) takes to check its destinations: null for every caller that does not verify.
struct CrcCheck {
    const uint32_t* d_image;  // crc_image on the device
    const uint32_t* expect;   // [n_dsts] (host) the digests the destinations must have
    uint32_t* computed;       // [n_dsts] (host) out, optional: filled whenever the digest launches ran
};
// the first destination whose digest differs
struct DecodeDigestError : std::runtime_error {
    uint64_t dst;
    uint32_t expected, computed;
    static std::string hex(uint32_t v) {
        char b[16];
        std::snprintf(b, sizeof b, "0x%08x", (unsigned)v);
        return b;
    }
    DecodeDigestError(uint64_t j, uint32_t want, uint32_t got)
        : std::runtime_error("digest mismatch: destination " + std::to_string(j) + " should have CRC-32 " + hex(want) + ", its decoded bytes have " + hex(got)),
          dst(j), expected(want), computed(got) {}
};

// One wavefront: the digest table of the destinations of a planes plan, made on the device from what the plan's upload and the
// index hold (no further upload): destination j's address, its size -- elems[j] x ((Q - 1) S + the last piece), as PlanePlan has it
// -- and the exclusive prefix sum of the tiles (PlaneScan's scan).
struct CrcPlan {
    const uint64_t* dsts;     // [n_dsts]
    const uint64_t* first_m;  // [n_dsts]
    const uint32_t* elems;    // [n_dsts]
    const uint32_t* pieces;   // [n_dsts] or nullptr: one
    uint64_t n_dsts;
    const uint32_t* out_len;  // [members]
    uint64_t *c_first, *c_addr, *c_len;  // [n_dsts] out
    static size_t lds_bytes() { return 0; }
    template <class W>
    ORZ_D void operator()(W& w) const {
        const uint32_t lane = w.lane();
        uint64_t carry = 0;
        for (uint64_t at = 0; at < n_dsts; at += 64) {
            const uint64_t j = at + lane;
            uint64_t v = 0;
            if (j < n_dsts) {
                const uint64_t f = first_m[j], Q = pieces ? pieces[j] : 1;
                const uint64_t len = ((Q - 1) * out_len[f] + out_len[f + Q - 1]) * elems[j];
                c_addr[j] = dsts[j];
                c_len[j] = len;
                v = crc_tiles(dsts[j], len);
            }
            uint64_t x = v;
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint64_t y = IndexScan::shfl64(w, x, lane >= d ? lane - d : lane);
                if (lane >= d) x += y;
            }
            if (j < n_dsts) c_first[j] = carry + x - v;
            carry += IndexScan::shfl64(w, x, 63);
        }
    }
};

}  // namespace orz
