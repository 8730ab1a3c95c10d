/*
 * orz_hip.h -- C ABI of the MI355X-native orz encoder (liborz_hip.so).
 *
 * This is the drop-in boundary of the repo: plain C, pointers and sizes only.  The reference
 * (richox/orz v1.6.1, Rust) exports no C symbols (its `// pub mod ffi;` at src/lib.rs:10 is dead),
 * so each entry point below replaces the Rust call surface that `orz::encode` / `orz::decode`
 * use; the file:line of the interface it stands in for is cited per function.  INTEGRATION.md
 * shows the Rust `extern "C"` binding a maintainer would add.
 *
 * Error convention: 0 = ok, negative = failure (ORZ_E*); nothing throws across the boundary.
 * orz_last_error() returns a thread-local description of the last failure.
 */
#ifndef ORZ_HIP_H
#define ORZ_HIP_H

#include <stddef.h>
#include <stdint.h>
#include <sys/types.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORZ_OK 0
#define ORZ_EINVAL (-22)  /* bad argument / InvalidData (io::ErrorKind::InvalidData, src/lz.rs:413-415) */
#define ORZ_ENOMEM (-12)  /* output buffer too small / allocation failure */
#define ORZ_EIO (-5)      /* read/write callback failed (io::Error from Read/Write, src/lib.rs:58-63) */
#define ORZ_ENODEV (-19)  /* no usable HIP device, or a HIP runtime error */
#define ORZ_EBADMSG (-74) /* decoded bytes whose CRC-32 digest differs from the one given (orz_decode_tensors_verified) */

/* src/lib.rs:31-34,54-55 -- window geometry the object-level API inherits */
#define ORZ_LZ_BLOCK_SIZE ((1u << 25) - 1)
#define ORZ_SBVEC_SENTINEL_LEN 480u
#define ORZ_SBVEC_PREMATCH_LEN (ORZ_LZ_BLOCK_SIZE / 2)

/* mirrors #[repr(C)] LZCfg, src/lz.rs:32-37 (three usize) */
typedef struct {
    size_t match_depth, lazy_match_depth1, lazy_match_depth2;
} orz_lzcfg;

/* level -> LZCfg, src/main.rs:97-102.  Returns ORZ_EINVAL for levels other than 0,1,2. */
int orz_lzcfg_from_level(int level, orz_lzcfg* out);

/* ---- object level: LZEncoder (src/lz.rs:69-346) --------------------------------------------- */
typedef struct orz_lz_encoder orz_lz_encoder;

/* LZEncoder::new, src/lz.rs:75-80.  `device` = HIP device ordinal.  NULL on failure. */
orz_lz_encoder* orz_lz_encoder_new(int device);
void orz_lz_encoder_free(orz_lz_encoder*);

/* LZEncoder::encode(&mut self, &LZCfg, sbuf, tbuf, spos) -> (spos, tpos), src/lz.rs:89-95,346.
 * Preconditions inherited from src/lib.rs:67-69: sbuf points ORZ_SBVEC_SENTINEL_LEN bytes inside
 * an allocation and sbuf[-480 .. sbuf_len+480) is readable (bytes past sbuf_len influence tail
 * decisions exactly as in the reference); spos >= ORZ_SBVEC_PREMATCH_LEN on the first call of a
 * block.  Produces ONE chunk (at most 2^20 items) per call like the reference.  The device parses
 * the whole block on the first call of a block and hands the remaining chunks out on the following
 * calls, which must continue at the returned *spos_out with the same sbuf contents. */
int orz_lz_encoder_encode(orz_lz_encoder*, const orz_lzcfg*, const uint8_t* sbuf, size_t sbuf_len, uint8_t* tbuf,
                          size_t tbuf_cap, size_t spos, size_t* spos_out, size_t* tlen_out);
/* LZEncoder::forward, src/lz.rs:82-87 (forward_len must be 2^24 = LZ_BLOCK_SIZE - PREMATCH, the
 * only value the reference ever passes, src/lib.rs:84). */
int orz_lz_encoder_forward(orz_lz_encoder*, size_t forward_len);

/* ---- stream level: orz::encode (src/lib.rs:58-92) ------------------------------------------- */
typedef ssize_t (*orz_read_fn)(void* ctx, uint8_t* buf, size_t cap); /* 0 = EOF, <0 = error */
typedef int (*orz_write_fn)(void* ctx, const uint8_t* buf, size_t len);
/* ProgressLogger, src/progress.rs:9-13 */
typedef void (*orz_progress_fn)(void* ctx, int is_finish, size_t in_bytes, size_t out_bytes);

int orz_encode(orz_read_fn, void* rctx, orz_write_fn, void* wctx, const orz_lzcfg*, orz_progress_fn, void* pctx,
               int device);

/* ---- decode side (host code: a stream decodes as one serial chain) ------------- */
typedef struct orz_lz_decoder orz_lz_decoder;
/* LZDecoder::new / decode / forward, src/lz.rs:352-478.  decode() writes the chunk's bytes at
 * sbuf[spos..] (sbuf laid out like the encoder's window, 480-byte pads, >= 2*LZ_BLOCK_SIZE long as in
 * src/lib.rs:102) and returns the new spos in *spos_end_out; ORZ_EINVAL = InvalidData. */
orz_lz_decoder* orz_lz_decoder_new(void);
void orz_lz_decoder_free(orz_lz_decoder*);
int orz_lz_decoder_decode(orz_lz_decoder*, const uint8_t* tbuf, size_t tlen, uint8_t* sbuf, size_t spos,
                          size_t* spos_end_out);
int orz_lz_decoder_forward(orz_lz_decoder*, size_t forward_len);
/* orz::decode, src/lib.rs:94-129 */
int orz_decode(orz_read_fn, void* rctx, orz_write_fn, void* wctx, orz_progress_fn, void* pctx);
/* whole-buffer convenience: decodes the first stream found at src; *consumed = bytes of src it used */
int orz_decode_mem(const uint8_t* src, size_t n, uint8_t** dst, size_t* dst_len, size_t* consumed);

/* ---- reusable stream encoder on caller memory (what bench.py and the Python mirror drive) ---- */
typedef struct {
    uint64_t blocks, sweeps, seg_evals, items, chunks, in_bytes, out_bytes;
    double t_prep_s, t_parse_s, t_post_s; /* host clock around device syncs */
    double parse_kernel_ms;               /* HIP-event time of the parse kernel launches (sum) */
    uint64_t parse_launches;
    double total_ms;                      /* HIP-event time of the whole encode on the stream */
    uint64_t host_syncs;                  /* times the host waited for a stream during the call (every hipStreamSynchronize of the
                                             encoder: reads of counts and sizes, copies of finished output, the closing wait) */
} orz_encode_stats;

typedef struct orz_stream orz_stream;
orz_stream* orz_stream_new(int device, const orz_lzcfg* cfg);
void orz_stream_free(orz_stream*);
/* Parse mode.  ORZ_MODE_EXACT reproduces the reference encoder's parse (src/lz.rs:131-235) item for item, so
 * the stream is byte-identical to `orz encode`; ORZ_MODE_FAST is the GPU-native parse (orz_amd/csrc/orz_fast.h):
 * same bitstream format, decodes bit-exactly with the reference decoder, size within +-0.5 % of the
 * reference's at the same level (BASELINE.json north_star), an order of magnitude faster.  New encoders start
 * in fast mode unless the environment says ORZ_MODE=exact.  tile_bytes (multiple of 4096) / rounds: 0 = keep. */
#define ORZ_MODE_EXACT 0
#define ORZ_MODE_FAST 1
int orz_stream_set_mode(orz_stream*, int mode, unsigned tile_bytes, unsigned rounds);
typedef struct {
    int mode;
    unsigned segment_bytes, window_segments;               /* exact mode: speculative segment / sweep window */
    unsigned fast_tile_bytes, fast_rounds, fast_row_entries; /* fast mode: Gauss-Seidel tile, rounds, candidates tabulated per position */
    unsigned unit_bytes;  /* bytes of a 16 MiB block encoded per pipeline unit (the whole block unless ORZ_FAST_UNIT says otherwise; a unit closes its last chunk) */
} orz_stream_config;
/* what the encoder actually runs with (bench.py reports these instead of literals) */
int orz_stream_get_config(orz_stream*, orz_stream_config* out);
/* HIP-event time and launch count of four kernels over the last orz_stream_encode call made with stats != NULL:
 * [0] the parse's per-position kernel (exact: ParseWave, fast: FastEval), [1] symbol ranking, [2] candidate table
 * build (fast mode), [3] path maps (fast mode).  What bench.py's roofline leg is computed from. */
int orz_stream_get_kernel_times(orz_stream*, double* ms4, uint64_t* launches4);
/* Profile mode: also bracket the kernels inside the fast parse's round loop ([0] and [3] above).  That loop normally
 * runs as one hipGraph replay per block (its launch sequence is the same for every full block); brackets need
 * individual launches, so a profiled encode is slower than a normal one -- use it for the roofline leg only. */
int orz_stream_set_profile(orz_stream*, int on);
/* Profile mode, all of it: EVERY kernel (and library call: sorts, scans, fills) of the last profiled orz_stream_encode made with
 * stats != NULL, by name, HIP-event time summed over its launches, largest first.  Returns the number of rows the encode
 * produced (copy at most `cap` of them into `rows`; rows == NULL just counts).  bench.py's per-kernel table and DESIGN.md 6
 * are generated from this (tools/kernel_table.py). */
typedef struct {
    char name[64];
    double ms;
    uint64_t launches;
} orz_kernel_row;
long orz_stream_get_kernel_table(orz_stream*, orz_kernel_row* rows, size_t cap);
/* tuning: bytes per speculative segment and segments per sweep window (0 = keep) */
int orz_stream_set_tuning(orz_stream*, unsigned seg_bytes, unsigned window_segs);
/* Encode `n` bytes at `src` (host memory, or device memory when src_on_device != 0) into a
 * library-owned orz stream (*dst, release with orz_free and nothing else: results of 1 MiB or more are page-locked buffers of
 * a small pool that orz_free hands back to it).  Same bytes as `orz encode` would write. */
int orz_stream_encode(orz_stream*, const void* src, size_t n, int src_on_device, uint8_t** dst, size_t* dst_len,
                      orz_encode_stats* stats);
void orz_free(void* p);
/* The same, with the finished stream left in DEVICE memory the caller owns (round 6): `d_dst` = `d_cap` bytes on the stream's
 * device; *dst_len bytes are written -- { LEB128(t) chunk[t] }* and the EOF byte, framed on the device (src/lib.rs:79-80,89).
 * The analogue of the reference handing LZEncoder::encode a caller-owned `tbuf` (src/lz.rs:89-95), for a whole stream: what the
 * multi-GPU gather sends from where it lies.  d_cap >= orz_stream_bound(n) always suffices; a buffer that turns out too small
 * fails the encode (ORZ_ENOMEM) without a byte of the overflowing block written.  One host wait per 16 MiB block and one per stream. */
size_t orz_stream_bound(size_t n);
int orz_stream_encode_to_device(orz_stream*, const void* src, size_t n, int src_on_device, uint8_t* d_dst, size_t d_cap,
                                size_t* dst_len, orz_encode_stats* stats);

/* Per-item trace of the last orz_stream_encode call (diagnostics / stage-level parity tests):
 * what the parse decided for each item, in stream order.  Mirrors the reference's MatchItem
 * (src/lz.rs:100-116) after the symrank pass. */
typedef struct {
    uint32_t block;         /* 0-based block index */
    uint32_t pos;           /* window offset of the item start (spos) */
    uint16_t symbol;        /* raw symbol: literal, 256 + roid*6 + lenid, or 388 (WORD) */
    uint16_t rank;          /* symbol after symrank */
    uint16_t ctx;           /* symrank_context (9 bit) */
    uint16_t robits;        /* robits | robitlen << 12 */
    uint8_t unlikely;       /* symrank_unlikely */
    uint8_t enc_len;        /* encoded_match_len */
    uint8_t after_literal;  /* bit 0: after_literal, bit 1: item is a match */
    uint8_t match_len;      /* match length (0 for literal / WORD) */
    uint32_t src;           /* window offset of the match source (0 for literal / WORD) */
} orz_item;
int orz_stream_set_item_trace(orz_stream*, int on);
/* copies up to cap items to out, returns the total number traced (or a negative error) */
long orz_stream_get_item_trace(orz_stream*, orz_item* out, size_t cap);

/* FOR TESTS of the validity gate: overwrite named fields of named items of the NEXT encode on this stream, after the parse and
 * before the items are coded -- the way a defect of the parse or of the item stage would appear, or (SRC) another legal parse.
 * `block` is the counter orz_item.block reports, `pos` the window offset of an item start of that block.  TYPE (low two bits of
 * the item type: 0 WORD, 1 literal), LEN (match length) and SRC (window offset of the match source) go into the parse's
 * per-position arrays before the len_min bookkeeping; LMV (the len_min a match is coded against) behind that bookkeeping; SYM,
 * CTX, AL (bit 0 of after_literal), ENC, ROB (robits | robitlen << 12), UNL into the item arrays before they are ranked, ORD into
 * the parse's ring ordinal at pos.  The list holds for one encode, whether it succeeds or not; n == 0 clears it.  A non-empty
 * list is announced on stderr like the environment's fault-injection hooks.  A patch that finds no item start at (block, pos)
 * is not applied and the encode fails for that reason: "item patches: ... were not applied".  ORZ_EINVAL, before anything
 * reaches the device, for every value a later kernel would index with out of range: an unknown field, pos outside the block's
 * new bytes, TYPE > 1 (no patch makes a match of an item without a source), LEN > 240, SRC outside [1, pos), SYM >= 389,
 * CTX >= 512, AL > 1, ENC >= 240, UNL > 255, LMV > 127, ROB with more than 12 extra bits or bits above their count; more than
 * 65536 patches.  Set the list after any call that reconfigures the stream (orz_stream_set_mode, orz_stream_set_tuning). */
enum { ORZ_PATCH_TYPE = 0, ORZ_PATCH_LEN, ORZ_PATCH_SRC, ORZ_PATCH_SYM, ORZ_PATCH_CTX, ORZ_PATCH_AL, ORZ_PATCH_ENC, ORZ_PATCH_ROB,
       ORZ_PATCH_UNL, ORZ_PATCH_ORD, ORZ_PATCH_LMV };
typedef struct {
    uint32_t block, pos, field, value;
} orz_item_patch;
int orz_stream_set_item_patches(orz_stream*, const orz_item_patch* patches, size_t n);

/* FOR TESTS: the static tables of one block of the fast parse (orz_fast.h, FastArgs), read between the block's prep kernels and
 * its first round.  name == NULL arms the capture for the `arm_block`-th encode_block call (0 = the first; a block encoded in
 * units makes one call per unit) of the NEXT encode on this stream, arm_block < 0 disarms; returns 0.  An armed encode waits
 * for the prep kernels of that block and copies its tables to host memory; its stream is the one an unarmed encode writes, and
 * an unarmed encode does nothing for this.  With a name: the size in bytes of that table of the captured block, of which up to
 * `cap` bytes are copied to dst.  Names: "scalars" (eight u64: n, nhist, nent, nk, K, stream offset of the block's first new
 * byte, block number, window offset of that byte), "hpos", "wsnap", "epos", "keys", "idx" (of the n new positions), "runstart",
 * "rlen", "vbits", "stext", "cl", "ccnt", "rows" (n x K), "rdist", "kpos", "kkeys", "krun", "kw", "wmask", "kmeta", "hcm",
 * "hpre".  ORZ_EINVAL, before anything reaches the device: an exact-mode stream, a block number above 65535, a name that no
 * table has, no captured block. */
long orz_stream_fast_tables(orz_stream*, int arm_block, const char* name, void* dst, size_t cap);

/* FOR TESTS: the repair stage of one block of the fast parse (orz_fast.h: RepairListWave, FastSource, FastRecut, FastWordCheckL,
 * FastWordApplyL, ...), pass by pass.  orz_stream_arm_repair_probe arms it for the `block`-th encode_block call of the NEXT encode
 * on this stream (block < 0 disarms).  The armed block runs its rounds and repair passes outside the captured graph -- the same
 * launches in the same order -- and waits before every FastPassEnd to copy the state to host memory; the stream is the one an
 * unarmed encode writes, and an unarmed encode does nothing for this.  ty / nl (n bytes each, or NULL / NULL / 0): a decision
 * field for every position of the armed block, on and off the path, that replaces the rounds' before the first pass: ty = 0 WORD,
 * 1 literal, 2 match; nl = 0 (undecided: read as a literal), 1 for a literal, 2 for WORD, 4..240 for a match; i + nl[i] <= n.
 * The path (walked from the block's first position) and the previous-item types follow from it; n must be the armed block's size
 * (else that encode returns ORZ_EINVAL when it reaches the block, before the block is parsed).  orz_stream_repair_probe: the size in bytes of a table of the probed block, of which up to `cap` bytes
 * are copied to dst.  Tables: "scalars" (eight u64: n, K, depth, block number, sizeof the control block, 1 in the lists form, 0, 0), "passes" (u32:
 * passes recorded, the last of which repaired nothing), "before.ty|nl|pt" (n + 1 bytes), "before.sbits" (u64 words), per pass k
 * "p<k>.ty|nl|pt|sbits", "p<k>.src" (n u32: window offsets), "p<k>.edge" (n bytes), "p<k>.cok" (512 u32: the per-context counters
 * and flags), "p<k>.ctl" (the control block as the pass left it: u32 chg, done, total, passes, nmem, acc, lt, lastflips, nent,
 * ncut, nfix, nwx, hot, hotacc), lists form: "p<k>.mcnt|wcnt" (entries per subtile) and "p<k>.mlist|wlist" (u16 rows of 1024 / 2048
 * entries, one row more than the block has subtiles; the rows are filled with 0xa5 before the first pass of the armed block), and
 * "final.S|TY|ML|W0" (n bytes), "final.ctl", lists form: "final.items" (u32).  ORZ_EINVAL, before anything reaches the device: an exact-mode stream, a block number above 65535, a field that
 * breaks the contract, a name that no table has, no probed block. */
int orz_stream_arm_repair_probe(orz_stream*, int block, const unsigned char* ty, const unsigned char* nl, size_t n);
long orz_stream_repair_probe(orz_stream*, const char* name, void* dst, size_t cap);

/* ---- many members per GPU (independent chunks, each a complete orz stream) ------------
 * A stream does not shard (its model state is one adaptive chain), so throughput beyond one stream
 * comes from encoding independent members concurrently: `jobs` stream encoders on one device, each fed
 * members of `member_bytes` input bytes by its own host thread.  The output is the members' streams
 * concatenated in input order; every member ends with its own EOF chunk, so the reference decoder reads
 * each piece (orz_decode_members_mem / `orz decode --members` loop over them). */
typedef struct orz_members orz_members;
orz_members* orz_members_new(int device, const orz_lzcfg* cfg, int jobs);
/* the same across several GPUs of the node: `jobs_per_device` stream encoders on each of the listed
 * devices, one host thread each; members go to whichever worker is free, the finished streams are collected in
 * host memory in member order (the only "gather" the job needs: the output lives on the host).  Input must be host
 * memory unless all workers sit on one device. */
orz_members* orz_members_new_multi(const int* devices, int n_devices, const orz_lzcfg* cfg, int jobs_per_device);
void orz_members_free(orz_members*);
int orz_members_encode(orz_members*, const void* src, size_t n, int src_on_device, size_t member_bytes, uint8_t** dst,
                       size_t* dst_len, size_t* n_members_out);
/* The same with the members' streams left in DEVICE memory the caller owns (round 6; all workers on ONE device): they are
 * written into `d_dst` (`d_cap` bytes on that device) in whatever order they finish; member k's stream is the
 * lens[k] bytes at d_dst + offs[k] (`offs`, `lens`: host arrays of at least (n + member_bytes - 1) / member_bytes entries,
 * 1 for n = 0).  d_cap >= orz_stream_bound(member_bytes) * members always suffices; ORZ_ENOMEM when the buffer fills. */
int orz_members_encode_to_device(orz_members*, const void* src, size_t n, int src_on_device, size_t member_bytes, uint8_t* d_dst,
                                 size_t d_cap, size_t* offs, size_t* lens, size_t* n_members_out);
/* ONE MEMBER PER CALLER-GIVEN SEGMENT, in segment order: segment k is the seg_len[k] bytes at seg_src[k] (all host memory, or
 * all on the workers' device when src_on_device != 0), for callers that hold a list of separate allocations of unequal sizes (the
 * tensors of a checkpoint, the pages of a table) and want neither a packing copy nor a member boundary inside a tensor.  Any
 * length: 0 (an empty member, as n == 0 gives above), below a block, several blocks; no alignment is asked of a pointer.  Member
 * k's stream is byte for byte what orz_members_encode writes for that segment alone with member_bytes >= seg_len[k], whichever
 * worker takes it and whatever that worker encoded before.  Workers, arenas and waits are those of the two calls above.
 * orz_members_bound_segments: the sum of orz_stream_bound(seg_len[k]), a d_cap that always suffices.
 * orz_members_encode_segments: the streams concatenated in segment order in host memory (*dst: release with orz_free);
 *   lens (optional, n_segs entries) = each member's stream length.
 * orz_members_encode_segments_to_device: the streams left in d_dst (d_cap bytes on the workers' one device) in whatever order
 *   they finish; member k's stream is the lens[k] bytes at d_dst + offs[k] (host arrays of n_segs entries): the table
 *   orz_decode_members_to_device, orz_decode_members_scatter and orz_reader_open take.
 * n_segs == 0: ORZ_OK, no members, no bytes, nothing launched.  ORZ_EINVAL, before anything reaches the device: NULL arrays with
 * n_segs > 0, a NULL segment of non-zero length, a device-resident segment that overlaps [d_dst, d_dst + d_cap), device-resident
 * segments with workers on several devices.  ORZ_ENOMEM when d_dst fills up. */
size_t orz_members_bound_segments(const size_t* seg_len, size_t n_segs);
int orz_members_encode_segments(orz_members*, const void* const* seg_src, const size_t* seg_len, size_t n_segs, int src_on_device,
                                uint8_t** dst, size_t* dst_len, size_t* lens);
int orz_members_encode_segments_to_device(orz_members*, const void* const* seg_src, const size_t* seg_len, size_t n_segs,
                                          int src_on_device, uint8_t* d_dst, size_t d_cap, size_t* offs, size_t* lens);
/* decodes every stream of a concatenation (a plain single stream is the 1-member case) */
int orz_decode_members_mem(const uint8_t* src, size_t n, uint8_t** dst, size_t* dst_len, size_t* n_members_out);

/* ---- members decoded on the device (decoder on GPU, one member per wavefront) --------
 * Replaces orz::decode (/root/reference/src/lib.rs:94-129) + LZDecoder::decode (src/lz.rs:366-478) for a
 * concatenation of members: decoding one stream is a serial chain, so each member is decoded by one lane of
 * its own wavefront and the parallelism is the number of members (up to 2048 in flight).  Members of several
 * blocks decode too (round 4): a member decodes straight into its place in the output, ring nodes hold offsets into
 * the member, and the reference's window slide (src/lib.rs:119-124, src/matcher.rs:82-87) is a counter that retires
 * the nodes that left the window.  Members of 4 GiB or more fail with ORZ_EINVAL and a message naming the host
 * decoder.  Same bytes out as orz_decode_members_mem; ORZ_EINVAL for what the reference reports as InvalidData. */
typedef struct {
    uint64_t members, in_bytes, out_bytes;
    uint64_t launches;     /* kernel launches (members / 2048, rounded up) */
    double kernel_ms;      /* HIP-event time of the decode kernel launches (sum) */
    double total_s;        /* wall time incl. framing scan, uploads and the download of the result */
} orz_decode_stats;
int orz_decode_members_device(int device, const uint8_t* src, size_t n, uint8_t** dst, size_t* dst_len,
                              size_t* n_members_out, orz_decode_stats* stats);
/* Members decoded from and into DEVICE memory.  `src` holds n bytes (device memory of `device` when src_on_device != 0, host
 * memory otherwise).  Layout: offs == NULL -> src is one concatenation of members (what orz_members_encode / orz_stream_encode
 * write); offs != NULL -> member k is the lens[k] bytes at src + offs[k] (host arrays of n_members entries, any order and gaps
 * allowed: what orz_members_encode_to_device reports; offs and lens are both given or both NULL).  Output: the members' bytes
 * concatenated in member order at d_dst (d_cap bytes on `device`); *dst_len = total decoded size, *n_members_out = members,
 * out_offs (optional host array, one entry a member) = where each member's bytes start.  d_dst == NULL with d_cap == 0 only
 * sizes: fills *dst_len / *n_members_out / out_offs and decodes nothing.  ORZ_ENOMEM when d_cap < *dst_len (nothing written to
 * d_dst; *dst_len and *n_members_out are filled); ORZ_EINVAL for malformed data, for a table entry out of range or not ending at
 * its member's EOF byte, and for a device-resident src that overlaps the d_cap bytes at d_dst -- the message names the first bad
 * member.  The framing is indexed ON the device (orz_decode_index.h): no host copy of the container or the output is made.
 * Bytes identical to orz_decode_members_mem; returns after the last byte is written.  Nothing outside
 * [d_dst, d_dst + *dst_len) is written, and the output does not depend on what d_dst held.  ORZ_DECODE_SLOTS = members in
 * flight, as for orz_decode_members_device. */
int orz_decode_members_to_device(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens,
                                 size_t n_members, uint8_t* d_dst, size_t d_cap, size_t* dst_len, size_t* n_members_out,
                                 size_t* out_offs, orz_decode_stats* stats);
/* EACH MEMBER INTO A DESTINATION OF ITS OWN (orz_decode_scatter.h).  src / n / src_on_device / offs / lens / n_members exactly as
 * for orz_decode_members_to_device.  Member k's decoded bytes go to d_dsts[k] (d_caps[k] bytes on `device`; host arrays of n_dsts
 * entries); out_lens (optional, n_dsts entries) = each member's decoded size, filled also when the call fails with ORZ_ENOMEM;
 * *n_members_out = members.  d_dsts == NULL only sizes: the first min(n_dsts, members) entries of out_lens are filled and nothing
 * is decoded.  A member that decodes to 0 bytes may have any pointer and capacity 0.
 *   ORZ_EINVAL, all found before any decode launch: malformed data and table entries as for orz_decode_members_to_device (the
 *     first bad member is named); n_dsts different from the member count; a NULL destination of a member that has bytes; two
 *     destinations of members that have bytes overlap (whole capacities count); a destination overlaps a device-resident src.
 *   ORZ_ENOMEM naming the first member whose destination is smaller than its decoded size: NOTHING has been written to any
 *     destination.
 *   ORZ_EINVAL naming the member, after the launches: payload damage (the content of the destinations is then unspecified).
 * Bytes identical to orz_decode_members_mem's, member by member.  Nothing outside [d_dsts[k], d_dsts[k] + out_lens[k]) is written
 * for any k, and the output does not depend on what the buffers held.  The decode launches are those of
 * orz_decode_members_to_device (ORZ_DECODE_SLOTS members in flight): this removes the copy that splits a concatenation, not
 * decode time.  The host waits a constant number of times whatever the number of members: one read of the index record, one
 * upload of destinations and capacities together, one read of the plan's record with the sizes, one read of the statuses -- 4,
 * and one more each for the upload of a member table and of a host-resident src (6 at most); a sizing call: the index's waits
 * and one read of the sizes.  orz_decode_members_scatter_host_waits: that count for the calling thread's last
 * orz_decode_members_scatter call (orz_decode_stats is laid out as it always was). */
int orz_decode_members_scatter(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens,
                               size_t n_members, uint8_t* const* d_dsts, const size_t* d_caps, size_t n_dsts,
                               size_t* out_lens, size_t* n_members_out, orz_decode_stats* stats);
uint64_t orz_decode_members_scatter_host_waits(void);

/* ---- tensors as byte planes, a member per plane (orz_planes.h) -----------------------------------------
 * For typed data: plane p of a segment of seg_elem-byte elements is byte p of every element (the bytes at offsets p, p + e,
 * p + 2 e, ...).  The predictable bytes of multi-byte elements -- sign and exponent, the high bytes of ids and counts -- then
 * stand next to each other instead of between noise bytes: weights shrink by about a tenth, ids and counts severalfold (DESIGN
 * 9).  The format does not change: every plane is an ordinary member, and a segment contributes seg_elem consecutive members,
 * plane 0 first (an element size of 1: its bytes unchanged as one member; an empty segment: seg_elem empty members).
 * seg_elem[k] is 1, 2, 4 or 8 and divides seg_len[k].  The stream of a plane is byte for byte what
 * orz_members_encode_segments_to_device writes for those plane bytes as a segment of their own.
 * orz_members_bound_planes: the sum of seg_elem[k] * orz_stream_bound(seg_len[k] / seg_elem[k]), a d_cap that always suffices.
 *   A stream's bound is dominated by about 1 MiB a member for small inputs, so callers with many small tensors should size
 *   d_dst themselves instead.
 * orz_members_encode_planes_to_device: offs / lens (host arrays of sum(seg_elem) entries, segment by segment, plane 0 first) say
 *   where each member's stream lies in d_dst.  Workers, arenas and waits are those of orz_members_encode_segments_to_device; it
 *   costs more: ONE device buffer for the call's duration that holds the planes of every segment with seg_elem > 1 (plane
 *   pitches rounded up to 16, each segment's planes at a multiple of 256) and, with src_on_device == 0, a copy of every segment
 *   (host input is uploaded first, every segment of it, and then takes the path of device-resident input); one upload of the
 *   descriptor table and ONE PlaneSplit launch for all segments, waited for once.  Device-resident segments with seg_elem == 1
 *   are encoded where they lie.
 * n_segs == 0: ORZ_OK, nothing launched.  ORZ_EINVAL, before anything reaches the device: what
 * orz_members_encode_segments_to_device refuses, a NULL seg_elem with n_segs > 0, an element size other than 1, 2, 4, 8, a
 * length its element size does not divide.  ORZ_ENOMEM when d_dst fills up or the staging buffer cannot be allocated. */
size_t orz_members_bound_planes(const size_t* seg_len, const uint32_t* seg_elem, size_t n_segs);
int orz_members_encode_planes_to_device(orz_members*, const void* const* seg_src, const size_t* seg_len, const uint32_t* seg_elem,
                                        size_t n_segs, int src_on_device, uint8_t* d_dst, size_t d_cap, size_t* offs, size_t* lens);
/* PLANES MERGED ON DECODE.  src / n / src_on_device / offs / lens / n_members exactly as for orz_decode_members_scatter.
 * Destination j (d_caps[j] bytes at d_dsts[j] on `device`; host arrays of n_dsts entries) takes the next elems[j] members as the
 * byte planes of elements of elems[j] bytes; out_lens (optional, n_dsts entries) = each destination's size in bytes, plane size
 * x elems[j], filled also when the call fails with ORZ_ENOMEM; *n_members_out = members.  d_dsts == NULL only sizes (elems is
 * still needed): nothing is decoded.  A destination of 0 bytes may have any pointer and capacity 0.
 *   ORZ_EINVAL, all found before any decode launch: what orz_decode_members_scatter refuses of a container; the sum of elems
 *     different from the member count ("X planes for Y members"); an element size other than 1, 2, 4, 8; the planes of one
 *     destination not all of the same decoded size (the destination and the first member that differs are named); a NULL
 *     destination that has bytes; two destinations that have bytes overlap (whole capacities count); a destination overlaps a
 *     device-resident src.
 *   ORZ_ENOMEM naming the first destination whose capacity is below its size: NOTHING has been written to any destination.  Also
 *     when the staging buffer cannot be allocated.
 *   ORZ_EINVAL naming the member, after the launches: payload damage (the content of the destinations is then unspecified).
 * Nothing outside [d_dsts[j], d_dsts[j] + out_lens[j]) is written for any j, and the output does not depend on what the buffers
 * held.  Members of destinations with elems == 1 decode straight into them; the others decode into a staging buffer (freed
 * before the call returns: at most the container's decoded size plus 32 bytes a member; none when every elems[j] is 1) and ONE
 * PlaneMerge launch queued behind the decode launches (ORZ_DECODE_SLOTS members in flight) writes their destinations.  Host
 * waits: those of orz_decode_members_scatter for the same container, whatever the number of destinations -- 4, and one more each
 * for a member table and a host-resident src.  orz_decode_members_planes_host_waits: that count for the calling thread's last
 * orz_decode_members_planes call. */
int orz_decode_members_planes(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens,
                              size_t n_members, uint8_t* const* d_dsts, const size_t* d_caps, const uint32_t* elems, size_t n_dsts,
                              size_t* out_lens, size_t* n_members_out, orz_decode_stats* stats);
uint64_t orz_decode_members_planes_host_waits(void);
/* PIECES: planes of large tensors cut into members that decode side by side.  A member decodes on one lane, so the number of
 * members is the decoder's parallelism; with a piece size of P = piece_elems elements (a multiple of 16) plane p of a segment of
 * `count` elements becomes Q = max(1, ceil(count / P)) consecutive members, piece q holding the plane's bytes
 * [q P, min(count, (q + 1) P)).  A segment contributes seg_elem x Q members, PLANE-MAJOR: plane 0's pieces 0 .. Q - 1, then plane
 * 1's.  piece_elems == 0 or >= count: one piece, the layout of orz_members_encode_planes_to_device.  The format does not change:
 * a piece is an ordinary member, byte for byte what orz_members_encode_segments_to_device writes for the piece's bytes as a
 * segment of their own.  The caller keeps elems and pieces as it keeps elems today.
 * orz_members_bound_planes_pieces: a d_cap that always suffices (the sum of the pieces' orz_stream_bound); *n_members_out
 *   (optional) = the members the encode call writes, sum(seg_elem[k] * Q_k).
 * orz_members_encode_planes_pieces_to_device: orz_members_encode_planes_to_device -- the same ONE staging buffer and ONE
 *   PlaneSplit launch -- with one work item per piece.  pieces_out[k] = Q of segment k (n_segs entries); offs / lens have
 *   sum(seg_elem[k] * Q_k) entries in member order.  With piece_elems == 0 every member is byte for byte that call's.
 *   ORZ_EINVAL before anything reaches the device: what that call refuses, a piece_elems that is no multiple of 16, a NULL
 *   pieces_out with n_segs > 0.
 * orz_decode_members_planes_pieces: orz_decode_members_planes with pieces[j] (n_dsts entries, each >= 1), the pieces per plane
 *   of destination j, which takes the next elems[j] x pieces[j] members.  Its contract is that call's word for word -- refusals
 *   before any decode launch, ORZ_ENOMEM naming the first short destination with nothing written, nothing written outside
 *   [d_dsts[j], d_dsts[j] + out_lens[j]), the same host waits whatever the number of destinations and pieces -- with
 *   out_lens[j] = elems[j] x ((Q - 1) S + the last piece's size), S being the decoded size of the destination's first member:
 *   a destination may exceed 4 GiB though every member stays below it.  A plane's pieces decode back to back, straight into a
 *   destination with elems == 1 and into the plane's place in staging otherwise; the ONE PlaneMerge launch is unchanged.
 *   ORZ_EINVAL in addition, each naming the destination and the first member that offends: pieces[j] == 0; sum(elems[j] x
 *   pieces[j]) different from the member count ("X pieces of planes for Y members"); with pieces[j] > 1: S no multiple of 16, a
 *   piece but the last of another size than S, a last piece of 0 or more than S bytes; planes of one destination whose pieces
 *   differ in size.
 * orz_decode_members_planes_pieces_host_waits: the host waits of the calling thread's last such call. */
size_t orz_members_bound_planes_pieces(const size_t* seg_len, const uint32_t* seg_elem, size_t n_segs, size_t piece_elems, size_t* n_members_out);
int orz_members_encode_planes_pieces_to_device(orz_members*, const void* const* seg_src, const size_t* seg_len, const uint32_t* seg_elem,
                                               size_t n_segs, size_t piece_elems, int src_on_device, uint8_t* d_dst, size_t d_cap, size_t* offs,
                                               size_t* lens, size_t* pieces_out);
int orz_decode_members_planes_pieces(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens,
                                     size_t n_members, uint8_t* const* d_dsts, const size_t* d_caps, const uint32_t* elems,
                                     const uint32_t* pieces, size_t n_dsts, size_t* out_lens, size_t* n_members_out, orz_decode_stats* stats);
uint64_t orz_decode_members_planes_pieces_host_waits(void);
/* DIGESTS: an end-to-end check of what a decode wrote (orz_crc.h).  The stream format carries no checksum and the device decoder
 * reports only damage that breaks a stream's structure: a flipped payload bit, a member table whose entries are mixed up or a
 * piece decoded into the wrong place decode without error to the right number of wrong bytes.  The digest is the zlib CRC-32 of
 * the tensor's own bytes (reflected polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF, crc32 of nothing == 0) --
 * zlib.crc32(t.cpu().numpy().tobytes()) -- whether the tensor is stored whole, as planes or as pieces; the caller keeps it beside
 * the container as it keeps elems and pieces.
 * orz_crc32_buffers: crcs[j] = the digest of the lens[j] bytes at bufs[j] (host arrays of n entries).  on_device == 0: the
 *   buffers lie in host memory and are digested on the host; no device is needed.  Otherwise they lie on `device` and are
 *   digested there: ONE upload of the table of addresses and lengths, three launches whatever n is (a wavefront per tile of 64
 *   KiB, a lane per tile, a wavefront per buffer), ONE read of the digests -- 2 host waits for any n.  (The first call of a
 *   process on a device also uploads the kernels' 17 KiB of tables, once.)  Nothing is written to any buffer and no byte outside
 *   [bufs[j], bufs[j] + lens[j]) is read, whatever the address.  n == 0: ORZ_OK.  ORZ_EINVAL before anything reaches the
 *   device: a NULL array with n > 0, a NULL buffer that has bytes.
 * orz_crc32_combine (host only): the digest of A followed by B from crc_a = that of A, crc_b = that of B and len_b = the length
 *   of B, which may exceed 4 GiB.
 * orz_decode_tensors_verified: ONE entry point for the three layouts.  Its contract is orz_decode_members_planes_pieces' word
 *   for word -- the arguments, the refusals before any decode launch with nothing written, ORZ_ENOMEM naming the first short
 *   destination, nothing written outside [d_dsts[j], d_dsts[j] + out_lens[j]) -- with these differences.  pieces == NULL: one
 *   piece each (the layout of orz_decode_members_planes).  elems == NULL: every element size is 1 (the layout of
 *   orz_decode_members_scatter: a member per destination).  crcs (n_dsts entries) = the digests the destinations must have; it
 *   is required: NULL is ORZ_EINVAL ("bad argument") before anything reaches the device, except in a sizing call (d_dsts ==
 *   NULL), which verifies nothing and ignores crcs.  Behind the PlaneMerge launch -- behind the decode launches when nothing is
 *   merged -- four launches whatever n_dsts is digest the destinations' decoded bytes where they lie: one that makes the table of
 *   addresses and sizes on the device from what the call's ONE plan upload already holds, and the three of orz_crc32_buffers.  The
 *   computed digests come back in ONE additional read after the statuses and are compared with crcs on the host: host waits =
 *   those of orz_decode_members_planes_pieces for the same container, plus 1.  Verdicts, in this order: the refusals before any
 *   launch, as there; a member whose decode failed, ORZ_EINVAL naming the member; otherwise the first destination whose digest
 *   differs, ORZ_EBADMSG, orz_last_error() naming the destination, the expected digest and the computed one ("digest mismatch:
 *   destination J should have CRC-32 0x..., its decoded bytes have 0x...").  The destinations keep what was decoded.  out_crcs
 *   (optional, n_dsts entries) = the computed digests, filled whenever the digest launches ran: with ORZ_OK, ORZ_EBADMSG and a
 *   failed member.  ORZ_ENOMEM also when the digests' device memory (4 bytes a destination and a tile) cannot be had, before any
 *   decode launch.
 * orz_decode_tensors_verified_host_waits: the host waits of the calling thread's last such call. */
int orz_crc32_buffers(int device, const void* const* bufs, const size_t* lens, size_t n, int on_device, uint32_t* crcs);
uint32_t orz_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
int orz_decode_tensors_verified(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens,
                                size_t n_members, uint8_t* const* d_dsts, const size_t* d_caps, const uint32_t* elems,
                                const uint32_t* pieces, size_t n_dsts, const uint32_t* crcs, size_t* out_lens, uint32_t* out_crcs,
                                size_t* n_members_out, orz_decode_stats* stats);
uint64_t orz_decode_tensors_verified_host_waits(void);
/* A measuring hook (tools/dev/planes_bench.py), not a data path: `reps` launches of PlaneSplit (merge == 0) or PlaneMerge over ONE
 * tensor of `count` elements of `elem` bytes (2, 4 or 8) -- interleaved at d_inter, planes at d_planes with a pitch of count
 * rounded up to 16, both on `device` and owned by the caller -- between two events after one warming launch; *ms = milliseconds
 * a launch. */
int orz_plane_move_time(int device, void* d_inter, void* d_planes, size_t count, uint32_t elem, int merge, int reps, double* ms);
/* DELTAS: tensors as the planes (and pieces) of tensor XOR base, merged with the base on the device.  For a tensor kept many
 * times with small differences -- step N and step N + 1 of a run, a fine-tune beside its base model -- when the reader already
 * holds the other one: the steps of a bf16 run shrink 2.3 to 6 times against their plain planes, a frozen layer costs almost
 * nothing.  XOR is its own inverse and works byte by byte, so it needs no rule per dtype and commutes with the split
 * into planes and pieces.  The container format does not change: every member is an ordinary orz stream, and WHICH tensors are
 * deltas, and of what, travels beside the container as elems, pieces and the digests do.  The base comes in where every byte
 * is touched once anyway, in the move between interleaved bytes and planes: no temporary of the tensor's size, no pass more.
 * orz_members_encode_deltas_to_device: orz_members_encode_planes_pieces_to_device word for word -- layout, pieces_out, bounds
 *   (orz_members_bound_planes_pieces still suffices), refusals -- with seg_base (n_segs entries): seg_base[k] = seg_len[k] bytes
 *   resident where the sources are (src_on_device governs both), elements of seg_elem[k] bytes, or NULL for no base.  Every
 *   member's stream is byte for byte what that call writes for the bytes src XOR base as a segment of their own; with no base
 *   anywhere the output is that call's byte for byte.  Host bases are uploaded into the call's one staging buffer beside their
 *   segments; still ONE table upload (the bases are a column of it), ONE split launch (PlaneSplitDelta) and one wait before the
 *   workers start.  A segment with seg_elem == 1 that has a base is staged like the others; without one a device-resident one
 *   is encoded where it lies, as there.  Neither the sources nor the bases are written.  ORZ_EINVAL in addition: a NULL
 *   seg_base with n_segs > 0.
 * orz_decode_tensors_delta: the contract of orz_decode_tensors_verified -- elems and pieces optional in the same way -- with
 *   these differences.  crcs may be NULL: nothing is verified, and launches and waits are those of
 *   orz_decode_members_planes_pieces.  With crcs: verification, the order of the verdicts and ORZ_EBADMSG as there; the digests
 *   are of the RESTORED tensors, not of the deltas, so a delta applied to another base than the one it was made of is a digest
 *   mismatch.  d_bases (n_dsts entries; NULL with n_dsts > 0 is ORZ_EINVAL, "bad argument"): d_bases[j] = out_lens[j] bytes on
 *   `device`, the base of destination j, or NULL for none.  A base may be EXACTLY its own destination's address (in place): the
 *   destination holds the base on entry and the tensor on return.  ORZ_EINVAL before any decode launch, with nothing written
 *   anywhere, each naming the destination: a base that wraps the address space, one that overlaps its own destination at any
 *   other address, one that overlaps another destination (whole capacities count).  A base may overlap the container or another
 *   base: all of them are only read.  The bases go up in the plan's ONE upload and ONE PlaneMergeDelta launch stands where
 *   PlaneMerge stood (a destination with elems == 1 that has a base is staged and merged too): host waits are exactly those of
 *   orz_decode_members_planes_pieces for the same container, plus 1 with crcs.  AFTER A FAILURE behind the launches -- payload
 *   damage (ORZ_EINVAL naming the member) or a digest mismatch -- a base given out of place is untouched, and a destination
 *   decoded in place holds NEITHER its base NOR its tensor: keep a copy of a base you cannot make again.
 * orz_decode_tensors_delta_host_waits: the host waits of the calling thread's last such call.
 * orz_plane_delta_move_time: orz_plane_move_time for PlaneSplitDelta / PlaneMergeDelta with the base at d_base (count x elem
 *   bytes on `device`); elem may be 1 too.  A measuring hook (tools/dev/delta_bench.py), not a data path. */
int orz_members_encode_deltas_to_device(orz_members*, const void* const* seg_src, const void* const* seg_base, const size_t* seg_len,
                                        const uint32_t* seg_elem, size_t n_segs, size_t piece_elems, int src_on_device, uint8_t* d_dst,
                                        size_t d_cap, size_t* offs, size_t* lens, size_t* pieces_out);
int orz_decode_tensors_delta(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens,
                             size_t n_members, uint8_t* const* d_dsts, const size_t* d_caps, const void* const* d_bases,
                             const uint32_t* elems, const uint32_t* pieces, size_t n_dsts, const uint32_t* crcs, size_t* out_lens,
                             uint32_t* out_crcs, size_t* n_members_out, orz_decode_stats* stats);
uint64_t orz_decode_tensors_delta_host_waits(void);
int orz_plane_delta_move_time(int device, void* d_inter, const void* d_base, void* d_planes, size_t count, uint32_t elem, int merge,
                              int reps, double* ms);
/* CHAINS: deltas are kept as a chain -- a keyframe every N steps and a delta per step against the step before.  A chain container
 * is `links` LINKS one behind the other, each byte for byte a container orz_members_encode_planes_pieces_to_device or
 * orz_members_encode_deltas_to_device wrote for the same list of tensors: the same element sizes and the same piece_elems, so the
 * same elems, pieces and number of members M1 = sum(elems[j] x pieces[j]).  The container has links x M1 members, link-major,
 * found from the framing or from a member table as in every other call.  Nothing in the format says so: that a container is a
 * chain travels beside it as elems, pieces, bases and digests do.  XOR is associative and commutes with the split into planes
 * and pieces, so
 *     destination j = d_bases[j] XOR (tensor j of link 0) XOR ... XOR (tensor j of link `links` - 1)
 *   is made in the plane domain in ONE merge launch (PlaneMergeChain) behind ONE decode of all links' members, which decode side
 *   by side in the same rounds.  THE ORDER OF THE LINKS DOES NOT MATTER to the result.  Without a base the result is the XOR of
 *   the links: a chain whose link 0 is a plain keyframe restores without bases, and a chain of deltas alone yields the composed
 *   delta, which a caller can encode again to shorten a chain.
 * orz_decode_tensors_chain: the arguments and the contract of orz_decode_tensors_delta, with `links` and these differences.
 *   d_bases may be NULL: no bases at all.  links == 1 IS orz_decode_tensors_delta (without d_bases: orz_decode_tensors_verified,
 *   or orz_decode_members_planes_pieces without crcs) -- the same launches, uploads, host waits and messages.  For any `links`
 *   the host waits are those of orz_decode_members_planes_pieces for the same container -- 4, +1 for a member table, +1 for a
 *   host container, +1 with crcs -- and the launches those of orz_decode_tensors_delta for a container of as many members.  crcs
 *   are the digests of the FINAL tensors: nobody needs the digests of the steps in between, and a destination restored in place
 *   never holds one of them.  out_lens are link 0's sizes.  Every destination is staged, single bytes too: staging memory, freed
 *   before the call returns, is `links` times the tensors' bytes (and 32 bytes a member).
 *   ORZ_EINVAL before any decode launch, with nothing written anywhere, each naming what offends: links == 0 (before anything
 *   reaches a device); links x M1 different from the member count ("K links of M1 members for M members"); per link what
 *   orz_decode_members_planes_pieces refuses of pieces and planes, naming the link and the member; a tensor whose planes in link k
 *   have another size than in link 0, naming k, the destination and both sizes; everything orz_decode_tensors_delta refuses of
 *   destinations and bases.  ORZ_ENOMEM: a short destination, as there; staging memory that cannot be had.
 *   AFTER A FAILURE behind the launches -- payload damage (ORZ_EINVAL naming the member) or a digest mismatch -- a base given out
 *   of place is untouched, and a destination restored in place holds NEITHER its base NOR its tensor.
 *   A reader (orz_reader_*) on a chain container still sees single links: it knows nothing of chains.
 * orz_decode_tensors_chain_host_waits: the host waits of the calling thread's last such call.
 * orz_plane_chain_move_time: orz_plane_delta_move_time for PlaneMergeChain: `links` plane sets, link k's planes
 *   elem x (count rounded up to 16) bytes behind link k - 1's, from d_planes; d_base may be NULL (no base).  A measuring hook
 *   (tools/dev/chain_bench.py), not a data path. */
int orz_decode_tensors_chain(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens,
                             size_t n_members, uint8_t* const* d_dsts, const size_t* d_caps, const void* const* d_bases,
                             const uint32_t* elems, const uint32_t* pieces, size_t n_dsts, const uint32_t* crcs, uint32_t links,
                             size_t* out_lens, uint32_t* out_crcs, size_t* n_members_out, orz_decode_stats* stats);
uint64_t orz_decode_tensors_chain_host_waits(void);
int orz_plane_chain_move_time(int device, void* d_inter, const void* d_base, const void* d_planes, size_t count, uint32_t elem,
                              uint32_t links, int reps, double* ms);

/* ---- byte ranges of a members container (orz_decode_range.h) ------------------------------------------
 * A reader indexes a container ONCE (on the device, as orz_decode_members_to_device does) and then serves reads of byte
 * ranges of its DECODED data.  A read decodes only the members its non-empty ranges touch, each once per call however many
 * ranges touch it, and each only as far as the furthest byte asked of it (decoding is causal: the first k bytes of a member
 * need only the items that start before k), so what a read costs follows the bytes asked for, not the container: a member
 * decodes at one lane's speed, and a range at a member's start costs a fraction of one at its end.  Nothing is kept between
 * reads but the index and buffers, unless the caller gives the reader a budget for cursors (orz_reader_set_cache, below).
 *
 * orz_reader_open: src / n / src_on_device / offs / lens / n_members exactly as for orz_decode_members_to_device.  A host
 * container is uploaded and owned by the reader; a device container is BORROWED: the caller keeps it alive and unchanged until
 * orz_reader_close.  NULL on failure, orz_last_error() as index errors read there (the first bad member is named).
 * orz_reader_info: members, total decoded size and, when member_offs != NULL, the first `cap` members' decoded start offsets.
 * orz_reader_read: n_ranges byte ranges [off[k], off[k] + len[k]) of the decoded data (member order, as
 * orz_decode_members_to_device lays it out), in any order, overlapping, repeated and empty ranges allowed.  Their bytes are
 * written back to back in range order at d_dst (d_cap bytes on the reader's device); *dst_len = the sum of len[].
 *   ORZ_EINVAL, before anything reaches the device: a range with off + len above the total or overflowing 64 bits, NULL
 *     arrays with n_ranges > 0, a device-resident container that overlaps [d_dst, d_dst + d_cap).
 *   ORZ_ENOMEM: d_cap below the sum of the lengths.  Nothing is written; *dst_len is filled.
 *   n_ranges == 0 or all lengths zero: ORZ_OK, *dst_len == 0, nothing is launched.
 *   ORZ_EINVAL naming the member: payload damage BEFORE the furthest byte asked of a member (the content of the output is
 *     then unspecified).  Damage behind that point is not seen and does not fail the read.
 * The bytes equal the same slices of what orz_decode_members_mem returns and do not depend on what d_dst held; nothing outside
 * [d_dst, d_dst + *dst_len) is written in any case.  A reader serves any number of reads and a failed read leaves it usable.
 * Reads on one reader are SERIAL: a reader is not thread-safe (readers of their own are independent).  The host waits three
 * times per read whatever the number of ranges: the upload of the ranges, one read of the plan's record, one read of the
 * members' verdicts.  ORZ_DECODE_SLOTS bounds the members in flight as for orz_decode_members_device: more needed members
 * than slots are several launches. */
typedef struct orz_reader orz_reader;
typedef struct {
    uint64_t ranges;           /* ranges of the call */
    uint64_t members_decoded;  /* distinct members touched by non-empty ranges (with cursors: those a decode ran for) */
    uint64_t decoded_bytes;    /* bytes the decoder produced: per member the furthest byte asked, plus at most one item (with
                                  cursors: the bytes NEWLY produced in this call) */
    uint64_t out_bytes;        /* sum of the lengths */
    uint64_t launches;         /* decode launches */
    uint64_t host_waits;
    double kernel_ms;          /* HIP-event time of the decode launches (sum) */
    double gather_ms;          /* HIP-event time of the copy into d_dst */
    double total_s;            /* wall time of the call */
} orz_read_stats;
orz_reader* orz_reader_open(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens,
                            size_t n_members);
void orz_reader_close(orz_reader*);
int orz_reader_info(orz_reader*, uint64_t* members, uint64_t* total, uint64_t* member_offs, size_t cap);
int orz_reader_read(orz_reader*, const uint64_t* off, const uint64_t* len, size_t n_ranges, uint8_t* d_dst, size_t d_cap,
                    uint64_t* dst_len, orz_read_stats* stats);

/* CURSORS (opt-in).  Without them every read starts every member it touches at byte 0, so walking through a member window by
 * window decodes its beginning again and again.  With a budget a reader keeps cursors: a member's decoded prefix in device
 * memory together with the decoder's state at its end, so a later read costs only the bytes not yet decoded and nothing for
 * bytes that are there (a second read of a range, a seek backwards).
 * orz_reader_set_cache: the budget in bytes of device memory; 0 = off, the default: every cursor is freed and a read is exactly
 *   what it is without this call.  A smaller budget evicts least recently touched cursors until the rest fits.
 * orz_reader_cursor_state_bytes: a cursor of a member that decodes to n bytes costs n rounded up to 256 plus this constant (the
 *   decoder's tables, a copy of its LDS, its registers: about 7.4 MB).  A budget below that of the members read keeps nothing.
 * Policy, over the members a call touches, in ascending member order: a cursor that holds the furthest byte asked of its member is
 * a HIT (no decode); one that falls short is RESUMED; a member without one gets a FRESH cursor if its cost fits the budget after
 * evicting least recently touched cursors that the call does not touch (ties: the lower member; nothing is evicted unless that
 * makes room), and is otherwise decoded as without the cache and nothing is kept (UNCACHED; so is a member whose cursor cannot
 * be allocated: not an error).  A member whose decode fails loses its cursor; the read reports ORZ_EINVAL naming it as above and
 * the reader stays usable.  Damage behind the furthest byte asked is still not seen.
 * With the cache on, orz_read_stats.decoded_bytes counts the bytes the decoder NEWLY produced in the call (0 for hits),
 * members_decoded the members a decode ran for (resumed + fresh + uncached), launches is 0 when every touched member is a hit,
 * and the host waits twice per read, whatever the ranges: the upload of the ranges and of the plan (made on the host from the
 * member offsets), and the read of the members' verdicts. */
typedef struct {
    uint64_t hits, resumed, fresh, uncached, evicted; /* of the last read, in members (all 0 while the cache is off) */
    uint64_t cursors, bytes, budget;                  /* now: cursors held, what they cost, orz_reader_set_cache's value */
} orz_cache_stats;
int orz_reader_set_cache(orz_reader*, uint64_t max_bytes);
uint64_t orz_reader_cursor_state_bytes(void);
int orz_reader_cache_stats(orz_reader*, orz_cache_stats* stats);

/* ELEMENT RANGES of plane-encoded tensors (orz_read_elements.h).  A container that orz_members_encode_planes_to_device wrote
 * holds a tensor of e-byte elements as e members, one per byte plane.  Once the reader knows which members are whose planes it
 * serves ranges of ELEMENTS, merged on the device: a read decodes only the planes its non-empty ranges touch, each once, and each
 * only as far as the furthest element asked of its tensor, and a tensor's planes decode side by side.
 * orz_reader_set_planes: tensor j is the next elems[j] members, plane 0 first; n_tensors == 0 withdraws the declaration.
 *   ORZ_EINVAL, with nothing changed and nothing launched: an element size other than 1, 2, 4 or 8 (the tensor and the size are
 *   named); a sum of elems[] different from the member count ("X planes for Y members"); planes of one tensor that decode to
 *   different sizes (the tensor and the first member that differs are named); elems == NULL with n_tensors > 0.  At most one host
 *   wait: the member offsets, if the reader has not fetched them yet.  Cursors are kept, and orz_reader_read does afterwards what
 *   it did before.
 * orz_reader_tensor_info: the tensors declared (0 = none) and, for the first `cap` of them, the element count and the element
 *   size; either array may be NULL.
 * orz_reader_read_elements: range k = count[k] elements of tensor tensor[k] from element first[k]; in any order, overlapping,
 *   repeated and empty ranges allowed, of one tensor or of several, tensors of single bytes among them.  Their INTERLEAVED bytes
 *   (count[k] * elems[tensor[k]] each) are written back to back in range order at d_dst (d_cap bytes on the reader's device);
 *   *dst_len = their sum.  The contract is orz_reader_read's:
 *   ORZ_EINVAL, before anything reaches the device: no declaration, NULL arrays with n_ranges > 0, a tensor number out of range,
 *     first + count above the tensor's element count or overflowing (the range is named), lengths whose sum overflows 64 bits,
 *     a device-resident container that overlaps [d_dst, d_dst + d_cap).
 *   ORZ_ENOMEM: d_cap below the sum of the bytes.  Nothing is written; *dst_len is filled.
 *   n_ranges == 0 or all counts zero: ORZ_OK, *dst_len == 0, nothing is launched.
 *   ORZ_EINVAL naming the member: payload damage in a plane BEFORE the furthest element asked of its tensor (the content of the
 *     output is then unspecified).  Damage behind that point is not seen.
 * The output does not depend on what d_dst held and nothing outside [d_dst, d_dst + *dst_len) is written in any case; a failed
 * read leaves the reader usable.  With a cursor budget planes are hit, resumed, fresh or uncached by orz_reader_read's policy.
 * The host waits as for orz_reader_read, whatever the number of ranges and tensors: 3 times with the cache off, twice with it
 * on.  orz_read_stats means what it means there: `ranges` the element ranges, `out_bytes` the sum of the bytes, `gather_ms` the
 * time of the launch that merges the planes into d_dst.
 * orz_reader_set_planes_pieces: orz_reader_set_planes for a container of orz_members_encode_planes_pieces_to_device: tensor j is
 *   the next elems[j] x pieces[j] members, pieces[j] (>= 1) to a plane, plane-major.  ORZ_EINVAL with nothing changed and nothing
 *   launched -- an earlier declaration and the cursors stay --: what orz_reader_set_planes refuses, a NULL pieces with
 *   n_tensors > 0, and what orz_decode_members_planes_pieces refuses of pieces and sizes ("tensor" for "destination").
 *   orz_reader_tensor_info then reports a tensor's elements over all its pieces, and orz_reader_read_elements serves element
 *   ranges exactly as above, but decodes ONLY THE PIECES a range touches, each only as far as the furthest element asked inside
 *   it, all of them side by side: the last rows of a tensor cost its last pieces, not the tensor.  orz_read_stats means what it
 *   means above, so members_decoded counts pieces; cursors work per member, so pieces are hit, resumed, fresh or uncached as any
 *   member; the host waits stay 3 and 2.
 * orz_reader_set_bases: the container holds DELTAS (orz_members_encode_deltas_to_device: the planes of tensor XOR base), and
 *   bases[j] is tensor j's base -- counts[j] x elems[j] bytes of device memory on the reader's device, as orz_reader_tensor_info
 *   reports them -- or NULL for none.  orz_reader_read_elements then returns RESTORED elements, planes XOR base, of the tensors
 *   that have a base, and the elements of the others as before.  n_tensors must be the number of tensors declared; n_tensors == 0
 *   withdraws the bases, and so does every successful orz_reader_set_planes / orz_reader_set_planes_pieces (a refused one leaves
 *   them).  The bases are BORROWED until they are withdrawn or the reader is closed, and only read: a base may overlap the
 *   container or another base.  The base of a tensor of no elements is not looked at.  ORZ_EINVAL with nothing changed: no
 *   declaration, n_tensors different from the tensors declared ("X bases for Y tensors"), bases == NULL with n_tensors > 0, a
 *   base whose bytes wrap the address space (the tensor is named).  Nothing is launched and the host does not wait; cursors are
 *   kept -- they hold planes and know nothing of bases --, so the same range read against another base decodes nothing anew.
 * orz_reader_read_elements WITH BASES: when a range that has elements names a tensor with a base, the ranges' base slices go up
 *   as one more column of the read's one upload and the launch that ends the read makes the XOR (ElementGatherDelta): no
 *   temporary, the same launches and the same host waits as the read without bases; a read none of whose non-empty ranges names
 *   such a tensor is the read without bases in every respect.  The base slice of range k -- count[k] x e bytes from bases[tensor[k]]
 *   + first[k] x e -- must be disjoint from ALL the bytes the read writes, [d_dst, d_dst + *dst_len), or BEGIN EXACTLY WHERE RANGE
 *   k's OWN BYTES GO: the read IN PLACE, the slice holding the base's elements on entry and the restored ones on return.  Any
 *   other overlap is ORZ_EINVAL naming the range, before anything reaches the device: the slice would be overwritten by, or
 *   overwrite, another range (two equal ranges cannot both be read in place).  After payload damage a slice read in place holds
 *   neither the base nor the tensor; a base given out of place is never written. */
int orz_reader_set_planes(orz_reader*, const uint32_t* elems, size_t n_tensors);
int orz_reader_set_planes_pieces(orz_reader*, const uint32_t* elems, const uint32_t* pieces, size_t n_tensors);
int orz_reader_set_bases(orz_reader*, const void* const* bases, size_t n_tensors);
/* orz_element_gather_time: the launch that ends ONE whole-tensor element read, alone: `count` elements (a multiple of 16) of `elem`
 * bytes whose planes lie count bytes apart from d_planes, merged to d_dst -- ElementGather, or with d_base (count x elem bytes)
 * ElementGatherDelta; *ms = milliseconds a launch, HIP events around `reps` launches after a warming one.  Everything on
 * `device`.  A measuring hook (tools/dev/delta_bench.py), not a data path. */
int orz_element_gather_time(int device, const void* d_planes, const void* d_base, void* d_dst, size_t count, uint32_t elem, int reps,
                            double* ms);
int orz_reader_tensor_info(orz_reader*, uint64_t* n_tensors, uint64_t* counts, uint32_t* elems, size_t cap);
int orz_reader_read_elements(orz_reader*, const uint64_t* tensor, const uint64_t* first, const uint64_t* count, size_t n_ranges,
                             uint8_t* d_dst, size_t d_cap, uint64_t* dst_len, orz_read_stats* stats);

/* The Huffman tables of `nchunks` chunks on the device, in the layout the encoder keeps them: a chunk is
 * orz_huffman_stride() = 389 + 389 + 240 entries (symbol ranks after a match / after a literal, long match lengths:
 * /root/reference/src/lz.rs:272-273,298-305), each of the three built as HuffmanTable::new_from_sym_weights(weights, 15)
 * (src/huffman.rs:27-111) followed by HuffmanEncoding::from_huffman_table (src/huffman.rs:118-141).  `lens` and `codes`
 * receive nchunks * stride entries.  Weights must be below 2^23 (a chunk holds at most 2^20 items, src/lib.rs:32);
 * ORZ_EINVAL otherwise.  `elapsed_us`, when not NULL, receives the HIP-event time of the one kernel launch. */
size_t orz_huffman_stride(void);
int orz_huffman_tables(int device, const uint32_t* weights, size_t nchunks, uint8_t* lens, uint16_t* codes, double* elapsed_us);

/* Symbol ranking of one launch: 512 contexts' tables (value[389], index[389], cnt lo/hi, sum lo/hi as u16, the encoder's
 * srstate layout, orz::kSrWords words a context) in and out; gsym[k] = symbol | excluded symbol << 16 in context order,
 * rstart[513] the first item of each context.  Runs HipBackend::symrank (backup, kernel, SymCheck, guarded rerun).
 * SymRankCoder::encode (src/symrank.rs:38-97) for every item of every context; `ranks` receives nitems ranks and `tables`
 * the tables as the chains left them (contexts without items unchanged).  `flags2`, when not NULL, receives the guard's two
 * counters (violations found after the first run, after the second; ORZ_SYMRANK_INJECT=k makes item k's first-run rank
 * wrong, as in an encode).  `elapsed_us`, when not NULL, the HIP-event time of the whole sequence.  ORZ_EINVAL, before
 * anything reaches the device, for rstart not monotone or not running from 0 to nitems, a symbol or excluded symbol of 389
 * or more, value[] / index[] of a context that are not inverse permutations, a count above 390 or a sum above
 * 1,151,320 (= 1,000,000 + 390 * 388, the largest the reference reaches). */
int orz_symrank_chains(int device, uint16_t* tables, const uint32_t* gsym, const uint32_t* rstart, size_t nitems,
                       uint16_t* ranks, uint32_t* flags2, double* elapsed_us);

/* FOR TESTS: the step machinery of the fast parse's round loop (orz_fast.h) run once on host arrays -- no stream object, no
 * encode; the launches are the product's own (orz_fast_step.h).  Arrays that a kernel writes are in/out: the caller pre-fills
 * them and gets them back whole, so what a kernel leaves alone comes back as it went in.  With nsub = ceil(n / 4096) and
 * ntile = ceil(n / tile), in entries: wbytes n + 2 (window offsets SBVEC_PREMATCH_LEN - 2 .. window end), ev n + 520, ty / nl /
 * x0 / pt n + 4608, x1 (nsub + 2) * 240, x2 (ntile + 2) * 240, centry nsub + 2, tentry ntile + 2, sbits n / 64 + 16, cm
 * (nsub + 2) * 256.
 * orz_fast_step_path: the path stage of one step over the tiles t_lo .. t_hi, the path entering at window offset `entry`
 * (tentry[t_lo]).  form 0: PathUpWave deciding, with a FastRetireDone part of zero positions; 1: FastDecide, then PathUpWave;
 * 2: the thread-per-item forms (FastDecide, PathSeg, PathChunk, PathTileDown, PathMark, CountWave); 0 and 1 go on with
 * PathTileDown and PathMarkWave.  lds_bytes, when not NULL, receives PathTileDown's LDS need (0 = the global-memory walk).
 * ORZ_EINVAL, before anything reaches the device, for a length field of ev[0 .. n) that is neither 0 nor 4 .. 240, an entry
 * outside [lo, lo + 240), a tile that is not a multiple of 4096, tiles outside the block.
 * orz_fast_step_counts: count != 0: CountWave over all subtiles (cm from sbits), else cm as given ([rows][256]); FastPrefix
 * {s0, s1, ext, cpt, live_end} alone into cp and as the prefix half of FlipPrefixWave (no positions to flip) into cp2
 * ([rows + 1][256] each, row s0 given); FastItemTotal over cp into acc2 (acc, hotacc); OrdWave into ord and OrdWave2 into ord2
 * (n entries each), both from cp.
 * orz_fast_step_horizon: FastHorizon over the subtiles s0 .. s1 alone into hz and as the horizon half of RetireHorizonWave (no
 * retiring positions) into hz2 ([s1 + 1][256][4] each); cp [rows][256] with rows >= s1 + 2, hpre [4097][256]. */
int orz_fast_step_path(int device, unsigned form, uint32_t n, uint32_t tile, uint32_t t_lo, uint32_t t_hi, uint32_t entry,
                       const uint8_t* wbytes, const uint32_t* ev, uint8_t* ty, uint8_t* nl, uint8_t* x0, uint8_t* x1, uint8_t* x2,
                       uint32_t* centry, uint32_t* tentry, uint64_t* sbits, uint8_t* pt, uint32_t* cm, uint64_t* lds_bytes);
int orz_fast_step_counts(int device, uint32_t n, const uint8_t* wbytes, const uint64_t* sbits, int count, uint32_t s0, uint32_t s1,
                         uint32_t ext, uint32_t cpt, uint32_t live_end, uint32_t rows, uint32_t* cm, uint32_t* cp, uint32_t* cp2,
                         uint32_t* ord, uint32_t* ord2, uint32_t* acc2);
int orz_fast_step_horizon(int device, const uint32_t* cp, uint32_t rows, const uint32_t* hpre, uint32_t s0, uint32_t s1, uint32_t* hz,
                          uint32_t* hz2);

int orz_device_count(void);
const char* orz_last_error(void);
const char* orz_version(void);

#ifdef __cplusplus
}
#endif
#endif
