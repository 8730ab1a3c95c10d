// orz_capi.hip -- C ABI of liborz_hip.so (declared in include/orz_hip.h).
//
// Host side of the MI355X encoder: mirrors the reference's LZEncoder / orz::encode call surface
// (/root/reference/src/lz.rs:69-95, src/lib.rs:58-92) on top of StreamEncoder<HipBackend>.
// There is no CPU fallback: if no HIP device is usable every constructor fails with ORZ_ENODEV.
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <atomic>
#include <thread>
#include <vector>

#include "../../include/orz_hip.h"
#include "backend_hip.h"
#include "orz_decode_device.h"
#include "orz_decode_index.h"
#include "orz_decode_range.h"
#include "orz_decode_scatter.h"
#include "orz_host_decode.h"
#include "orz_planes.h"
#include "orz_chain.h"
#include "orz_read_elements.h"
#include "orz_decode_check.h"
#include "orz_stream.h"
#include "orz_fast_step.h"

namespace {
// An encoder drives three HIP streams (parse; symbol ranking; Huffman + packing) and the members interface runs several
// encoders side by side.  The HIP runtime multiplexes all streams of a process onto GPU_MAX_HW_QUEUES hardware queues
// (4 by default): streams that share a queue run their kernels one after another, so another member's 50 ms
// symbol-ranking launch stalls a parse behind it.  Measured on MI355X, 8 encoders, 64 MiB members, -l1: 4 queues
// 344 MB/s, 8: 385, 16: 443, 32: 437.  The variable is read when the HIP runtime initialises, so it is set here, when
// the library is loaded, unless the host process has chosen a value itself.
struct HwQueueDefault {
    HwQueueDefault() { setenv("GPU_MAX_HW_QUEUES", "16", 0); }
} g_hw_queue_default;


thread_local std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

orz::Cfg to_cfg(const orz_lzcfg* c) {
    return orz::Cfg{(int)c->match_depth, (int)c->lazy_match_depth1, (int)c->lazy_match_depth2};
}
bool cfg_ok(const orz_lzcfg* c) {
    return c && c->match_depth >= 1 && c->match_depth <= 200 && c->lazy_match_depth1 <= 200 &&
           c->lazy_match_depth2 <= 200;
}

constexpr unsigned kDefaultSeg = 62;  // window: 0 = as many segments as parse waves fit the device at once

unsigned env_u(const char* name, unsigned dflt) {
    const char* v = std::getenv(name);
    return v && *v ? (unsigned)std::strtoul(v, nullptr, 10) : dflt;
}

// ---- shared by the decode entry points
unsigned decode_slots() { return env_u("ORZ_DECODE_SLOTS", 2048); }  // members in flight at once
bool device_ok(int device) { return device >= 0 && device < orz_device_count(); }
void put_stats(orz_decode_stats* out, const orz::DecodeStats& st) {
    if (!out) return;
    out->members = st.members; out->in_bytes = st.in_bytes; out->out_bytes = st.out_bytes;
    out->launches = st.launches; out->kernel_ms = st.kernel_ms; out->total_s = st.total_s;
}
// Runs f.  What it throws becomes the thread's message and ORZ_EBADMSG (a digest that differs), ORZ_ENOMEM (a buffer of the
// caller's that is too small, memory that ran out) or ORZ_EINVAL (anything else).
template <class F>
int mapped(F&& f) {
    try {
        f();
        return ORZ_OK;
    } catch (const orz::DecodeDigestError& e) {
        return fail(ORZ_EBADMSG, e.what());
    } catch (const orz::DecodeCapacityError& e) {
        return fail(ORZ_ENOMEM, e.what());
    } catch (const std::bad_alloc& e) {
        return fail(ORZ_ENOMEM, e.what());
    } catch (const std::exception& e) {
        return fail(ORZ_EINVAL, e.what());
    }
}

// The four decodes into a list of destinations (scatter, planes, pieces, verified) around their drivers: `waits`, the entry's own
// thread-local count of host waits, answers for this call from here on; `bad`, the entry's own argument check, and the device are
// refused; run(be, members, st) drives a backend of the call's own; the member count is stored however the call ends, the
// stats when it succeeds.
template <class Run>
int decode_into_list(uint64_t& waits, bool bad, int device, size_t* n_members_out, orz_decode_stats* stats, Run&& run) {
    waits = 0;
    if (bad) return fail(ORZ_EINVAL, "bad argument");
    if (!device_ok(device)) return fail(ORZ_ENODEV, "no such HIP device");
    uint64_t members = 0;
    orz::DecodeScatterStats st;
    const int rc = mapped([&] {
        orz::HipBackend be(device);
        run(be, members, st);
    });
    waits = st.host_waits;
    if (n_members_out) *n_members_out = (size_t)members;
    if (rc == ORZ_OK) put_stats(stats, st);
    return rc;
}
// `bytes` (or none) handed to the caller as a malloc'ed buffer, released with orz_free
int give_bytes(const std::vector<uint8_t>& bytes, uint8_t** dst, size_t* dst_len) {
    uint8_t* p = (uint8_t*)std::malloc(bytes.size() ? bytes.size() : 1);
    if (!p) return fail(ORZ_ENOMEM, "malloc failed");
    if (!bytes.empty()) std::memcpy(p, bytes.data(), bytes.size());
    *dst = p;
    *dst_len = bytes.size();
    return ORZ_OK;
}

using Enc = orz::StreamEncoder<orz::HipBackend>;

// parse mode of a new encoder: the GPU-native fast mode unless ORZ_MODE=exact asks for the reference-identical parse
bool mode_from_env() {
    const char* v = std::getenv("ORZ_MODE");
    return !(v && std::string(v) == "exact");
}

// ORZ_VERIFY=decode (bin/orz encode --verify): every finished stream goes through the library's OWN decoder
// (orz_host_decode.h, src/lz.rs:366-478) before its bytes leave the library, and must reproduce the input bit for bit;
// what the per-block validity gate (orz_verify.h) cannot see -- symbol ranking, Huffman tables, bit packing -- is covered by
// this.  The check is incremental: input and output are fed as they arrive, a chunk is decoded as soon as it is complete, so
// the streaming entry point (orz_encode) verifies a block's bytes BEFORE it hands them to the caller's sink.
bool verify_decode_on() {
    const char* v = std::getenv("ORZ_VERIFY");
    return v && std::string(v) == "decode";
}
// a whole stream in memory against its input (host or device resident)
void verify_stream_decode(const uint8_t* src, size_t n, bool src_on_device, const uint8_t* out, size_t out_len) {
    std::vector<uint8_t> host;
    if (src_on_device && n) {
        host.resize(n);
        ORZ_HIP_CHECK(hipMemcpy(host.data(), src, n, hipMemcpyDeviceToHost));
        src = host.data();
    }
    orz::host::DecodeCheck chk;
    chk.feed_input(src, n);
    chk.feed_output(out, out_len);
    chk.finish();
}

unsigned window_for(const orz::HipBackend& be, const orz_lzcfg& c, unsigned asked) {
    if (asked) return asked;
    const size_t dmax = std::max(c.match_depth, std::max(c.lazy_match_depth1, c.lazy_match_depth2));
    return be.resident_parse_waves(orz::ParseLds::make((uint32_t)dmax, false).total);
}

}  // namespace

// ---- the results of orz_stream_encode: page-locked host buffers from a small process-wide pool.
// A stream's bytes used to come to the host by a blocking copy into freshly malloc'ed (pageable, untouched) memory after the
// last kernel of every call: 5.5 ms for the 28 MB of the 100 MB text workload, 0.6 ms into a page-locked buffer.
// Allocating a page-locked buffer costs more than the copy, so buffers are kept:
// a capacity is a power of two (a caller's streams of similar size reuse each other's buffers), at most two idle buffers wait
// for the next call, and the idle ones are released with the last stream handle.  Results under 1 MiB stay malloc'ed.
namespace {
constexpr size_t kPoolMin = size_t(1) << 20;
constexpr size_t kPoolIdleMax = 2;
struct ResultPool {
    std::mutex mu;
    std::map<void*, size_t> out;                  // handed to callers: pointer -> capacity
    std::vector<std::pair<void*, size_t>> idle;   // waiting for the next call
    size_t handles = 0;                           // live orz_stream handles
    static size_t capacity_for(size_t n) {
        size_t c = kPoolMin;
        while (c < n) c <<= 1;
        return c;
    }
    // a buffer of n bytes or more; nullptr when page-locked memory cannot be had (the caller falls back to malloc)
    void* take(size_t n) {
        const size_t cap = capacity_for(n);
        {
            std::lock_guard<std::mutex> g(mu);
            size_t best = idle.size();
            for (size_t i = 0; i < idle.size(); i++)
                if (idle[i].second >= cap && (best == idle.size() || idle[i].second < idle[best].second)) best = i;
            if (best < idle.size()) {
                void* p = idle[best].first;
                out[p] = idle[best].second;
                idle.erase(idle.begin() + (long)best);
                return p;
            }
        }
        void* p = nullptr;
        if (hipHostMalloc(&p, cap, hipHostMallocPortable) != hipSuccess || !p) {
            (void)hipGetLastError();
            return nullptr;
        }
        std::lock_guard<std::mutex> g(mu);
        out[p] = cap;
        return p;
    }
    // true: p was a pool buffer and is taken back (kept idle, or released when two wait already or no stream is left)
    bool give(void* p) {
        size_t cap = 0;
        {
            std::lock_guard<std::mutex> g(mu);
            auto it = out.find(p);
            if (it == out.end()) return false;
            cap = it->second;
            out.erase(it);
            if (handles > 0 && idle.size() < kPoolIdleMax) {
                idle.emplace_back(p, cap);
                return true;
            }
        }
        (void)hipHostFree(p);
        return true;
    }
    void handle_born() {
        std::lock_guard<std::mutex> g(mu);
        handles++;
    }
    void handle_gone() {
        std::vector<std::pair<void*, size_t>> drop;
        {
            std::lock_guard<std::mutex> g(mu);
            if (handles > 0 && --handles == 0) drop.swap(idle);
        }
        for (auto& b : drop) (void)hipHostFree(b.first);
    }
};
ResultPool& result_pool() {
    static ResultPool* const pool = new ResultPool;  // (never destroyed: orz_free may run during process teardown)
    return *pool;
}
}  // namespace

struct orz_stream {
    std::unique_ptr<orz::HipBackend> be;
    std::unique_ptr<Enc> enc;
    orz_lzcfg cfg;
    unsigned seg, win;
    orz::ItemTrace trace;
    bool tracing = false;
    orz::FastTableCapture tables;  // (tests) orz_stream_fast_tables
    orz::FastRepairProbe probe;    // (tests) orz_stream_repair_probe
    bool fast = false;
    unsigned ftile = orz::kFastTile, frounds = orz::kFastRounds;
    unsigned unit = 0;  // fast mode: bytes per unit of a block; 0 = the encoder's default (a stream that has the GPU to itself)
    double kernel_ms[4] = {0, 0, 0, 0};
    uint64_t kernel_n[4] = {0, 0, 0, 0};
    std::vector<orz::KernelRow> ktable;  // profile mode: every kernel of the last encode by name (orz_stream_get_kernel_table)
    // Build the encoder for the current settings.  The new one is constructed BEFORE the old one is dropped (a constructor
    // that throws -- bad tile size, failed allocation -- leaves the handle as it was); callers that change settings go
    // through `reconfigure`, which also restores them.
    void rebuild() {
        std::unique_ptr<Enc> fresh;
        try {
            fresh.reset(new Enc(*be, to_cfg(&cfg), seg, fast ? 64 : window_for(*be, cfg, win), fast, ftile, frounds));
        } catch (const std::exception&) {
            // a stream's state is ~5 GB: two of them may not fit a loaded device where one does.  Was the failure a bad
            // setting, the second attempt fails the same way and the handle has no encoder left (every call on it reports
            // that); was it memory, dropping the old encoder first makes room.
            if (!enc) throw;
            (void)hipGetLastError();
            enc.reset();
            be->clear_graphs();
            fresh.reset(new Enc(*be, to_cfg(&cfg), seg, fast ? 64 : window_for(*be, cfg, win), fast, ftile, frounds));
        }
        if (fast && unit && !getenv("ORZ_FAST_UNIT")) fresh->set_unit(unit);
        be->clear_graphs();  // (captured launches hold the old encoder's buffer addresses)
        enc = std::move(fresh);
        enc->trace = tracing ? &trace : nullptr;
        enc->tables = &tables;
        enc->repair_probe = &probe;
    }
    // apply a settings change + rebuild as a transaction: on failure every setting is as before and the old encoder lives on
    template <class Change>
    void reconfigure(Change change) {
        const unsigned seg0 = seg, win0 = win, ftile0 = ftile, frounds0 = frounds;
        const bool fast0 = fast;
        change();
        try {
            rebuild();
        } catch (...) {
            seg = seg0; win = win0; ftile = ftile0; frounds = frounds0; fast = fast0;
            if (!enc) {  // (the old encoder was dropped to make room: bring it back with the old settings)
                try { rebuild(); } catch (...) {}
            }
            throw;
        }
    }
};

struct orz_lz_encoder {
    std::unique_ptr<orz::HipBackend> be;
    std::unique_ptr<Enc> enc;
    orz_lzcfg cfg{0, 0, 0};
    unsigned seg, win;
    // chunks of the block parsed last, handed out one per encode() call
    std::vector<uint8_t> framed;  // { LEB128(t) chunk[t] }*
    size_t framed_pos = 0;
    std::vector<size_t> chunk_end_spos;
    size_t next_chunk = 0;
    size_t expect_spos = 0;
    bool first_block = true;
    bool slid = false;  // forward() was called: the two bytes in front of the device window are history, not sentinel
};

extern "C" {

const char* orz_last_error(void) { return g_err.c_str(); }
const char* orz_version(void) { return "orz_hip 0.1 (bitstream: richox/orz 1.6.1)"; }

int orz_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int orz_lzcfg_from_level(int level, orz_lzcfg* out) {  // src/main.rs:97-102
    if (!out) return fail(ORZ_EINVAL, "null cfg");
    switch (level) {
        case 0: *out = orz_lzcfg{5, 3, 2}; return ORZ_OK;
        case 1: *out = orz_lzcfg{15, 9, 6}; return ORZ_OK;
        case 2: *out = orz_lzcfg{45, 27, 18}; return ORZ_OK;
        default: return fail(ORZ_EINVAL, "invalid level");
    }
}

void orz_free(void* p) {
    if (!p) return;
    if (!result_pool().give(p)) std::free(p);
}

// ------------------------------------------------------------------------------ orz_stream
static orz_stream* stream_new(int device, const orz_lzcfg* cfg, bool lone) {
    if (!cfg_ok(cfg)) { fail(ORZ_EINVAL, "bad LZCfg"); return nullptr; }
    try {
        if (device < 0 || device >= orz_device_count()) { fail(ORZ_ENODEV, "no such HIP device"); return nullptr; }
        std::unique_ptr<orz_stream> s(new orz_stream);
        s->be.reset(new orz::HipBackend(device, lone));
        s->be->enable_arena();
        s->cfg = *cfg;
        s->seg = env_u("ORZ_SEG", kDefaultSeg);
        s->win = env_u("ORZ_WIN", 0);
        s->fast = mode_from_env();
        s->ftile = env_u("ORZ_FAST_TILE", orz::kFastTile);
        s->frounds = env_u("ORZ_FAST_ROUNDS", orz::kFastRounds);
        s->be->set_graphs(env_u("ORZ_GRAPHS", 1) != 0);
        if (!lone) s->unit = orz::kNewMax;  // one of several encoders on the device: whole blocks (orz_stream.h, unit_)
        s->rebuild();
        result_pool().handle_born();
        return s.release();
    } catch (const std::exception& e) {
        fail(ORZ_ENODEV, e.what());
        return nullptr;
    }
}
orz_stream* orz_stream_new(int device, const orz_lzcfg* cfg) { return stream_new(device, cfg, true); }
void orz_stream_free(orz_stream* s) {
    if (!s) return;
    s->enc.reset();
    s->be.reset();
    delete s;
    result_pool().handle_gone();
}
int orz_stream_set_tuning(orz_stream* s, unsigned seg_bytes, unsigned window_segs) {
    if (!s) return fail(ORZ_EINVAL, "null stream");
    try {
        s->reconfigure([&] {
            if (seg_bytes) s->seg = seg_bytes;
            if (window_segs) s->win = window_segs;
        });
        return ORZ_OK;
    } catch (const std::exception& e) {
        return fail(ORZ_EINVAL, e.what());
    }
}
int orz_stream_set_mode(orz_stream* s, int mode, unsigned tile_bytes, unsigned rounds) {
    if (!s || (mode != ORZ_MODE_EXACT && mode != ORZ_MODE_FAST)) return fail(ORZ_EINVAL, "bad mode");
    try {
        s->reconfigure([&] {
            s->fast = mode == ORZ_MODE_FAST;
            if (tile_bytes) s->ftile = tile_bytes;
            if (rounds) s->frounds = rounds;
        });
        return ORZ_OK;
    } catch (const std::exception& e) {
        return fail(ORZ_EINVAL, e.what());
    }
}
int orz_stream_set_profile(orz_stream* s, int on) {
    if (!s) return fail(ORZ_EINVAL, "null stream");
    s->be->set_profile(on != 0);
    return ORZ_OK;
}
int orz_stream_get_kernel_times(orz_stream* s, double* ms4, uint64_t* launches4) {
    if (!s || !ms4 || !launches4) return fail(ORZ_EINVAL, "null argument");
    for (int i = 0; i < 4; i++) { ms4[i] = s->kernel_ms[i]; launches4[i] = s->kernel_n[i]; }
    return ORZ_OK;
}
long orz_stream_get_kernel_table(orz_stream* s, orz_kernel_row* rows, size_t cap) {
    if (!s) return fail(ORZ_EINVAL, "null stream");
    for (size_t i = 0; i < s->ktable.size() && i < cap && rows; i++) {
        std::memset(&rows[i], 0, sizeof rows[i]);
        std::strncpy(rows[i].name, s->ktable[i].name.c_str(), sizeof rows[i].name - 1);
        rows[i].ms = s->ktable[i].ms;
        rows[i].launches = s->ktable[i].launches;
    }
    return (long)s->ktable.size();
}
int orz_stream_get_config(orz_stream* s, orz_stream_config* out) {
    if (!s || !out) return fail(ORZ_EINVAL, "null argument");
    if (!s->enc) return fail(ORZ_ENOMEM, "the stream has no encoder (a reconfiguration ran out of device memory)");
    out->mode = s->enc->fast() ? ORZ_MODE_FAST : ORZ_MODE_EXACT;
    out->segment_bytes = s->enc->seg_size();
    out->window_segments = s->enc->window_segs();
    out->fast_tile_bytes = s->enc->fast_tile();
    out->fast_rounds = s->enc->fast_rounds();
    out->fast_row_entries = s->enc->fast_row();
    out->unit_bytes = s->enc->unit_bytes();
    return ORZ_OK;
}
// One stream through the encoder with the finished stream left in device memory (`d_dst` / `d_cap`: the caller's buffer, or nullptr
// for the encoder's own): the common body of orz_stream_encode and orz_stream_encode_to_device.  Throws.
static orz::StreamEncoder<orz::HipBackend>::DeviceResult stream_encode_device(orz_stream* s, const void* src, size_t n, int src_on_device,
                                                                              uint8_t* d_dst, size_t d_cap, orz_encode_stats* stats) {
    orz::HipBackend& be = *s->be;
    be.set_timing(stats != nullptr);
    be.begin_encode();
    struct Events {  // destroyed on every path out of this function
        orz::HipBackend& be;
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { be.set_end_event(nullptr); if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev{be};
    ORZ_HIP_CHECK(hipSetDevice(be.device()));
    ORZ_HIP_CHECK(hipEventCreate(&ev.a));
    ORZ_HIP_CHECK(hipEventCreate(&ev.b));
    ORZ_HIP_CHECK(hipEventRecord(ev.a, be.stream()));
    be.set_end_event(ev.b);  // (recorded behind the stream's last frame kernel, before the closing wait: finish_device)
    s->trace.clear();
    struct Pin {  // host input: page-lock it for the call so the block uploads are real asynchronous DMA
        void* p = nullptr;
        ~Pin() { if (p) (void)hipHostUnregister(p); }
    } pin;
    bool pinned = false;
    if (!src_on_device && n >= (1u << 20) && hipHostRegister(const_cast<void*>(src), n, hipHostRegisterDefault) == hipSuccess) {
        pin.p = const_cast<void*>(src);
        pinned = true;
    } else {
        (void)hipGetLastError();  // (registration refused: pageable copies, synchronised per block)
    }
    struct Disarm {  // (tests) a capture is armed for ONE encode, whether it reached the block or not
        orz::FastTableCapture& c;
        ~Disarm() { c.arm = -1; }
    } disarm{s->tables};
    struct DisarmProbe {
        orz::FastRepairProbe& c;
        ~DisarmProbe() { c.arm = -1; c.inj_ty.clear(); c.inj_nl.clear(); }
    } disarm_probe{s->probe};
    struct ClearPatches {  // (tests) an item patch list holds for ONE encode, however it ends
        orz_stream* s;
        ~ClearPatches() { if (s->enc) s->enc->clear_item_patches(); }
    } clear_patches{s};
    const auto r = orz::encode_stream_device(*s->enc, be, (const uint8_t*)src, n, src_on_device != 0, d_dst, d_cap, pinned);
    if (stats) {
        float total = 0;
        ORZ_HIP_CHECK(hipEventElapsedTime(&total, ev.a, ev.b));
        const orz::EncodeStats& st = s->enc->stats;
        stats->blocks = st.blocks; stats->sweeps = st.sweeps; stats->seg_evals = st.seg_evals;
        stats->items = st.items; stats->chunks = st.chunks; stats->in_bytes = st.in_bytes;
        stats->out_bytes = r.len;
        stats->t_prep_s = st.t_prep; stats->t_parse_s = st.t_parse; stats->t_post_s = st.t_post;
        stats->parse_kernel_ms = be.collect_timed(&stats->parse_launches, s->kernel_ms, s->kernel_n);
        stats->total_ms = total;
        stats->host_syncs = st.host_syncs + be.take_host_syncs();
        if (be.profile()) s->ktable = be.collect_named();
    }
    return r;
}
int orz_stream_encode(orz_stream* s, const void* src, size_t n, int src_on_device, uint8_t** dst, size_t* dst_len,
                      orz_encode_stats* stats) {
    if (!s || !dst || !dst_len || (!src && n)) return fail(ORZ_EINVAL, "null argument");
    if (!s->enc) return fail(ORZ_ENOMEM, "the stream has no encoder (a reconfiguration ran out of device memory)");
    try {
        const auto r = stream_encode_device(s, src, n, src_on_device, nullptr, 0, stats);
        // the finished stream comes to the host in ONE copy (round 6; before: a wait for the sizes and one for the bytes of every
        // block) -- into a page-locked buffer of the result pool when it is 1 MiB or more
        uint8_t* p = r.len >= kPoolMin ? (uint8_t*)result_pool().take(r.len) : nullptr;
        if (!p) p = (uint8_t*)std::malloc(r.len ? r.len : 1);
        if (!p) return fail(ORZ_ENOMEM, "out of host memory");
        hipError_t ce = hipMemcpyAsync(p, r.data, r.len, hipMemcpyDeviceToHost, s->be->stream());
        if (ce == hipSuccess) ce = hipStreamSynchronize(s->be->stream());
        if (stats) stats->host_syncs += 1;
        if (ce != hipSuccess) { orz_free(p); return fail(ORZ_ENODEV, hipGetErrorString(ce)); }
        if (verify_decode_on()) {
            try { verify_stream_decode((const uint8_t*)src, n, src_on_device != 0, p, r.len); } catch (...) { orz_free(p); throw; }
        }
        *dst_len = r.len;
        *dst = p;
        return ORZ_OK;
    } catch (const std::invalid_argument& e) {  // (tests: a decision field of another size than the armed block's)
        return fail(ORZ_EINVAL, e.what());
    } catch (const std::bad_alloc&) {
        return fail(ORZ_ENOMEM, "out of host memory");
    } catch (const std::exception& e) {
        return fail(ORZ_ENODEV, e.what());
    }
}
size_t orz_stream_bound(size_t n) { return orz::stream_bound(n); }
int orz_stream_encode_to_device(orz_stream* s, const void* src, size_t n, int src_on_device, uint8_t* d_dst, size_t d_cap,
                                size_t* dst_len, orz_encode_stats* stats) {
    if (!s || !d_dst || !dst_len || (!src && n)) return fail(ORZ_EINVAL, "null argument");
    if (!s->enc) return fail(ORZ_ENOMEM, "the stream has no encoder (a reconfiguration ran out of device memory)");
    try {
        const auto r = stream_encode_device(s, src, n, src_on_device, d_dst, d_cap, stats);
        if (verify_decode_on()) {
            std::vector<uint8_t> host(r.len);
            ORZ_HIP_CHECK(hipMemcpy(host.data(), r.data, r.len, hipMemcpyDeviceToHost));
            verify_stream_decode((const uint8_t*)src, n, src_on_device != 0, host.data(), host.size());
        }
        *dst_len = r.len;
        return ORZ_OK;
    } catch (const std::bad_alloc&) {
        return fail(ORZ_ENOMEM, "out of host memory");
    } catch (const std::exception& e) {
        const std::string msg = e.what();
        return fail(msg.find("output buffer is too small") != std::string::npos ? ORZ_ENOMEM : ORZ_ENODEV, msg);
    }
}

int orz_stream_set_item_trace(orz_stream* s, int on) {
    if (!s || !s->enc) return fail(ORZ_EINVAL, "null stream");
    s->tracing = on != 0;
    s->enc->trace = s->tracing ? &s->trace : nullptr;
    if (!on) s->trace.clear();
    return ORZ_OK;
}
long orz_stream_get_item_trace(orz_stream* s, orz_item* out, size_t cap) {
    if (!s) return fail(ORZ_EINVAL, "null stream");
    const orz::ItemTrace& t = s->trace;
    const size_t n = t.pos.size();
    for (size_t i = 0; i < n && i < cap && out; i++) {
        orz_item it;
        it.block = t.block[i]; it.pos = t.pos[i]; it.symbol = t.sym[i]; it.rank = t.rank[i]; it.ctx = t.ctx[i];
        it.robits = t.rob[i]; it.unlikely = t.unl[i]; it.enc_len = t.enc[i]; it.after_literal = t.al[i]; it.match_len = t.mlen[i];
        it.src = t.src[i];
        out[i] = it;
    }
    return (long)n;
}

// (tests of the validity gate) item patches of the next encode, see include/orz_hip.h and orz_verify.h
int orz_stream_set_item_patches(orz_stream* s, const orz_item_patch* patches, size_t n) {
    if (!s || !s->enc) return fail(ORZ_EINVAL, "null stream");
    static_assert(sizeof(orz_item_patch) == sizeof(orz::ItemPatch), "orz_item_patch is the device's ItemPatch");
    try {
        ORZ_HIP_CHECK(hipSetDevice(s->be->device()));
        s->enc->set_item_patches(reinterpret_cast<const orz::ItemPatch*>(patches), n);
        return ORZ_OK;
    } catch (const std::invalid_argument& e) {
        return fail(ORZ_EINVAL, e.what());
    } catch (const std::bad_alloc&) {
        return fail(ORZ_ENOMEM, "out of memory");
    } catch (const std::exception& e) {
        return fail(ORZ_ENODEV, e.what());
    }
}

// (tests) the static tables of one block of the fast parse, see include/orz_hip.h
long orz_stream_fast_tables(orz_stream* s, int arm_block, const char* name, void* dst, size_t cap) {
    if (!s || !s->enc) return fail(ORZ_EINVAL, "null stream");
    if (!s->enc->fast()) return fail(ORZ_EINVAL, "the exact mode has no such tables");
    orz::FastTableCapture& c = s->tables;
    if (!name) {
        if (arm_block > 65535) return fail(ORZ_EINVAL, "bad block number");
        c.arm = arm_block < 0 ? -1 : arm_block;
        c.taken = false;
        c.tab.clear();
        return 0;
    }
    if (!c.taken) return fail(ORZ_EINVAL, "no block was captured");
    const std::vector<uint8_t>* t = c.find(name);
    if (!t) return fail(ORZ_EINVAL, "no such table");
    if (dst && cap) std::memcpy(dst, t->data(), std::min(cap, t->size()));
    return (long)t->size();
}

// (tests) the repair stage of one block of the fast parse, pass by pass, see include/orz_hip.h
int orz_stream_arm_repair_probe(orz_stream* s, int block, const uint8_t* ty, const uint8_t* nl, size_t n) {
    if (!s || !s->enc) return fail(ORZ_EINVAL, "null stream");
    if (!s->enc->fast()) return fail(ORZ_EINVAL, "the exact mode has no repair stage");
    if (block > 65535) return fail(ORZ_EINVAL, "bad block number");
    orz::FastRepairProbe& c = s->probe;
    if (block >= 0 && (ty || nl || n)) {
        if (const char* why = orz::FastRepairProbe::field_invalid(ty, nl, n)) return fail(ORZ_EINVAL, why);
    }
    c.arm = block < 0 ? -1 : block;
    c.taken = false;
    c.tab.clear();
    c.inj_ty.clear();
    c.inj_nl.clear();
    if (block >= 0 && n) { c.inj_ty.assign(ty, ty + n); c.inj_nl.assign(nl, nl + n); }
    return ORZ_OK;
}
long orz_stream_repair_probe(orz_stream* s, const char* name, void* dst, size_t cap) {
    if (!s || !s->enc || !name) return fail(ORZ_EINVAL, "null argument");
    const orz::FastRepairProbe& c = s->probe;
    if (!c.taken) return fail(ORZ_EINVAL, "no block was probed");
    const std::vector<uint8_t>* t = c.find(name);
    if (!t) return fail(ORZ_EINVAL, "no such table");
    if (dst && cap) std::memcpy(dst, t->data(), std::min(cap, t->size()));
    return (long)t->size();
}

// ------------------------------------------------------------------------------ members
struct orz_members {
    std::vector<orz_stream*> workers;
    std::map<int, std::pair<uint8_t*, size_t>> arena;  // per device: where the finished members of a job are collected (orz_members_encode)
};
orz_members* orz_members_new_multi(const int* devices, int n_devices, const orz_lzcfg* cfg, int jobs_per_device) {
    if (!cfg_ok(cfg) || !devices || n_devices < 1 || n_devices > 64 || jobs_per_device < 1 || jobs_per_device > 64) {
        fail(ORZ_EINVAL, "bad argument");
        return nullptr;
    }
    std::unique_ptr<orz_members> m(new orz_members);
    auto drop = [&]() { for (orz_stream* w : m->workers) orz_stream_free(w); m->workers.clear(); };
    for (int d = 0; d < n_devices; d++)
        for (int i = 0; i < jobs_per_device; i++) {
            orz_stream* s = stream_new(devices[d], cfg, n_devices * jobs_per_device == 1);
            if (!s) { drop(); return nullptr; }
            if (jobs_per_device > 1 && !s->fast) {  // exact mode: several streams share the GPU: a smaller speculative window each
                s->win = env_u("ORZ_MEMBER_WIN", std::max(256u, window_for(*s->be, *cfg, 0) / (unsigned)jobs_per_device));
                try { s->reconfigure([] {}); } catch (const std::exception& e) { fail(ORZ_ENODEV, e.what()); orz_stream_free(s); drop(); return nullptr; }
            }
            m->workers.push_back(s);
        }
    return m.release();
}
orz_members* orz_members_new(int device, const orz_lzcfg* cfg, int jobs) { return orz_members_new_multi(&device, 1, cfg, jobs); }
void orz_members_free(orz_members* m) {
    if (!m) return;
    for (orz_stream* w : m->workers) orz_stream_free(w);
    for (auto& kv : m->arena)
        if (kv.second.first) { (void)hipSetDevice(kv.first); (void)hipFree(kv.second.first); }
    delete m;
}
// The members of a job on the workers' devices.  A worker leaves a finished member in its encoder's own device buffer
// (encode_stream_device: one host wait per block, one per member) and moves it -- device to device, on its copy stream, no host
// wait: the next member's frame kernels queue behind the copy -- into the job's ARENA on that device at an offset drawn from an
// atomic counter; `place[k]` says where member k lies.  Arena = the caller's buffer (orz_members_encode_to_device) or one the
// members object owns; a member that does not fit an OWNED arena goes to host memory instead (incompressible input: the arena
// is sized for ratio 0.5), into the caller's it fails the job.  What a worker encodes is a list of WORK ITEMS, one member each:
// the cuts of one input every member_bytes (orz_members_encode) or the caller's own segments (orz_members_encode_segments).
namespace {
struct MemberItem { const uint8_t* p; size_t len; };
// the work items of one contiguous input cut every member_bytes: one empty member for n == 0
void member_cuts(const void* src, size_t n, size_t member_bytes, std::vector<MemberItem>& items) {
    const size_t nm = n == 0 ? 1 : (n + member_bytes - 1) / member_bytes;
    items.resize(nm);
    for (size_t i = 0; i < nm; i++) {
        const size_t off = i * member_bytes;
        items[i] = MemberItem{(const uint8_t*)src + off, n == 0 ? 0 : std::min(member_bytes, n - off)};
    }
}
struct MemberPlace { int device = -1; size_t off = 0, len = 0; std::vector<uint8_t> host; };
struct MemberArena {
    int device; uint8_t* p; size_t cap; bool caller;
    std::atomic<size_t> used{0};
    MemberArena(int d, uint8_t* q, size_t c, bool cl) : device(d), p(q), cap(c), caller(cl) {}
};
int members_run(orz_members* m, const std::vector<MemberItem>& items, int src_on_device, std::vector<std::unique_ptr<MemberArena>>& arenas,
                std::vector<MemberPlace>& place) {
    const size_t nm = items.size();
    std::atomic<size_t> next{0};
    std::atomic<int> rc{ORZ_OK};
    std::string err;
    const bool verify = verify_decode_on();
    auto arena_of = [&](int dev) -> MemberArena* {
        for (auto& a : arenas) if (a->device == dev) return a.get();
        return nullptr;
    };
    auto work = [&](orz_stream* s) {
        bool copied = false;
        try {
            orz::HipBackend& be = *s->be;
            ORZ_HIP_CHECK(hipSetDevice(be.device()));  // every host thread talks to its worker's device
            MemberArena* ar = arena_of(be.device());
            for (;;) {
                const size_t i = next.fetch_add(1);
                if (i >= nm || rc.load() != ORZ_OK) break;
                if (!s->enc) throw std::runtime_error("a worker has no encoder (a reconfiguration ran out of device memory)");
                const uint8_t* const src = items[i].p;
                const size_t len = items[i].len;
                be.begin_encode();
                const auto r = orz::encode_stream_device(*s->enc, be, src, len, src_on_device != 0, nullptr, 0);
                MemberPlace& pl = place[i];
                pl.len = r.len;
                // a place in the arena is taken only when the member fits it: one that does not leaves the counter as it was,
                // so the smaller members behind it still land there
                size_t at = ar ? ar->used.load() : 0;
                bool fits = false;
                while (ar && r.len <= ar->cap && at <= ar->cap - r.len && !(fits = ar->used.compare_exchange_weak(at, at + r.len))) {}
                if (fits) {
                    pl.device = be.device(); pl.off = at;
                    be.select(3);
                    be.d2d(ar->p + at, r.data, r.len);
                    be.select(0);
                    copied = true;
                } else {
                    if (ar && ar->caller) throw std::runtime_error("the output buffer is too small for the members' streams");
                    pl.host.resize(r.len);
                    ORZ_HIP_CHECK(hipMemcpy(pl.host.data(), r.data, r.len, hipMemcpyDeviceToHost));
                }
                if (verify) {
                    std::vector<uint8_t> h(r.len);
                    ORZ_HIP_CHECK(hipMemcpy(h.data(), r.data, r.len, hipMemcpyDeviceToHost));
                    verify_stream_decode(src, len, src_on_device != 0, h.data(), h.size());
                }
            }
            if (copied) { be.select(3); be.sync(); be.select(0); }  // (the worker's moves into the arena: one wait per job)
        } catch (const std::exception& e) {
            int expect = ORZ_OK;
            const std::string msg = e.what();
            if (rc.compare_exchange_strong(expect, msg.find("output buffer is too small") != std::string::npos ? ORZ_ENOMEM : ORZ_ENODEV)) err = msg;
            if (copied) {  // (a failed job returns the arena too: no move into it may still be under way)
                try { s->be->select(3); s->be->sync(); s->be->select(0); } catch (const std::exception&) {}
            }
        }
    };
    struct Joiner {  // joins whatever was started, also when starting a later thread throws
        std::vector<std::thread> th;
        ~Joiner() { for (auto& t : th) if (t.joinable()) t.join(); }
    } joiner;
    for (size_t i = 1; i < m->workers.size(); i++) joiner.th.emplace_back(work, m->workers[i]);
    work(m->workers[0]);
    for (auto& t : joiner.th) t.join();
    if (rc.load() != ORZ_OK) return fail(rc.load(), err);
    return ORZ_OK;
}
}  // namespace
namespace {
bool one_device(const orz_members* m) {
    const int d0 = m->workers[0]->be->device();
    for (orz_stream* w : m->workers)
        if (w->be->device() != d0) return false;
    return true;
}
// The members of `items` gathered in host memory in item order (*dst: malloc'ed), by way of an arena per device the workers sit on,
// owned by the members object and kept between calls, of `want` bytes at least.  lens (optional): each member's stream length.
int members_encode_host(orz_members* m, const std::vector<MemberItem>& items, int src_on_device, size_t want, uint8_t** dst, size_t* dst_len,
                        size_t* lens) {
    try {
        std::vector<std::unique_ptr<MemberArena>> arenas;
        for (orz_stream* w : m->workers) {
            const int dev = w->be->device();
            bool have = false;
            for (auto& a : arenas) have = have || a->device == dev;
            if (have) continue;
            auto& slot = m->arena[dev];
            if (slot.second < want) {
                ORZ_HIP_CHECK(hipSetDevice(dev));
                if (slot.first) (void)hipFree(slot.first);
                slot = {nullptr, 0};
                void* p = nullptr;
                if (hipMalloc(&p, want) == hipSuccess) slot = {(uint8_t*)p, want};
                else (void)hipGetLastError();  // (no arena on this device: its members go through host memory)
            }
            if (slot.first) {
                std::unique_ptr<MemberArena> a(new MemberArena(dev, slot.first, slot.second, false));
                arenas.push_back(std::move(a));
            }
        }
        std::vector<MemberPlace> place(items.size());
        const int rc = members_run(m, items, src_on_device, arenas, place);
        if (rc != ORZ_OK) return rc;
        // the members in input order: ONE copy each, from where it lies to its place in the result (round 6; before: device ->
        // a vector per member -> the result)
        size_t total = 0;
        for (auto& pl : place) total += pl.len;
        uint8_t* p = (uint8_t*)std::malloc(total ? total : 1);
        if (!p) return fail(ORZ_ENOMEM, "malloc failed");
        size_t at = 0;
        int cur = -1;
        for (auto& pl : place) {
            if (pl.device >= 0) {
                if (cur != pl.device) { (void)hipSetDevice(pl.device); cur = pl.device; }
                uint8_t* base = nullptr;
                for (auto& a : arenas) if (a->device == pl.device) base = a->p;
                const hipError_t ce = hipMemcpy(p + at, base + pl.off, pl.len, hipMemcpyDeviceToHost);
                if (ce != hipSuccess) { std::free(p); return fail(ORZ_ENODEV, hipGetErrorString(ce)); }
            } else {
                std::memcpy(p + at, pl.host.data(), pl.len);
            }
            at += pl.len;
        }
        if (lens)
            for (size_t k = 0; k < place.size(); k++) lens[k] = place[k].len;
        *dst = p;
        *dst_len = total;
        return ORZ_OK;
    } catch (const std::exception& e) {  // (allocation / thread start failures never cross the C boundary)
        return fail(ORZ_ENOMEM, e.what());
    }
}
// The members of `items` left in the caller's device buffer wherever they finish; offs / lens: where each lies.
int members_encode_device(orz_members* m, const std::vector<MemberItem>& items, int src_on_device, uint8_t* d_dst, size_t d_cap, size_t* offs,
                          size_t* lens) {
    try {
        std::vector<std::unique_ptr<MemberArena>> arenas;
        arenas.emplace_back(new MemberArena(m->workers[0]->be->device(), d_dst, d_cap, true));
        std::vector<MemberPlace> place(items.size());
        const int rc = members_run(m, items, src_on_device, arenas, place);
        if (rc != ORZ_OK) return rc;
        for (size_t k = 0; k < place.size(); k++) { offs[k] = place[k].off; lens[k] = place[k].len; }
        return ORZ_OK;
    } catch (const std::exception& e) {
        return fail(ORZ_ENOMEM, e.what());
    }
}
// the caller's segments as work items, or the reason they are refused
const char* segment_items(const orz_members* m, const void* const* seg_src, const size_t* seg_len, size_t n_segs, int src_on_device,
                          std::vector<MemberItem>& items) {
    if (!m) return "null members object";
    if (n_segs && (!seg_src || !seg_len)) return "null segment arrays";
    for (size_t k = 0; k < n_segs; k++)
        if (!seg_src[k] && seg_len[k]) return "a null segment of non-zero length";
    if (src_on_device && n_segs && !one_device(m)) return "device-resident input needs all workers on that device";
    items.resize(n_segs);
    for (size_t k = 0; k < n_segs; k++) items[k] = MemberItem{(const uint8_t*)seg_src[k], seg_len[k]};
    return nullptr;
}
// ORZ_OK when the members of `segs` can go to the caller's device buffer, else ORZ_EINVAL with the reason as the thread's message:
// what the calls with a device-resident output check last, behind their own checks and the answer for no segments
int device_output_check(const orz_members* m, const std::vector<MemberItem>& segs, int src_on_device, const uint8_t* d_dst, size_t d_cap,
                        const size_t* offs, const size_t* lens) {
    if (!d_dst || !offs || !lens) return fail(ORZ_EINVAL, "bad argument");
    if (!one_device(m)) return fail(ORZ_EINVAL, "device-resident output needs all workers on one device");
    if (src_on_device)
        for (size_t k = 0; k < segs.size(); k++)
            if (segs[k].len && d_cap && segs[k].p < d_dst + d_cap && d_dst < segs[k].p + segs[k].len)
                return fail(ORZ_EINVAL, "segment " + std::to_string(k) + " overlaps the output buffer");
    return ORZ_OK;
}
}  // namespace
int orz_members_encode(orz_members* m, const void* src, size_t n, int src_on_device, size_t member_bytes, uint8_t** dst,
                       size_t* dst_len, size_t* n_members_out) {
    if (!m || !dst || !dst_len || (!src && n) || member_bytes == 0) return fail(ORZ_EINVAL, "bad argument");
    if (src_on_device && m->workers.size() > 1 && !one_device(m)) return fail(ORZ_EINVAL, "device-resident input needs all workers on that device");
    try {
        std::vector<MemberItem> items;
        member_cuts(src, n, member_bytes, items);
        const size_t nm = items.size();
        // the arena: sized for ratio 0.5 (text: 0.28) or the streams' bound, whichever is smaller
        const size_t want = std::min(nm * orz::stream_bound(std::min(member_bytes, n ? n : 1)), n / 2 + nm * 65536 + (32u << 20));
        const int rc = members_encode_host(m, items, src_on_device, want, dst, dst_len, nullptr);
        if (rc == ORZ_OK && n_members_out) *n_members_out = nm;
        return rc;
    } catch (const std::exception& e) {
        return fail(ORZ_ENOMEM, e.what());
    }
}
int orz_members_encode_to_device(orz_members* m, const void* src, size_t n, int src_on_device, size_t member_bytes, uint8_t* d_dst,
                                 size_t d_cap, size_t* offs, size_t* lens, size_t* n_members_out) {
    if (!m || !d_dst || !offs || !lens || (!src && n) || member_bytes == 0) return fail(ORZ_EINVAL, "bad argument");
    if (!one_device(m)) return fail(ORZ_EINVAL, "device-resident output needs all workers on one device");
    try {
        std::vector<MemberItem> items;
        member_cuts(src, n, member_bytes, items);
        const int rc = members_encode_device(m, items, src_on_device, d_dst, d_cap, offs, lens);
        if (rc == ORZ_OK && n_members_out) *n_members_out = items.size();
        return rc;
    } catch (const std::exception& e) {
        return fail(ORZ_ENOMEM, e.what());
    }
}
size_t orz_members_bound_segments(const size_t* seg_len, size_t n_segs) {
    size_t total = 0;
    for (size_t k = 0; seg_len && k < n_segs; k++) total += orz::stream_bound(seg_len[k]);
    return total;
}
int orz_members_encode_segments(orz_members* m, const void* const* seg_src, const size_t* seg_len, size_t n_segs, int src_on_device,
                                uint8_t** dst, size_t* dst_len, size_t* lens) {
    if (!dst || !dst_len) return fail(ORZ_EINVAL, "bad argument");
    try {
        std::vector<MemberItem> items;
        if (const char* why = segment_items(m, seg_src, seg_len, n_segs, src_on_device, items)) return fail(ORZ_EINVAL, why);
        if (!n_segs) return give_bytes({}, dst, dst_len);  // no members, no bytes, nothing launched
        size_t in_total = 0;
        for (const MemberItem& it : items) in_total += it.len;
        const size_t want = std::min(orz_members_bound_segments(seg_len, n_segs), in_total / 2 + n_segs * 65536 + (32u << 20));
        return members_encode_host(m, items, src_on_device, want, dst, dst_len, lens);
    } catch (const std::exception& e) {
        return fail(ORZ_ENOMEM, e.what());
    }
}
int orz_members_encode_segments_to_device(orz_members* m, const void* const* seg_src, const size_t* seg_len, size_t n_segs,
                                          int src_on_device, uint8_t* d_dst, size_t d_cap, size_t* offs, size_t* lens) {
    try {
        std::vector<MemberItem> items;
        if (const char* why = segment_items(m, seg_src, seg_len, n_segs, src_on_device, items)) return fail(ORZ_EINVAL, why);
        if (!n_segs) return ORZ_OK;
        if (const int rc = device_output_check(m, items, src_on_device, d_dst, d_cap, offs, lens)) return rc;
        return members_encode_device(m, items, src_on_device, d_dst, d_cap, offs, lens);
    } catch (const std::exception& e) {
        return fail(ORZ_ENOMEM, e.what());
    }
}
// ---- tensors as byte planes (orz_planes.h): the planes of every segment staged in ONE device buffer by ONE PlaneSplit launch,
// then the segment call's path over the planes as device-resident items
size_t orz_members_bound_planes(const size_t* seg_len, const uint32_t* seg_elem, size_t n_segs) {
    size_t total = 0;
    for (size_t k = 0; seg_len && seg_elem && k < n_segs; k++)
        if (seg_elem[k]) total += (size_t)seg_elem[k] * orz::stream_bound(seg_len[k] / seg_elem[k]);
    return total;
}
namespace {
// pieces to a plane of `count` elements at a piece size of `piece_elems` (0: never cut)
size_t plane_pieces(size_t count, size_t piece_elems) { return piece_elems && piece_elems < count ? (count + piece_elems - 1) / piece_elems : 1; }

// orz_members_encode_planes_pieces_to_device; pieces_out == nullptr and piece_elems == 0: orz_members_encode_planes_to_device;
// seg_base not null: orz_members_encode_deltas_to_device -- seg_base[k] = segment k's base, resident where the sources are, or
// nullptr for none.  A segment that has a base and bytes is a row of the split whatever its element size, its base one more
// column of the table's ONE upload, and the ONE launch is PlaneSplitDelta; with no base anywhere the call is the pieces call.
int encode_planes_pieces(orz_members* m, const void* const* seg_src, const size_t* seg_len, const uint32_t* seg_elem, size_t n_segs,
                         size_t piece_elems, int src_on_device, uint8_t* d_dst, size_t d_cap, size_t* offs, size_t* lens, size_t* pieces_out,
                         const void* const* seg_base = nullptr) {
    struct Staging {  // the call's one device buffer: the descriptor table, then the planes (and the uploads of host segments)
        void* p = nullptr;
        ~Staging() { if (p) (void)hipFree(p); }
    } staging;
    try {
        std::vector<MemberItem> segs;
        if (const char* why = segment_items(m, seg_src, seg_len, n_segs, src_on_device, segs)) return fail(ORZ_EINVAL, why);
        if (n_segs && !seg_elem) return fail(ORZ_EINVAL, "null element sizes");
        if (piece_elems % orz::kPlaneUnit)
            return fail(ORZ_EINVAL, "pieces of " + std::to_string(piece_elems) + " elements are no multiple of " + std::to_string(orz::kPlaneUnit));
        for (size_t k = 0; k < n_segs; k++) {
            if (!orz::plane_elem_ok(seg_elem[k]))
                return fail(ORZ_EINVAL, "segment " + std::to_string(k) + " has elements of " + std::to_string(seg_elem[k]) + " bytes (1, 2, 4 or 8)");
            if (segs[k].len % seg_elem[k])
                return fail(ORZ_EINVAL, "the " + std::to_string(segs[k].len) + " bytes of segment " + std::to_string(k) + " are no multiple of its element size " +
                                            std::to_string(seg_elem[k]));
        }
        if (!n_segs) return ORZ_OK;
        if (const int rc = device_output_check(m, segs, src_on_device, d_dst, d_cap, offs, lens)) return rc;
        // the staging buffer's layout: table [| base column] | per segment, at multiples of 256: [its upload] [its base's upload] [its planes]
        const auto base_of = [&](size_t k) { return seg_base && segs[k].len ? (const uint8_t*)seg_base[k] : nullptr; };
        size_t n_rows = 0, n_items = 0;
        bool deltas = false;
        for (size_t k = 0; k < n_segs; k++) {
            const size_t Q = plane_pieces(segs[k].len / seg_elem[k], piece_elems);
            n_rows += seg_elem[k] > 1 || base_of(k);
            deltas = deltas || base_of(k);
            n_items += seg_elem[k] * Q;
            if (pieces_out) pieces_out[k] = Q;
        }
        const auto up256 = [](size_t x) { return (x + 255) / 256 * 256; };
        const size_t bases_at = orz::plane_table_bytes(n_rows);  // (a multiple of 8)
        size_t at = up256(bases_at + (deltas ? n_rows * 8 : 0));
        std::vector<size_t> raw_at(n_segs, 0), base_at(n_segs, 0), planes_at(n_segs, 0);
        for (size_t k = 0; k < n_segs; k++) {
            if (!src_on_device && segs[k].len) { raw_at[k] = at; at = up256(at + segs[k].len); }
            if (!src_on_device && base_of(k)) { base_at[k] = at; at = up256(at + segs[k].len); }
            if ((seg_elem[k] > 1 || base_of(k)) && segs[k].len) { planes_at[k] = at; at = up256(at + (size_t)seg_elem[k] * orz::plane_pitch(segs[k].len / seg_elem[k])); }
        }
        const bool need = n_rows || !src_on_device;
        orz::HipBackend& be = *m->workers[0]->be;
        uint8_t* stage = nullptr;
        if (need) {
            ORZ_HIP_CHECK(hipSetDevice(be.device()));
            if (hipMalloc(&staging.p, at) != hipSuccess) {
                (void)hipGetLastError();
                staging.p = nullptr;
                return fail(ORZ_ENOMEM, "no device memory for " + std::to_string(at) + " bytes of plane staging");
            }
            stage = (uint8_t*)staging.p;
        }
        std::vector<MemberItem> items;
        items.reserve(n_items);
        std::vector<orz::PlaneRow> rows;
        rows.reserve(n_rows);
        std::vector<uint64_t> row_base;  // the rows' bases
        row_base.reserve(n_rows);
        for (size_t k = 0; k < n_segs; k++) {
            const uint32_t e = seg_elem[k];
            const size_t count = segs[k].len / e;
            const uint8_t* d_seg = segs[k].p;
            const uint8_t* d_base = base_of(k);
            if (!src_on_device && segs[k].len) {
                be.h2d(stage + raw_at[k], segs[k].p, segs[k].len);
                d_seg = stage + raw_at[k];
            }
            if (!src_on_device && d_base) {
                be.h2d(stage + base_at[k], d_base, segs[k].len);
                d_base = stage + base_at[k];
            }
            // plane p's pieces: its bytes [q P, min(count, (q + 1) P)), an item each (P a multiple of 16: each starts as aligned as the plane)
            const size_t Q = plane_pieces(count, piece_elems), P = Q > 1 ? piece_elems : count;
            const auto cut = [&](const uint8_t* plane) {
                for (size_t q = 0; q < Q; q++) items.push_back(MemberItem{count ? plane + q * P : nullptr, std::min(P, count - q * P)});
            };
            if (e == 1 && !d_base) {
                cut(d_seg);
                continue;
            }
            const size_t pitch = orz::plane_pitch(count);
            for (uint32_t p = 0; p < e; p++) cut(stage + planes_at[k] + p * pitch);
            rows.push_back(orz::PlaneRow{(uint64_t)(uintptr_t)d_seg, (uint64_t)(uintptr_t)(stage + planes_at[k]), count, e});
            row_base.push_back((uint64_t)(uintptr_t)d_base);
        }
        if (!rows.empty()) {
            std::vector<uint64_t> image;
            uint64_t units = 0;
            const orz::PlaneTable t = orz::plane_table_image(rows, stage, image, units);
            if (deltas) image.insert(image.end(), row_base.begin(), row_base.end());  // (image ends at bases_at)
            if (units) {
                be.h2d(stage, image.data(), image.size() * 8);
                if (deltas) be.launch((size_t)units, orz::PlaneSplitDelta{t, (const uint64_t*)(stage + bases_at), units});
                else be.launch((size_t)units, orz::PlaneSplit{t, units});
                be.sync();  // (the workers read the planes on streams of their own)
            }
        }
        return members_encode_device(m, items, 1, d_dst, d_cap, offs, lens);
    } catch (const std::bad_alloc& e) {
        return fail(ORZ_ENOMEM, e.what());
    } catch (const std::exception& e) {
        return fail(ORZ_ENODEV, e.what());
    }
}
}  // namespace
int orz_members_encode_planes_to_device(orz_members* m, const void* const* seg_src, const size_t* seg_len, const uint32_t* seg_elem,
                                        size_t n_segs, int src_on_device, uint8_t* d_dst, size_t d_cap, size_t* offs, size_t* lens) {
    return encode_planes_pieces(m, seg_src, seg_len, seg_elem, n_segs, 0, src_on_device, d_dst, d_cap, offs, lens, nullptr);
}
size_t orz_members_bound_planes_pieces(const size_t* seg_len, const uint32_t* seg_elem, size_t n_segs, size_t piece_elems, size_t* n_members_out) {
    size_t total = 0, members = 0;
    for (size_t k = 0; seg_len && seg_elem && k < n_segs; k++) {
        if (!seg_elem[k]) continue;
        const size_t count = seg_len[k] / seg_elem[k], Q = plane_pieces(count, piece_elems);
        const size_t last = Q > 1 ? count - (Q - 1) * piece_elems : count;
        total += (size_t)seg_elem[k] * ((Q - 1) * orz::stream_bound(Q > 1 ? piece_elems : 0) + orz::stream_bound(last));
        members += (size_t)seg_elem[k] * Q;
    }
    if (n_members_out) *n_members_out = members;
    return total;
}
int orz_members_encode_planes_pieces_to_device(orz_members* m, const void* const* seg_src, const size_t* seg_len, const uint32_t* seg_elem,
                                               size_t n_segs, size_t piece_elems, int src_on_device, uint8_t* d_dst, size_t d_cap, size_t* offs,
                                               size_t* lens, size_t* pieces_out) {
    if (n_segs && !pieces_out) return fail(ORZ_EINVAL, "bad argument");
    return encode_planes_pieces(m, seg_src, seg_len, seg_elem, n_segs, piece_elems, src_on_device, d_dst, d_cap, offs, lens, pieces_out);
}
int orz_members_encode_deltas_to_device(orz_members* m, const void* const* seg_src, const void* const* seg_base, const size_t* seg_len,
                                        const uint32_t* seg_elem, size_t n_segs, size_t piece_elems, int src_on_device, uint8_t* d_dst,
                                        size_t d_cap, size_t* offs, size_t* lens, size_t* pieces_out) {
    if (n_segs && (!pieces_out || !seg_base)) return fail(ORZ_EINVAL, "bad argument");
    static const void* const none = nullptr;  // (no segments: still "with bases")
    return encode_planes_pieces(m, seg_src, seg_len, seg_elem, n_segs, piece_elems, src_on_device, d_dst, d_cap, offs, lens, pieces_out,
                                seg_base ? seg_base : &none);
}
int orz_decode_members_mem(const uint8_t* src, size_t n, uint8_t** dst, size_t* dst_len, size_t* n_members_out) {
    if ((!src && n) || !dst || !dst_len) return fail(ORZ_EINVAL, "bad argument");
    try {
        std::vector<uint8_t> out;
        size_t at = 0, members = 0;
        orz::host::DecodeWorkspace ws;  // one window / model allocation for all members
        while (at < n) {
            orz::host::decode_stream(
                ws,
                [&](uint8_t* buf, size_t k) {
                    if (at + k > n) return false;
                    std::memcpy(buf, src + at, k);
                    at += k;
                    return true;
                },
                [&](const uint8_t* buf, size_t k) { out.insert(out.end(), buf, buf + k); }, [](bool, size_t, size_t) {});
            members++;
        }
        if (const int rc = give_bytes(out, dst, dst_len)) return rc;
        if (n_members_out) *n_members_out = members;
        return ORZ_OK;
    } catch (const std::exception& e) {
        return fail(ORZ_EINVAL, e.what());
    }
}

int orz_decode_members_device(int device, const uint8_t* src, size_t n, uint8_t** dst, size_t* dst_len,
                              size_t* n_members_out, orz_decode_stats* stats) {
    if ((!src && n) || !dst || !dst_len) return fail(ORZ_EINVAL, "bad argument");
    if (!device_ok(device)) return fail(ORZ_ENODEV, "no such HIP device");
    try {
        orz::HipBackend be(device);
        std::vector<uint8_t> out;
        orz::DecodeStats st;
        orz::decode_members_device(be, src, n, out, st, decode_slots());
        if (const int rc = give_bytes(out, dst, dst_len)) return rc;
        if (n_members_out) *n_members_out = (size_t)st.members;
        put_stats(stats, st);
        return ORZ_OK;
    } catch (const std::exception& e) {
        return fail(ORZ_EINVAL, e.what());
    }
}

int orz_decode_members_to_device(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens,
                                 size_t n_members, uint8_t* d_dst, size_t d_cap, size_t* dst_len, size_t* n_members_out,
                                 size_t* out_offs, orz_decode_stats* stats) {
    if ((!src && n) || !dst_len || (!d_dst && d_cap) || (!offs != !lens))
        return fail(ORZ_EINVAL, "bad argument");
    if (!device_ok(device)) return fail(ORZ_ENODEV, "no such HIP device");
    static_assert(sizeof(size_t) == sizeof(uint64_t), "the member table is handed to the device as 64-bit words");
    uint64_t total = 0, members = 0;
    const auto sizes_out = [&] {
        *dst_len = (size_t)total;
        if (n_members_out) *n_members_out = (size_t)members;
    };
    return mapped([&] {
        orz::HipBackend be(device);
        orz::DecodeToDeviceStats st;
        try {
            orz::decode_members_to_device(be, (const uint8_t*)src, n, src_on_device != 0, offs != nullptr, (const uint64_t*)offs,
                                          (const uint64_t*)lens, n_members, d_dst, d_cap, total, members, (uint64_t*)out_offs, st,
                                          decode_slots());
        } catch (const orz::DecodeCapacityError&) {  // (the size is known: reported as the sizing call reports it)
            sizes_out();
            throw;
        }
        sizes_out();
        put_stats(stats, st);
    });
}

thread_local uint64_t g_scatter_waits = 0;
int orz_decode_members_scatter(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens,
                               size_t n_members, uint8_t* const* d_dsts, const size_t* d_caps, size_t n_dsts, size_t* out_lens,
                               size_t* n_members_out, orz_decode_stats* stats) {
    const bool bad = (!src && n) || (!offs != !lens) || (d_dsts && n_dsts && !d_caps);
    return decode_into_list(g_scatter_waits, bad, device, n_members_out, stats, [&](orz::HipBackend& be, uint64_t& members, orz::DecodeScatterStats& st) {
        orz::decode_members_scatter(be, (const uint8_t*)src, n, src_on_device != 0, offs != nullptr, (const uint64_t*)offs,
                                    (const uint64_t*)lens, n_members, d_dsts, (const uint64_t*)d_caps, n_dsts, (uint64_t*)out_lens, members, st,
                                    decode_slots());
    });
}
uint64_t orz_decode_members_scatter_host_waits(void) { return g_scatter_waits; }

thread_local uint64_t g_planes_waits = 0;
int orz_decode_members_planes(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens,
                              size_t n_members, uint8_t* const* d_dsts, const size_t* d_caps, const uint32_t* elems, size_t n_dsts,
                              size_t* out_lens, size_t* n_members_out, orz_decode_stats* stats) {
    const bool bad = (!src && n) || (!offs != !lens) || (d_dsts && n_dsts && !d_caps) || (n_dsts && !elems);
    return decode_into_list(g_planes_waits, bad, device, n_members_out, stats, [&](orz::HipBackend& be, uint64_t& members, orz::DecodeScatterStats& st) {
        orz::decode_members_planes(be, (const uint8_t*)src, n, src_on_device != 0, offs != nullptr, (const uint64_t*)offs, (const uint64_t*)lens,
                                   n_members, d_dsts, (const uint64_t*)d_caps, elems, n_dsts, (uint64_t*)out_lens, members, st, decode_slots());
    });
}
uint64_t orz_decode_members_planes_host_waits(void) { return g_planes_waits; }

thread_local uint64_t g_pieces_waits = 0;
int orz_decode_members_planes_pieces(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens,
                                     size_t n_members, uint8_t* const* d_dsts, const size_t* d_caps, const uint32_t* elems,
                                     const uint32_t* pieces, size_t n_dsts, size_t* out_lens, size_t* n_members_out, orz_decode_stats* stats) {
    const bool bad = (!src && n) || (!offs != !lens) || (d_dsts && n_dsts && !d_caps) || (n_dsts && (!elems || !pieces));
    static const uint32_t none = 0;  // (no destinations: still "with pieces")
    return decode_into_list(g_pieces_waits, bad, device, n_members_out, stats, [&](orz::HipBackend& be, uint64_t& members, orz::DecodeScatterStats& st) {
        orz::decode_members_planes(be, (const uint8_t*)src, n, src_on_device != 0, offs != nullptr, (const uint64_t*)offs, (const uint64_t*)lens,
                                   n_members, d_dsts, (const uint64_t*)d_caps, elems, n_dsts, (uint64_t*)out_lens, members, st, decode_slots(),
                                   pieces ? pieces : &none);
    });
}
uint64_t orz_decode_members_planes_pieces_host_waits(void) { return g_pieces_waits; }

// ------------------------------------------------------------------------------ CRC-32 digests (orz_crc.h)
// The kernels' tables on `device`: computed and uploaded once per device and process, never freed.  (A copy of its own, not one of
// a backend's stream: it is no host wait of the call that happens to be the first.)
static const uint32_t* crc_device_image(int device) {
    static std::mutex m;
    static std::map<int, uint32_t*> images;
    std::lock_guard<std::mutex> lk(m);
    auto it = images.find(device);
    if (it != images.end()) return it->second;
    ORZ_HIP_CHECK(hipSetDevice(device));
    uint32_t* d = nullptr;
    ORZ_HIP_CHECK(hipMalloc((void**)&d, orz::kCrcImageWords * 4));
    const hipError_t e = hipMemcpy(d, orz::crc_host_image(), orz::kCrcImageWords * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e) + " at the upload of the CRC tables");
    }
    images[device] = d;
    return d;
}

int orz_crc32_buffers(int device, const void* const* bufs, const size_t* lens, size_t n, int on_device, uint32_t* crcs) {
    if (!n) return ORZ_OK;
    if (!bufs || !lens || !crcs) return fail(ORZ_EINVAL, "bad argument");
    for (size_t j = 0; j < n; j++)
        if (!bufs[j] && lens[j]) return fail(ORZ_EINVAL, "buffer " + std::to_string(j) + " is NULL and has bytes");
    if (!on_device) {
        for (size_t j = 0; j < n; j++) crcs[j] = orz::crc32_host((const uint8_t*)bufs[j], lens[j]);
        return ORZ_OK;
    }
    if (!device_ok(device)) return fail(ORZ_ENODEV, "no such HIP device");
    return mapped([&] {
        orz::HipBackend be(device);
        std::vector<uint64_t> addrs(n);
        for (size_t j = 0; j < n; j++) addrs[j] = (uint64_t)(uintptr_t)bufs[j];
        uint64_t waits = 0;
        orz::crc32_device_buffers(be, crc_device_image(device), addrs.data(), (const uint64_t*)lens, n, crcs, waits);
    });
}
uint32_t orz_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return orz::crc32_combine(crc_a, crc_b, len_b); }

thread_local uint64_t g_verified_waits = 0;
int orz_decode_tensors_verified(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens, size_t n_members,
                                uint8_t* const* d_dsts, const size_t* d_caps, const uint32_t* elems, const uint32_t* pieces, size_t n_dsts,
                                const uint32_t* crcs, size_t* out_lens, uint32_t* out_crcs, size_t* n_members_out, orz_decode_stats* stats) {
    const bool bad = (!src && n) || (!offs != !lens) || (d_dsts && n_dsts && (!d_caps || !crcs));
    return decode_into_list(g_verified_waits, bad, device, n_members_out, stats, [&](orz::HipBackend& be, uint64_t& members, orz::DecodeScatterStats& st) {
        const std::vector<uint32_t> ones(elems ? 0 : n_dsts + 1, 1);  // (no element sizes: bytes, the scatter layout)
        const orz::CrcCheck check{d_dsts ? crc_device_image(device) : nullptr, crcs, out_crcs};
        orz::decode_members_planes(be, (const uint8_t*)src, n, src_on_device != 0, offs != nullptr, (const uint64_t*)offs, (const uint64_t*)lens,
                                   n_members, d_dsts, (const uint64_t*)d_caps, elems ? elems : ones.data(), n_dsts, (uint64_t*)out_lens, members, st,
                                   decode_slots(), pieces, &check);
    });
}
uint64_t orz_decode_tensors_verified_host_waits(void) { return g_verified_waits; }

thread_local uint64_t g_delta_waits = 0;
int orz_decode_tensors_delta(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens, size_t n_members,
                             uint8_t* const* d_dsts, const size_t* d_caps, const void* const* d_bases, const uint32_t* elems, const uint32_t* pieces,
                             size_t n_dsts, const uint32_t* crcs, size_t* out_lens, uint32_t* out_crcs, size_t* n_members_out, orz_decode_stats* stats) {
    static_assert(sizeof(void*) == sizeof(uint64_t), "the bases are handed to the device as 64-bit words");
    const bool bad = (!src && n) || (!offs != !lens) || (d_dsts && n_dsts && !d_caps) || (n_dsts && !d_bases);
    static const uint64_t none = 0;  // (no destinations: still "with bases")
    return decode_into_list(g_delta_waits, bad, device, n_members_out, stats, [&](orz::HipBackend& be, uint64_t& members, orz::DecodeScatterStats& st) {
        const std::vector<uint32_t> ones(elems ? 0 : n_dsts + 1, 1);  // (no element sizes: bytes, a member per destination)
        const orz::CrcCheck check{d_dsts && crcs ? crc_device_image(device) : nullptr, crcs, out_crcs};
        orz::decode_members_planes(be, (const uint8_t*)src, n, src_on_device != 0, offs != nullptr, (const uint64_t*)offs, (const uint64_t*)lens,
                                   n_members, d_dsts, (const uint64_t*)d_caps, elems ? elems : ones.data(), n_dsts, (uint64_t*)out_lens, members, st,
                                   decode_slots(), pieces, crcs ? &check : nullptr, d_bases ? (const uint64_t*)d_bases : &none);
    });
}
uint64_t orz_decode_tensors_delta_host_waits(void) { return g_delta_waits; }

thread_local uint64_t g_chain_waits = 0;
int orz_decode_tensors_chain(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens, size_t n_members,
                             uint8_t* const* d_dsts, const size_t* d_caps, const void* const* d_bases, const uint32_t* elems, const uint32_t* pieces,
                             size_t n_dsts, const uint32_t* crcs, uint32_t links, size_t* out_lens, uint32_t* out_crcs, size_t* n_members_out,
                             orz_decode_stats* stats) {
    const bool bad = (!src && n) || (!offs != !lens) || (d_dsts && n_dsts && !d_caps);
    if (!bad && !links) {
        g_chain_waits = 0;
        return fail(ORZ_EINVAL, "invalid argument: a chain of 0 links");
    }
    return decode_into_list(g_chain_waits, bad, device, n_members_out, stats, [&](orz::HipBackend& be, uint64_t& members, orz::DecodeScatterStats& st) {
        const std::vector<uint32_t> ones(elems ? 0 : n_dsts + 1, 1);  // (no element sizes: bytes, a member per destination and link)
        const orz::CrcCheck check{d_dsts && crcs ? crc_device_image(device) : nullptr, crcs, out_crcs};
        orz::decode_members_chain(be, (const uint8_t*)src, n, src_on_device != 0, offs != nullptr, (const uint64_t*)offs, (const uint64_t*)lens,
                                  n_members, d_dsts, (const uint64_t*)d_caps, elems ? elems : ones.data(), n_dsts, (uint64_t*)out_lens, members, st,
                                  decode_slots(), pieces, crcs ? &check : nullptr, (const uint64_t*)d_bases, links);
    });
}
uint64_t orz_decode_tensors_chain_host_waits(void) { return g_chain_waits; }

// `reps` PlaneMergeChain launches over ONE tensor whose `links` plane sets lie elem x plane_pitch(count) bytes apart from d_planes
int orz_plane_chain_move_time(int device, void* d_inter, const void* d_base, const void* d_planes, size_t count, uint32_t elem, uint32_t links,
                              int reps, double* ms) {
    if (!d_inter || !d_planes || !count || !links || !ms || reps < 1 || !orz::plane_elem_ok(elem)) return fail(ORZ_EINVAL, "bad argument");
    if (!device_ok(device)) return fail(ORZ_ENODEV, "no such HIP device");
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    try {
        orz::HipBackend be(device);
        orz::DeviceBuffers<orz::HipBackend> own(be);
        // first | inter | pitch | count | base | plane0[links] | elem (u32)
        const uint64_t pitch = orz::plane_pitch(count), units = orz::plane_units(count);
        std::vector<uint64_t> image(5 + (size_t)links + 1, 0);
        image[1] = (uint64_t)(uintptr_t)d_inter;
        image[2] = pitch;
        image[3] = count;
        image[4] = (uint64_t)(uintptr_t)d_base;
        for (uint32_t k = 0; k < links; k++) image[5 + k] = (uint64_t)(uintptr_t)d_planes + (uint64_t)k * elem * pitch;
        *(uint32_t*)(image.data() + 5 + links) = elem;
        uint64_t* d = own.alloc<uint64_t>(image.size(), false);
        be.h2d(d, image.data(), image.size() * 8);
        const orz::PlaneTable t{d, d + 1, d + 5, d + 2, d + 3, (const uint32_t*)(d + 5 + links), 1};
        ORZ_HIP_CHECK(hipEventCreate(&ev.a));
        ORZ_HIP_CHECK(hipEventCreate(&ev.b));
        for (int r = -1; r < reps; r++) {  // (the first launch warms up)
            if (r == 0) ORZ_HIP_CHECK(hipEventRecord(ev.a, be.stream()));
            be.launch((size_t)units, orz::PlaneMergeChain{t, d + 4, units, links});
        }
        ORZ_HIP_CHECK(hipEventRecord(ev.b, be.stream()));
        ORZ_HIP_CHECK(hipEventSynchronize(ev.b));
        float total = 0;
        ORZ_HIP_CHECK(hipEventElapsedTime(&total, ev.a, ev.b));
        *ms = (double)total / reps;
        return ORZ_OK;
    } catch (const std::exception& e) {
        return fail(ORZ_ENODEV, e.what());
    }
}
namespace {
int plane_move_time(int device, void* d_inter, const void* d_base, void* d_planes, size_t count, uint32_t elem, int merge, int reps, double* ms);
}
int orz_plane_move_time(int device, void* d_inter, void* d_planes, size_t count, uint32_t elem, int merge, int reps, double* ms) {
    if (!d_inter || !d_planes || !count || !ms || reps < 1 || (elem != 2 && elem != 4 && elem != 8)) return fail(ORZ_EINVAL, "bad argument");
    return plane_move_time(device, d_inter, nullptr, d_planes, count, elem, merge, reps, ms);
}
int orz_plane_delta_move_time(int device, void* d_inter, const void* d_base, void* d_planes, size_t count, uint32_t elem, int merge, int reps,
                              double* ms) {
    if (!d_inter || !d_base || !d_planes || !count || !ms || reps < 1 || !orz::plane_elem_ok(elem)) return fail(ORZ_EINVAL, "bad argument");
    return plane_move_time(device, d_inter, d_base, d_planes, count, elem, merge, reps, ms);
}
namespace {
// d_base == nullptr: the plain kernels; else the delta kernels with that base
int plane_move_time(int device, void* d_inter, const void* d_base, void* d_planes, size_t count, uint32_t elem, int merge, int reps, double* ms) {
    if (!device_ok(device)) return fail(ORZ_ENODEV, "no such HIP device");
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    try {
        orz::HipBackend be(device);
        orz::DeviceBuffers<orz::HipBackend> own(be);
        std::vector<orz::PlaneRow> rows{orz::PlaneRow{(uint64_t)(uintptr_t)d_inter, (uint64_t)(uintptr_t)d_planes, count, elem}};
        uint8_t* d_table = own.alloc<uint8_t>(orz::plane_table_bytes(1) + 8, false);  // (the table, then the base column)
        std::vector<uint64_t> image;
        uint64_t units = 0;
        const orz::PlaneTable t = orz::plane_table_image(rows, d_table, image, units);
        image.push_back((uint64_t)(uintptr_t)d_base);
        const uint64_t* d_bases = (const uint64_t*)(d_table + orz::plane_table_bytes(1));
        be.h2d(d_table, image.data(), image.size() * 8);
        ORZ_HIP_CHECK(hipEventCreate(&ev.a));
        ORZ_HIP_CHECK(hipEventCreate(&ev.b));
        for (int r = -1; r < reps; r++) {  // (the first launch warms up)
            if (r == 0) ORZ_HIP_CHECK(hipEventRecord(ev.a, be.stream()));
            if (d_base && merge) be.launch((size_t)units, orz::PlaneMergeDelta{t, d_bases, units});
            else if (d_base) be.launch((size_t)units, orz::PlaneSplitDelta{t, d_bases, units});
            else if (merge) be.launch((size_t)units, orz::PlaneMerge{t, units});
            else be.launch((size_t)units, orz::PlaneSplit{t, units});
        }
        ORZ_HIP_CHECK(hipEventRecord(ev.b, be.stream()));
        ORZ_HIP_CHECK(hipEventSynchronize(ev.b));
        float total = 0;
        ORZ_HIP_CHECK(hipEventElapsedTime(&total, ev.a, ev.b));
        *ms = (double)total / reps;
        return ORZ_OK;
    } catch (const std::exception& e) {
        return fail(ORZ_ENODEV, e.what());
    }
}
}  // namespace

// ONE whole-tensor element read's gather alone, timed: `count` elements (a multiple of 16) of `elem` bytes whose planes lie `count`
// bytes apart from d_planes, merged to d_dst; d_base == nullptr: ElementGather, else ElementGatherDelta with that base
int orz_element_gather_time(int device, const void* d_planes, const void* d_base, void* d_dst, size_t count, uint32_t elem, int reps, double* ms) {
    if (!d_planes || !d_dst || !count || count % orz::kPlaneUnit || !ms || reps < 1 || !orz::plane_elem_ok(elem)) return fail(ORZ_EINVAL, "bad argument");
    if (!device_ok(device)) return fail(ORZ_ENODEV, "no such HIP device");
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    try {
        orz::HipBackend be(device);
        orz::DeviceBuffers<orz::HipBackend> own(be);
        // ufirst | first | count | member | dst_off | bslice | place[elem] | elem, status[elem] (u32)
        const uint64_t units = orz::ElementGather::units_of(0, count);
        std::vector<uint64_t> image(6 + elem + 1 + (elem + 1) / 2, 0);
        image[2] = count;
        image[5] = (uint64_t)(uintptr_t)d_base;
        for (uint32_t p = 0; p < elem; p++) image[6 + p] = (uint64_t)p * count;
        uint32_t* tail = (uint32_t*)(image.data() + 6 + elem);
        tail[0] = elem;
        for (uint32_t p = 0; p < elem; p++) tail[2 + p] = orz::kDecOk;
        uint64_t* d = own.alloc<uint64_t>(image.size(), false);
        be.h2d(d, image.data(), image.size() * 8);
        const uint32_t* d_tail = (const uint32_t*)(d + 6 + elem);
        const orz::ElementGather g{d, d + 1, d + 2, d + 3, d + 4, d_tail, 1, units, d + 6, d_tail + 2, (const uint8_t*)d_planes, (uint8_t*)d_dst};
        ORZ_HIP_CHECK(hipEventCreate(&ev.a));
        ORZ_HIP_CHECK(hipEventCreate(&ev.b));
        for (int r = -1; r < reps; r++) {  // (the first launch warms up)
            if (r == 0) ORZ_HIP_CHECK(hipEventRecord(ev.a, be.stream()));
            if (d_base) be.launch((size_t)units, orz::ElementGatherDelta{g, d + 5});
            else be.launch((size_t)units, g);
        }
        ORZ_HIP_CHECK(hipEventRecord(ev.b, be.stream()));
        ORZ_HIP_CHECK(hipEventSynchronize(ev.b));
        float total = 0;
        ORZ_HIP_CHECK(hipEventElapsedTime(&total, ev.a, ev.b));
        *ms = (double)total / reps;
        return ORZ_OK;
    } catch (const std::exception& e) {
        return fail(ORZ_ENODEV, e.what());
    }
}

// ------------------------------------------------------------------------------ byte ranges of a container
struct orz_reader {
    std::unique_ptr<orz::HipBackend> be;
    std::unique_ptr<orz::RangeReader<orz::HipBackend>> rd;  // (declared after the backend: destroyed before it)
    std::unique_ptr<orz::ElementReader<orz::HipBackend>> el;  // (borrows rd: destroyed before it)
};

orz_reader* orz_reader_open(int device, const void* src, size_t n, int src_on_device, const size_t* offs, const size_t* lens,
                            size_t n_members) {
    if ((!src && n) || (!offs != !lens)) { fail(ORZ_EINVAL, "bad argument"); return nullptr; }
    if (!device_ok(device)) { fail(ORZ_ENODEV, "no such HIP device"); return nullptr; }
    std::unique_ptr<orz_reader> r;
    const int rc = mapped([&] {
        r.reset(new orz_reader);
        r->be.reset(new orz::HipBackend(device));
        r->rd.reset(new orz::RangeReader<orz::HipBackend>(*r->be, (const uint8_t*)src, n, src_on_device != 0, offs != nullptr,
                                                          (const uint64_t*)offs, (const uint64_t*)lens, n_members));
        r->el.reset(new orz::ElementReader<orz::HipBackend>(*r->rd));
    });
    return rc == ORZ_OK ? r.release() : nullptr;
}

void orz_reader_close(orz_reader* r) { delete r; }

int orz_reader_info(orz_reader* r, uint64_t* members, uint64_t* total, uint64_t* member_offs, size_t cap) {
    if (!r) return fail(ORZ_EINVAL, "bad argument");
    try {
        if (members) *members = r->rd->ix.members;
        if (total) *total = r->rd->ix.total;
        if (member_offs && cap) {
            const std::vector<uint64_t>& o = r->rd->member_offsets();
            std::copy(o.begin(), o.begin() + std::min(cap, o.size()), member_offs);
        }
        return ORZ_OK;
    } catch (const std::exception& e) {
        return fail(ORZ_EINVAL, e.what());
    }
}

namespace {
void put_read_stats(orz_read_stats* stats, const orz::RangeReadStats& st) {
    if (!stats) return;
    stats->ranges = st.ranges; stats->members_decoded = st.members_decoded; stats->decoded_bytes = st.decoded_bytes;
    stats->out_bytes = st.out_bytes; stats->launches = st.launches; stats->host_waits = st.host_waits;
    stats->kernel_ms = st.kernel_ms; stats->gather_ms = st.gather_ms; stats->total_s = st.total_s;
}
}  // namespace

int orz_reader_read(orz_reader* r, const uint64_t* off, const uint64_t* len, size_t n_ranges, uint8_t* d_dst, size_t d_cap,
                    uint64_t* dst_len, orz_read_stats* stats) {
    if (!r || !dst_len) return fail(ORZ_EINVAL, "bad argument");
    orz::RangeReadStats st;
    uint64_t total = 0;
    const int rc = mapped([&] { r->rd->read(off, len, n_ranges, d_dst, d_cap, total, st, decode_slots()); });
    *dst_len = total;
    put_read_stats(stats, st);
    return rc;
}

int orz_reader_set_planes(orz_reader* r, const uint32_t* elems, size_t n_tensors) {
    if (!r) return fail(ORZ_EINVAL, "bad argument");
    return mapped([&] { r->el->set_planes(elems, n_tensors); });
}

int orz_reader_set_planes_pieces(orz_reader* r, const uint32_t* elems, const uint32_t* pieces, size_t n_tensors) {
    if (!r || (n_tensors && !pieces)) return fail(ORZ_EINVAL, "bad argument");
    return mapped([&] { r->el->set_planes(elems, n_tensors, pieces); });
}

int orz_reader_set_bases(orz_reader* r, const void* const* bases, size_t n_tensors) {
    static_assert(sizeof(void*) == sizeof(uint64_t), "the bases are handed to the device as 64-bit words");
    if (!r) return fail(ORZ_EINVAL, "bad argument");
    return mapped([&] { r->el->set_bases((const uint64_t*)bases, n_tensors); });
}

int orz_reader_tensor_info(orz_reader* r, uint64_t* n_tensors, uint64_t* counts, uint32_t* elems, size_t cap) {
    if (!r) return fail(ORZ_EINVAL, "bad argument");
    const orz::ElementReader<orz::HipBackend>& el = *r->el;
    if (n_tensors) *n_tensors = el.elems.size();
    const size_t k = std::min(cap, el.elems.size());
    if (counts) std::copy(el.counts.begin(), el.counts.begin() + k, counts);
    if (elems) std::copy(el.elems.begin(), el.elems.begin() + k, elems);
    return ORZ_OK;
}

int orz_reader_read_elements(orz_reader* r, const uint64_t* tensor, const uint64_t* first, const uint64_t* count, size_t n_ranges,
                             uint8_t* d_dst, size_t d_cap, uint64_t* dst_len, orz_read_stats* stats) {
    if (!r || !dst_len) return fail(ORZ_EINVAL, "bad argument");
    orz::RangeReadStats st;
    uint64_t total = 0;
    const int rc = mapped([&] { r->el->read(tensor, first, count, n_ranges, d_dst, d_cap, total, st, decode_slots()); });
    *dst_len = total;
    put_read_stats(stats, st);
    return rc;
}

int orz_reader_set_cache(orz_reader* r, uint64_t max_bytes) {
    if (!r) return fail(ORZ_EINVAL, "bad argument");
    return mapped([&] { r->rd->set_cache(max_bytes); });
}

uint64_t orz_reader_cursor_state_bytes(void) { return orz::RangeReader<orz::HipBackend>::cursor_state_bytes(); }

int orz_reader_cache_stats(orz_reader* r, orz_cache_stats* stats) {
    if (!r || !stats) return fail(ORZ_EINVAL, "bad argument");
    const orz::RangeCacheStats c = r->rd->cache_stats();
    stats->hits = c.hits; stats->resumed = c.resumed; stats->fresh = c.fresh; stats->uncached = c.uncached; stats->evicted = c.evicted;
    stats->cursors = c.cursors; stats->bytes = c.bytes; stats->budget = c.budget;
    return ORZ_OK;
}

// ------------------------------------------------------------------------------ Huffman tables alone
size_t orz_huffman_stride(void) { return orz::kHwStride; }
int orz_huffman_tables(int device, const uint32_t* weights, size_t nchunks, uint8_t* lens, uint16_t* codes, double* elapsed_us) {
    if (!weights || !lens || !codes || nchunks > (1u << 20)) return fail(ORZ_EINVAL, "bad argument");
    if (device < 0 || device >= orz_device_count()) return fail(ORZ_ENODEV, "no such HIP device");
    const size_t n = nchunks * orz::kHwStride;
    for (size_t i = 0; i < n; i++)
        if (weights[i] > orz::HuffBuild::kMaxWeight) return fail(ORZ_EINVAL, "symbol weight of 2^23 or more");
    if (!n) return ORZ_OK;
    try {
        orz::HipBackend be(device);
        struct Bufs {
            orz::HipBackend& be;
            uint32_t* w = nullptr; uint8_t* l = nullptr; uint16_t* c = nullptr;
            ~Bufs() { be.free(w); be.free(l); be.free(c); }
        } b{be};
        b.w = be.alloc<uint32_t>(n, false);
        b.l = be.alloc<uint8_t>(n);
        b.c = be.alloc<uint16_t>(n);
        be.h2d(b.w, weights, n * 4);
        const orz::HuffBuild f{b.w, (uint32_t)nchunks, b.l, b.c};
        be.huffbuild(f);  // (warm: code object load)
        struct Events {  // destroyed on every path out
            hipEvent_t a = nullptr, b = nullptr;
            ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
        } ev;
        ORZ_HIP_CHECK(hipEventCreate(&ev.a));
        ORZ_HIP_CHECK(hipEventCreate(&ev.b));
        ORZ_HIP_CHECK(hipEventRecord(ev.a, be.stream()));
        be.huffbuild(f);
        ORZ_HIP_CHECK(hipEventRecord(ev.b, be.stream()));
        be.d2h(lens, b.l, n);
        be.d2h(codes, b.c, n * 2);
        float ms = 0;
        ORZ_HIP_CHECK(hipEventElapsedTime(&ms, ev.a, ev.b));
        if (elapsed_us) *elapsed_us = (double)ms * 1000.0;
        return ORZ_OK;
    } catch (const std::exception& e) {
        return fail(ORZ_EINVAL, e.what());
    }
}

// ------------------------------------------------------------------------------ the fast parse's step machinery alone
int orz_fast_step_path(int device, unsigned form, uint32_t n, uint32_t tile, uint32_t t_lo, uint32_t t_hi, uint32_t entry,
                       const uint8_t* wbytes, const uint32_t* ev, uint8_t* ty, uint8_t* nl, uint8_t* x0, uint8_t* x1, uint8_t* x2,
                       uint32_t* centry, uint32_t* tentry, uint64_t* sbits, uint8_t* pt, uint32_t* cm, uint64_t* lds_bytes) {
    const int bad = mapped([&] { orz::fast_step_path_check(form, n, tile, t_lo, t_hi, entry, wbytes, ev, ty, nl, x0, x1, x2, centry, tentry, sbits, pt, cm); });
    if (bad) return bad;
    if (!device_ok(device)) return fail(ORZ_ENODEV, "no such HIP device");
    return mapped([&] {
        orz::HipBackend be(device);
        orz::fast_step_path(be, form, n, tile, t_lo, t_hi, entry, wbytes, ev, ty, nl, x0, x1, x2, centry, tentry, sbits, pt, cm, lds_bytes);
    });
}
int orz_fast_step_counts(int device, uint32_t n, const uint8_t* wbytes, const uint64_t* sbits, int count, uint32_t s0, uint32_t s1,
                         uint32_t ext, uint32_t cpt, uint32_t live_end, uint32_t rows, uint32_t* cm, uint32_t* cp, uint32_t* cp2,
                         uint32_t* ord, uint32_t* ord2, uint32_t* acc2) {
    const int bad = mapped([&] { orz::fast_step_counts_check(n, wbytes, sbits, s0, s1, ext, cpt, live_end, rows, cm, cp, cp2, ord, ord2, acc2); });
    if (bad) return bad;
    if (!device_ok(device)) return fail(ORZ_ENODEV, "no such HIP device");
    return mapped([&] {
        orz::HipBackend be(device);
        orz::fast_step_counts(be, n, wbytes, sbits, count, s0, s1, ext, cpt, live_end, rows, cm, cp, cp2, ord, ord2, acc2);
    });
}
int orz_fast_step_horizon(int device, const uint32_t* cp, uint32_t rows, const uint32_t* hpre, uint32_t s0, uint32_t s1, uint32_t* hz,
                          uint32_t* hz2) {
    const int bad = mapped([&] { orz::fast_step_horizon_check(cp, rows, hpre, s0, s1, hz, hz2); });
    if (bad) return bad;
    if (!device_ok(device)) return fail(ORZ_ENODEV, "no such HIP device");
    return mapped([&] {
        orz::HipBackend be(device);
        orz::fast_step_horizon(be, cp, rows, hpre, s0, s1, hz, hz2);
    });
}

// ------------------------------------------------------------------------------ symbol ranking alone
int orz_symrank_chains(int device, uint16_t* tables, const uint32_t* gsym, const uint32_t* rstart, size_t nitems,
                       uint16_t* ranks, uint32_t* flags2, double* elapsed_us) {
    if (!tables || !rstart || (!gsym && nitems) || (!ranks && nitems)) return fail(ORZ_EINVAL, "bad argument");
    if (device < 0 || device >= orz_device_count()) return fail(ORZ_ENODEV, "no such HIP device");
    if (const char* why = orz::symrank_chains_invalid(tables, gsym, rstart, nitems)) return fail(ORZ_EINVAL, why);
    try {
        orz::HipBackend be(device);
        const size_t nt = (size_t)512 * orz::kSrWords;
        struct Bufs {
            orz::HipBackend& be;
            uint16_t *st = nullptr, *backup = nullptr, *rk = nullptr;
            uint32_t *gs = nullptr, *rs = nullptr, *fl = nullptr;
            ~Bufs() { be.free(st); be.free(backup); be.free(rk); be.free(gs); be.free(rs); be.free(fl); }
        } b{be};
        b.st = be.alloc<uint16_t>(nt, false);
        b.backup = be.alloc<uint16_t>(nt, false);
        b.rk = be.alloc<uint16_t>(nitems, false);
        b.gs = be.alloc<uint32_t>(nitems, false);
        b.rs = be.alloc<uint32_t>(513, false);
        b.fl = be.alloc<uint32_t>(3);
        be.h2d(b.st, tables, nt * 2);
        be.h2d(b.gs, gsym, nitems * 4);
        be.h2d(b.rs, rstart, 513 * 4);
        struct Events {  // destroyed on every path out
            hipEvent_t a = nullptr, b = nullptr;
            ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
        } ev;
        ORZ_HIP_CHECK(hipEventCreate(&ev.a));
        ORZ_HIP_CHECK(hipEventCreate(&ev.b));
        ORZ_HIP_CHECK(hipEventRecord(ev.a, be.stream()));
        // the encoder's own sequence: backup, kernel, SymCheck, the guarded rerun (ORZ_SYMRANK_INJECT acts here as in an encode)
        be.symrank(b.st, b.gs, b.rk, b.rs, (uint32_t)nitems, b.fl, b.backup, nullptr);
        ORZ_HIP_CHECK(hipEventRecord(ev.b, be.stream()));
        uint32_t fl[3] = {0, 0, 0};
        be.d2h(fl, b.fl, sizeof fl);
        be.d2h(tables, b.st, nt * 2);
        if (nitems) be.d2h(ranks, b.rk, nitems * 2);
        if (flags2) { flags2[0] = fl[0]; flags2[1] = fl[1]; }
        float ms = 0;
        ORZ_HIP_CHECK(hipEventElapsedTime(&ms, ev.a, ev.b));
        if (elapsed_us) *elapsed_us = (double)ms * 1000.0;
        return ORZ_OK;
    } catch (const std::exception& e) {
        return fail(ORZ_EINVAL, e.what());
    }
}

// ------------------------------------------------------------------------------ orz_lz_encoder
orz_lz_encoder* orz_lz_encoder_new(int device) {
    try {
        if (device < 0 || device >= orz_device_count()) { fail(ORZ_ENODEV, "no such HIP device"); return nullptr; }
        std::unique_ptr<orz_lz_encoder> e(new orz_lz_encoder);
        e->be.reset(new orz::HipBackend(device));
        e->be->enable_arena();
        e->seg = env_u("ORZ_SEG", kDefaultSeg);
        e->win = env_u("ORZ_WIN", 0);
        return e.release();
    } catch (const std::exception& ex) {
        fail(ORZ_ENODEV, ex.what());
        return nullptr;
    }
}
void orz_lz_encoder_free(orz_lz_encoder* e) {
    if (!e) return;
    e->enc.reset();
    e->be.reset();
    delete e;
}

int orz_lz_encoder_encode(orz_lz_encoder* e, const orz_lzcfg* cfg, const uint8_t* sbuf, size_t sbuf_len, uint8_t* tbuf,
                          size_t tbuf_cap, size_t spos, size_t* spos_out, size_t* tlen_out) {
    if (!e || !sbuf || !tbuf || !spos_out || !tlen_out || !cfg_ok(cfg)) return fail(ORZ_EINVAL, "bad argument");
    if (sbuf_len > orz::kBlock || spos > sbuf_len || spos < orz::kPre) return fail(ORZ_EINVAL, "bad window geometry");
    try {
        const bool same_cfg = e->enc && std::memcmp(&e->cfg, cfg, sizeof *cfg) == 0;
        if (!e->enc) {
            e->cfg = *cfg;
            const bool fast = mode_from_env();
            e->enc.reset(new Enc(*e->be, to_cfg(cfg), e->seg, fast ? 64 : window_for(*e->be, *cfg, e->win), fast,
                                 env_u("ORZ_FAST_TILE", orz::kFastTile), env_u("ORZ_FAST_ROUNDS", orz::kFastRounds)));
        } else if (!same_cfg) {
            return fail(ORZ_EINVAL, "LZCfg changed inside a stream");
        }
        const bool continuing = e->next_chunk < e->chunk_end_spos.size() && spos == e->expect_spos;
        if (!continuing) {
            if (spos != orz::kPre) return fail(ORZ_EINVAL, "a block must start at SBVEC_PREMATCH_LEN");
            // upload the caller's window exactly as it is, sentinel pads included (src/lib.rs:67-69) -- except, after a
            // forward(), the pad in FRONT of the window: the caller's copy_within (src/lib.rs:83) leaves the sentinel's zeros
            // there, but the context of the item start at window offset 1 (hash1 of offset 0, src/lz.rs:482-486) looks at the
            // byte before the window, and this encoder rebuilds its tables from the window's bytes -- slide(false) kept the
            // two real bytes on the device, and the upload must not wipe them (round 3's slide defect, at this seam)
            if (e->slid) e->be->h2d(e->enc->dwin(), sbuf, (size_t)sbuf_len + orz::kSent);
            else e->be->h2d(e->enc->dwinbuf(), sbuf - orz::kSent, (size_t)sbuf_len + 2 * orz::kSent);
            e->framed.clear();
            e->chunk_end_spos.clear();
            e->enc->encode_block((uint32_t)(sbuf_len - orz::kPre), e->framed, &e->chunk_end_spos);
            e->framed_pos = 0;
            e->next_chunk = 0;
        }
        // un-frame the next chunk: LEB128(t) chunk[t]
        size_t t = 0, shift = 0, at = e->framed_pos;
        for (;;) {
            uint8_t b = e->framed[at++];
            t |= (size_t)(b & 0x7f) << shift;
            shift += 7;
            if (!(b & 0x80)) break;
        }
        if (t > tbuf_cap) return fail(ORZ_ENOMEM, "tbuf too small");
        std::memcpy(tbuf, e->framed.data() + at, t);
        e->framed_pos = at + t;
        *tlen_out = t;
        *spos_out = e->chunk_end_spos[e->next_chunk++];
        e->expect_spos = *spos_out;
        return ORZ_OK;
    } catch (const std::exception& ex) {
        return fail(ORZ_ENODEV, ex.what());
    }
}

int orz_lz_encoder_forward(orz_lz_encoder* e, size_t forward_len) {
    if (!e || !e->enc) return fail(ORZ_EINVAL, "forward before encode");
    if (forward_len != orz::kNewMax) return fail(ORZ_EINVAL, "forward_len must be 2^24");
    try {
        e->enc->slide(false);  // the caller re-supplies the slid window on the next encode()
        e->slid = true;
        e->chunk_end_spos.clear();
        e->next_chunk = 0;
        return ORZ_OK;
    } catch (const std::exception& ex) {
        return fail(ORZ_ENODEV, ex.what());
    }
}

// ------------------------------------------------------------------------------ decode (host)
struct orz_lz_decoder {
    orz::host::Decoder dec;
};
orz_lz_decoder* orz_lz_decoder_new(void) {
    try {
        return new orz_lz_decoder();
    } catch (const std::exception& e) {
        fail(ORZ_ENOMEM, e.what());
        return nullptr;
    }
}
void orz_lz_decoder_free(orz_lz_decoder* d) { delete d; }
int orz_lz_decoder_decode(orz_lz_decoder* d, const uint8_t* tbuf, size_t tlen, uint8_t* sbuf, size_t spos,
                          size_t* spos_end_out) {
    if (!d || !tbuf || !sbuf || !spos_end_out || spos < 3) return fail(ORZ_EINVAL, "bad argument");
    try {
        *spos_end_out = d->dec.decode(tbuf, tlen, sbuf, spos);
        return ORZ_OK;
    } catch (const std::exception& e) {
        return fail(ORZ_EINVAL, e.what());
    }
}
int orz_lz_decoder_forward(orz_lz_decoder* d, size_t forward_len) {
    if (!d) return fail(ORZ_EINVAL, "null decoder");
    d->dec.forward(forward_len);
    return ORZ_OK;
}
int orz_decode(orz_read_fn rd, void* rctx, orz_write_fn wr, void* wctx, orz_progress_fn prog, void* pctx) {
    if (!rd || !wr) return fail(ORZ_EINVAL, "bad argument");
    int io = ORZ_OK;
    try {
        orz::host::decode_stream(
            [&](uint8_t* buf, size_t n) {
                size_t got = 0;
                while (got < n) {
                    ssize_t r = rd(rctx, buf + got, n - got);
                    if (r < 0) { io = ORZ_EIO; return false; }
                    if (r == 0) return false;
                    got += (size_t)r;
                }
                return true;
            },
            [&](const uint8_t* buf, size_t n) {
                if (n && wr(wctx, buf, n) != 0) { io = ORZ_EIO; throw std::runtime_error("write failed"); }
            },
            [&](bool fin, size_t a, size_t b) {
                if (prog) prog(pctx, fin ? 1 : 0, a, b);
            });
        return ORZ_OK;
    } catch (const std::exception& e) {
        return fail(io != ORZ_OK ? io : ORZ_EINVAL, e.what());
    }
}
int orz_decode_mem(const uint8_t* src, size_t n, uint8_t** dst, size_t* dst_len, size_t* consumed) {
    if ((!src && n) || !dst || !dst_len) return fail(ORZ_EINVAL, "bad argument");
    try {
        std::vector<uint8_t> out;
        size_t at = 0;
        orz::host::decode_stream(
            [&](uint8_t* buf, size_t k) {
                if (at + k > n) return false;
                std::memcpy(buf, src + at, k);
                at += k;
                return true;
            },
            [&](const uint8_t* buf, size_t k) { out.insert(out.end(), buf, buf + k); }, [](bool, size_t, size_t) {});
        uint8_t* p = (uint8_t*)std::malloc(out.size() ? out.size() : 1);
        if (!p) return fail(ORZ_ENOMEM, "malloc failed");
        std::memcpy(p, out.data(), out.size());
        *dst = p;
        *dst_len = out.size();
        if (consumed) *consumed = at;
        return ORZ_OK;
    } catch (const std::exception& e) {
        return fail(ORZ_EINVAL, e.what());
    }
}

// ------------------------------------------------------------------------------ orz::encode
int orz_encode(orz_read_fn rd, void* rctx, orz_write_fn wr, void* wctx, const orz_lzcfg* cfg, orz_progress_fn prog,
               void* pctx, int device) {
    if (!rd || !wr || !cfg_ok(cfg)) return fail(ORZ_EINVAL, "bad argument");
    orz_stream* s = orz_stream_new(device, cfg);
    if (!s) return ORZ_ENODEV;
    int rc = ORZ_OK;
    try {
        Enc& enc = *s->enc;
        orz::HipBackend& be = *s->be;
        enc.reset();
        struct PinnedBuf {  // the block read buffer, page-locked (pinned hipMemcpyAsync feed)
            uint8_t* p = nullptr;
            PinnedBuf() { if (hipHostMalloc((void**)&p, orz::kNewMax, hipHostMallocDefault) != hipSuccess) { p = nullptr; throw std::runtime_error("hipHostMalloc failed"); } }
            ~PinnedBuf() { if (p) (void)hipHostFree(p); }
            uint8_t* data() { return p; }
            size_t size() const { return orz::kNewMax; }
        } in;
        std::vector<uint8_t> out;
        size_t in_total = 0, out_total = 0;
        bool first = true;
        std::unique_ptr<orz::host::DecodeCheck> chk(verify_decode_on() ? new orz::host::DecodeCheck : nullptr);  // (verifies a block's bytes before the sink sees them)
        for (;;) {
            // read_repeatedly, src/lib.rs:42-52: fill the block or hit EOF
            size_t got = 0;
            while (got < in.size()) {
                ssize_t r = rd(rctx, in.data() + got, in.size() - got);
                if (r < 0) { rc = fail(ORZ_EIO, "read failed"); break; }
                if (r == 0) break;
                got += (size_t)r;
            }
            if (rc != ORZ_OK || got == 0) break;
            if (!first) enc.slide();
            first = false;
            be.h2d_pinned(enc.dwin() + orz::kPre, in.data(), got);  // encode_block syncs before `in` is refilled
            if (chk) chk->feed_input(in.data(), got);
            out.clear();
            enc.encode_block_units((uint32_t)got, in_total == 0 && got == in.size(), out);
            if (chk && !out.empty()) chk->feed_output(out.data(), out.size());
            if (!out.empty() && wr(wctx, out.data(), out.size()) != 0) { rc = fail(ORZ_EIO, "write failed"); break; }
            in_total += got;
            out_total += out.size();
            if (prog) prog(pctx, 0, in_total, out_total);
            if (got < in.size()) break;
        }
        if (rc == ORZ_OK) {  // the last block's tail stage is still in flight: take its bytes
            out.clear();
            enc.finish(out);
            if (chk) {
                const uint8_t z = 0;
                if (!out.empty()) chk->feed_output(out.data(), out.size());
                chk->feed_output(&z, 1);
                chk->finish();
            }
            if (!out.empty() && wr(wctx, out.data(), out.size()) != 0) rc = fail(ORZ_EIO, "write failed");
            out_total += out.size();
        }
        if (rc == ORZ_OK) {
            const uint8_t eof = 0;  // write_len(0), src/lib.rs:89
            if (wr(wctx, &eof, 1) != 0) rc = fail(ORZ_EIO, "write failed");
            out_total += 1;
            if (prog) prog(pctx, 1, in_total, out_total);
        }
    } catch (const std::exception& ex) {
        rc = fail(ORZ_ENODEV, ex.what());
    }
    orz_stream_free(s);
    return rc;
}

}  // extern "C"
