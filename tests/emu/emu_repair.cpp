// emu_repair.cpp -- orz_stream_arm_repair_probe / orz_stream_repair_probe on the emulation backend (TEST INFRASTRUCTURE ONLY): the
// same host lines (StreamEncoder::fast_parse with its probe hooks) and kernel bodies as the library.
#include "emu_backend.cpp"

static orz::FastRepairProbe g_emu_probe;
// (an encoder is kept from call to call while the settings stay the same, as a caller of the library would keep its own; an
// encode that fails drops it)
struct EmuRepairKept {
    std::string key;
    std::unique_ptr<EmuBackend> be;
    std::unique_ptr<orz::StreamEncoder<EmuBackend>> enc;
};
static EmuRepairKept g_emu_repair_kept;

// `src` as one stream through a fresh fast-mode encoder (tile / rounds: 0 = the defaults) whose `block`-th encode_block call is
// probed (block < 0: unarmed); ty / nl (nfield bytes each, or null): the decision field to inject.  Returns 0 and the stream,
// -22 when the field breaks its contract, -1 for any other failure (message in err; the kept encoder is dropped).  items / cap / nitems (optional): the stream's
// item trace, as emu_encode_fast_trace returns it.
extern "C" int emu_repair_encode(const uint8_t* src, size_t n, int depth, int lazy1, int lazy2, unsigned tile, unsigned rounds, int block,
                                 const uint8_t* ty, const uint8_t* nl, size_t nfield, uint8_t** dst, size_t* dst_len, EmuItem* items, size_t cap,
                                 size_t* nitems, char* err, size_t errcap) {
    try {
        g_emu_probe = orz::FastRepairProbe();
        if (block >= 0 && (ty || nl || nfield)) {
            if (const char* why = orz::FastRepairProbe::field_invalid(ty, nl, nfield)) {
                put_err(std::invalid_argument(why), err, errcap);
                return -22;
            }
            g_emu_probe.inj_ty.assign(ty, ty + nfield);
            g_emu_probe.inj_nl.assign(nl, nl + nfield);
        }
        g_emu_probe.arm = block < 0 ? -1 : block;
        EmuRepairKept& kept = g_emu_repair_kept;
        const char* unit = std::getenv("ORZ_FAST_UNIT");
        const std::string key = std::to_string(depth) + "," + std::to_string(lazy1) + "," + std::to_string(lazy2) + "," + std::to_string(tile) + "," +
                                std::to_string(rounds) + "," + (unit ? unit : "");
        if (!kept.enc || kept.key != key) {
            kept.enc.reset();
            kept.be.reset(new EmuBackend);
            orz::Cfg cfg{depth, lazy1, lazy2};
            kept.enc.reset(new orz::StreamEncoder<EmuBackend>(*kept.be, cfg, 62, 64, true, tile ? tile : orz::kFastTile, rounds ? rounds : orz::kFastRounds));
            kept.key = key;
        }
        EmuBackend& be = *kept.be;
        orz::StreamEncoder<EmuBackend>& enc = *kept.enc;
        struct Clear {
            orz::StreamEncoder<EmuBackend>& e;
            ~Clear() { e.trace = nullptr; e.repair_probe = nullptr; }
        } clear{enc};
        enc.repair_probe = &g_emu_probe;
        orz::ItemTrace tr;
        if (items) enc.trace = &tr;
        std::vector<uint8_t> out;
        orz::encode_stream(enc, be, src, n, false, out);
        if (items) {
            const size_t k = tr.pos.size() < cap ? tr.pos.size() : cap;
            for (size_t i = 0; i < k; i++)
                items[i] = EmuItem{tr.block[i], tr.pos[i], tr.src[i], tr.sym[i], tr.rank[i], tr.ctx[i], tr.mlen[i], tr.al[i], tr.unl[i], tr.enc[i]};
            *nitems = tr.pos.size();
        }
        *dst = (uint8_t*)std::malloc(out.size() ? out.size() : 1);
        std::memcpy(*dst, out.data(), out.size());
        *dst_len = out.size();
        return 0;
    } catch (const std::invalid_argument& e) {  // (a field of another size than the armed block's: refused before the block is parsed)
        put_err(e, err, errcap);
        return -22;
    } catch (const std::exception& e) {
        g_emu_repair_kept.enc.reset();
        put_err(e, err, errcap);
        return -1;
    }
}
extern "C" long emu_repair_table(const char* name, void* dst, size_t cap) {
    if (!name || !g_emu_probe.taken) return -22;
    const std::vector<uint8_t>* t = g_emu_probe.find(name);
    if (!t) return -22;
    if (dst && cap) std::memcpy(dst, t->data(), std::min(cap, t->size()));
    return (long)t->size();
}
