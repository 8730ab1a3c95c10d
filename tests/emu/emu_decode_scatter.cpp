// emu_decode_scatter.cpp -- ScatterPlan / ScatterVerdict and decode_members_scatter (orz_decode_scatter.h) on the emulation
// backend (TEST INFRASTRUCTURE ONLY).  "Device memory" is host memory here: the caller's buffers are handed over as they are.
#include "emu_backend.cpp"
#include "../../orz_amd/csrc/orz_decode_scatter.h"

// the two plan launches alone, over arrays the caller made up: out_off / verdict (members entries) and rec3 = members, first bad
// member, its verdict
extern "C" void emu_scatter_plan(const uint64_t* dsts, const uint64_t* caps, const uint32_t* out_len, uint64_t members, uint64_t base,
                                 uint64_t* out_off, uint32_t* verdict, uint32_t* sizes, uint64_t* rec3) {
    EmuBackend be;
    orz::ScatterRecord rec{~0ull, ~0ull, ~0u, 0};
    be.launch(members, orz::ScatterPlan{dsts, caps, out_len, base, out_off, verdict, sizes, members});
    be.launch_waves(1, orz::ScatterVerdict{verdict, members, &rec}, orz::ScatterVerdict::lds_bytes());
    rec3[0] = rec.members; rec3[1] = rec.bad; rec3[2] = rec.status;
}

// decode_members_scatter: 0, -12 (DecodeCapacityError) or -22 (anything else) with the message in err.  dsts == nullptr sizes.
// stats3 = launches, host waits, members.
extern "C" int emu_decode_scatter(const uint8_t* src, size_t n, int src_on_device, const uint64_t* offs, const uint64_t* lens, size_t n_table,
                                  uint8_t* const* dsts, const uint64_t* caps, size_t n_dsts, unsigned slots, uint64_t* out_lens,
                                  uint64_t* members, uint64_t* stats3, char* err, size_t errcap) {
    uint64_t m = 0;
    int rc = 0;
    orz::DecodeScatterStats st;
    try {
        EmuBackend be;
        orz::decode_members_scatter(be, src, n, src_on_device != 0, offs != nullptr, offs, lens, n_table, dsts, caps, n_dsts, out_lens, m, st,
                                    slots ? slots : 2048);
    } catch (const orz::DecodeCapacityError& e) {
        put_err(e, err, errcap);
        rc = -12;
    } catch (const std::exception& e) {
        put_err(e, err, errcap);
        rc = -22;
    }
    *members = m;
    if (stats3) { stats3[0] = st.launches; stats3[1] = st.host_waits; stats3[2] = st.members; }
    return rc;
}
