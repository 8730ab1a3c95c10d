// emu_fast_step.cpp -- the stand-alone entry points of the fast parse's step machinery (orz_fast_step.h) on the emulation
// backend (TEST INFRASTRUCTURE ONLY): the same host lines and kernel bodies as orz_fast_step_path / _counts / _horizon of the
// library.  0, -12 (std::bad_alloc) or -22 (anything else) with the message in err.
#include "emu_backend.cpp"
#include "../../orz_amd/csrc/orz_fast_step.h"

template <class F>
static int step_mapped(F&& f, char* err, size_t errcap) {
    try {
        f();
        return 0;
    } catch (const std::bad_alloc& e) {
        put_err(e, err, errcap);
        return -12;
    } catch (const std::exception& e) {
        put_err(e, err, errcap);
        return -22;
    }
}

extern "C" int emu_fast_step_path(unsigned form, uint32_t n, uint32_t tile, uint32_t t_lo, uint32_t t_hi, uint32_t entry, const uint8_t* wbytes,
                                  const uint32_t* ev, uint8_t* ty, uint8_t* nl, uint8_t* x0, uint8_t* x1, uint8_t* x2, uint32_t* centry,
                                  uint32_t* tentry, uint64_t* sbits, uint8_t* pt, uint32_t* cm, uint64_t* lds_bytes, char* err, size_t errcap) {
    return step_mapped([&] {
        EmuBackend be;
        be.order = 2;  // (the blocks of a launch in a shuffled order: no kernel of the stage may depend on it)
        orz::fast_step_path(be, form, n, tile, t_lo, t_hi, entry, wbytes, ev, ty, nl, x0, x1, x2, centry, tentry, sbits, pt, cm, lds_bytes);
    }, err, errcap);
}

extern "C" int emu_fast_step_counts(uint32_t n, const uint8_t* wbytes, const uint64_t* sbits, int count, uint32_t s0, uint32_t s1, uint32_t ext,
                                    uint32_t cpt, uint32_t live_end, uint32_t rows, uint32_t* cm, uint32_t* cp, uint32_t* cp2, uint32_t* ord,
                                    uint32_t* ord2, uint32_t* acc2, char* err, size_t errcap) {
    return step_mapped([&] {
        EmuBackend be;
        be.order = 2;
        orz::fast_step_counts(be, n, wbytes, sbits, count, s0, s1, ext, cpt, live_end, rows, cm, cp, cp2, ord, ord2, acc2);
    }, err, errcap);
}

extern "C" int emu_fast_step_horizon(const uint32_t* cp, uint32_t rows, const uint32_t* hpre, uint32_t s0, uint32_t s1, uint32_t* hz, uint32_t* hz2,
                                     char* err, size_t errcap) {
    return step_mapped([&] {
        EmuBackend be;
        orz::fast_step_horizon(be, cp, rows, hpre, s0, s1, hz, hz2);
    }, err, errcap);
}
