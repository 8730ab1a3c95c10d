// freeparse_main.cpp -- the device decoder's kernel body and its drivers on the emulation backend as a STAND-ALONE program, so
// that it can be built with -fsanitize=address,undefined and run on its own (TEST INFRASTRUCTURE ONLY; tests/
// test_freeparse_decoders.py builds and runs it).  For every NAME.orz of the directory given: the member decode, the range reads
// of NAME.ranges (one "offset length" a line, one read each, first without and then with the cursor cache) and the scatter decode
// into buffers with guard bands.  A stream may be refused by all three alike; what is decoded must be the same bytes each way and
// equal NAME.want where that file exists.  Exit status 0: every file went through; 2: a mismatch; a sanitizer report ends the run
// by itself.
#include <dirent.h>

#include <cstdio>
#include <fstream>
#include <sstream>

#include "emu_reader_cache.cpp"
#include "../../orz_amd/csrc/orz_decode_scatter.h"

namespace {
bool slurp(const std::string& path, std::vector<uint8_t>& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

int fail(const std::string& name, const char* what) {
    std::fprintf(stderr, "%s: %s\n", name.c_str(), what);
    return 2;
}

int one(const std::string& dir, const std::string& name) {
    std::vector<uint8_t> src, want, whole;
    if (!slurp(dir + "/" + name + ".orz", src)) return fail(name, "cannot read");
    const bool have_want = slurp(dir + "/" + name + ".want", want);
    // the member decode
    bool ok = true;
    try {
        EmuBackend be;
        orz::DecodeStats st;
        orz::decode_members_device(be, src.data(), src.size(), whole, st, 2);
    } catch (const std::exception& e) {
        ok = false;
        std::printf("%s: refused: %s\n", name.c_str(), e.what());
    }
    if (ok && have_want && whole != want) return fail(name, "the member decode differs from the data");
    if (!ok && have_want) return fail(name, "a stream with known data was refused");
    // the range reads
    std::vector<std::pair<uint64_t, uint64_t>> ranges;
    {
        std::ifstream f(dir + "/" + name + ".ranges");
        uint64_t o, n;
        while (f >> o >> n) ranges.push_back({o, n});
    }
    std::vector<uint64_t> member_offs;
    for (int cached = 0; cached < 2; cached++) {
        try {
            EmuBackend be;
            orz::RangeReader<EmuBackend> rd(be, src.data(), src.size(), true, false, nullptr, nullptr, 0);
            if (!ok) {  // the framing held: the payload must be refused by a read of everything
                std::vector<uint8_t> dst(rd.ix.total + 1);
                uint64_t o = 0, n = rd.ix.total, total = 0;
                orz::RangeReadStats st;
                try {
                    rd.read(&o, &n, 1, dst.data(), dst.size(), total, st, 2);
                } catch (const std::exception&) {
                    continue;
                }
                return fail(name, "the member decode refused what the reader decoded");
            }
            if (rd.ix.total != whole.size()) return fail(name, "the reader's total differs");
            member_offs = rd.member_offsets();
            if (cached) rd.set_cache((uint64_t)1 << 32);
            for (auto& r : ranges) {
                std::vector<uint8_t> dst(r.second + 16, 0xA5);
                uint64_t total = 0;
                orz::RangeReadStats st;
                rd.read(&r.first, &r.second, 1, dst.data(), r.second, total, st, 3);
                if (total != r.second || std::memcmp(dst.data(), whole.data() + r.first, r.second) != 0) return fail(name, "a range read differs");
                for (size_t k = r.second; k < dst.size(); k++)
                    if (dst[k] != 0xA5) return fail(name, "a range read wrote behind its bytes");
            }
        } catch (const std::exception& e) {
            if (ok) return fail(name, e.what());
        }
    }
    // the scatter decode: every member between guard bands
    if (ok) {
        const size_t guard = 64, M = member_offs.size();
        std::vector<uint64_t> caps(M), sizes(M);
        std::vector<uint8_t*> dsts(M);
        std::vector<uint8_t> arena(whole.size() + (M + 1) * guard, 0xA5);
        for (size_t k = 0; k < M; k++) {
            caps[k] = (k + 1 < M ? member_offs[k + 1] : whole.size()) - member_offs[k];
            dsts[k] = arena.data() + member_offs[k] + (k + 1) * guard;
        }
        try {
            EmuBackend be;
            uint64_t m = 0;
            orz::DecodeScatterStats st;
            orz::decode_members_scatter(be, src.data(), src.size(), true, false, nullptr, nullptr, 0, dsts.data(), caps.data(), M, sizes.data(), m, st, 3);
        } catch (const std::exception& e) {
            return fail(name, e.what());
        }
        std::vector<uint8_t> expect(arena.size(), 0xA5);
        for (size_t k = 0; k < M; k++) std::memcpy(expect.data() + member_offs[k] + (k + 1) * guard, whole.data() + member_offs[k], caps[k]);
        if (arena != expect) return fail(name, "the scatter decode wrote outside a member, or other bytes");
    }
    std::printf("%s: %s\n", name.c_str(), ok ? "decoded three ways" : "refused three ways");
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 64;
    std::vector<std::string> names;
    if (DIR* d = opendir(argv[1])) {
        while (dirent* e = readdir(d)) {
            const std::string f = e->d_name;
            if (f.size() > 4 && f.substr(f.size() - 4) == ".orz") names.push_back(f.substr(0, f.size() - 4));
        }
        closedir(d);
    }
    std::sort(names.begin(), names.end());
    if (names.empty()) return 65;
    for (const std::string& n : names)
        if (int rc = one(argv[1], n)) return rc;
    return 0;
}
