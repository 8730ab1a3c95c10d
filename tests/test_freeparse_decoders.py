"""Every decoder of the project held to legal streams that no encoder writes (tests/_freeparse.py): random parses, random code
lengths up to 15 bits, declared maxima above the actual ones, chunks down to one item, items that overrun their chunk's end field
inside the member and past the member's announced end.  The oracle's decoder (the restatement of the reference's) must turn
every generated stream into its data and consume all of it -- that is what makes a stream legal; if it does not, the WRITER is
wrong and the fixture raises.  Then the host decoder, the device decoder's kernel body on the emulation, the two framing indexes,
the range reader with and without cursors and the scatter driver must all return the same bytes."""
import ctypes
import os
import subprocess

import pytest

import _cachecases as cc
import _freeparse as fp
import _rangecases as rc
import _scattercases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUITES = fp.SUITES


@pytest.fixture(scope="module")
def suites(oracle):
    out = fp.load_cases()
    assert sorted(out) == sorted(SUITES)
    for cases in out.values():
        for c in cases:  # (no generated stream is left out: one the oracle does not follow fails every test of this file)
            oracle.assert_decodes_to(c.stream, c.data, "free-parse stream " + c.name)
    return out


@pytest.fixture(scope="module")
def mixed(suites, oracle):
    return fp.container(suites, oracle)


def _emu_decode_members(emu, blob, slots):
    lib = emu.lib
    dst = ctypes.POINTER(ctypes.c_uint8)()
    n, m = ctypes.c_size_t(), ctypes.c_size_t()
    err = ctypes.create_string_buffer(256)
    rc_ = lib.emu_decode_members(bytes(blob), ctypes.c_size_t(len(blob)), slots, ctypes.byref(dst), ctypes.byref(n), ctypes.byref(m), err,
                                 ctypes.c_size_t(256))
    if rc_:
        return None, err.value.decode()
    out = ctypes.string_at(dst, n.value)
    lib.emu_free(dst)
    return out, m.value


# ------------------------------------------------------------------------------------------------ the writer did what it is for
def test_every_feature_occurred(suites):
    """the knobs are conditions, not measurements: each path the decoders carry for such streams was taken by some stream here"""
    every = [c for s in SUITES for c in suites[s]]
    for key in ("literals", "words", "matches", "words_declined", "rank388_literals", "overlapping_matches", "matches_241_255",
                "matches_below_8", "matches_above_32", "one_item_chunks", "declared_above_actual", "tables_with_unused_symbols",
                "empty_third_tables", "codes_13_15_used"):
        assert fp.total(every, key) > 0, key
    assert [max(c.counters["longest_code"][k] for c in every) for k in range(3)] == [15, 15, 15]
    assert fp.total(every, "chunks") > 3 * len(every)
    assert fp.total(suites["plain"], "overruns") == 0
    assert fp.total(suites["overrun"], "overruns") >= len(suites["overrun"])
    assert fp.total(suites["overrun"], "overruns_past_end") == 0  # (inside the member: the other suite has the rest)
    end = suites["end-overrun"]
    assert len(end) >= 12 and all(c.counters["overruns_past_end_followed"] >= 1 for c in end)
    assert all(1500 <= len(c.data) <= 6000 for c in every)


# ------------------------------------------------------------------------------------------------ the host decoder
@pytest.mark.parametrize("suite", SUITES)
def test_host_decoder(suites, suite):
    import orz_amd

    for c in suites[suite]:
        out, used = orz_amd.decode_bytes(c.stream)
        assert out == c.data and used == len(c.stream), c.name
    blob = b"".join(c.stream for c in suites[suite])
    out, m = orz_amd.decode_members(blob)
    assert m == len(suites[suite]) and out == b"".join(c.data for c in suites[suite])


# ------------------------------------------------------------------------------------------------ the kernel body
@pytest.mark.parametrize("suite", SUITES)
def test_kernel_body_one_suite(suites, emu, suite):
    cases = suites[suite]
    out, m = _emu_decode_members(emu, b"".join(c.stream for c in cases), 3)
    assert out is not None, m
    for c, at in zip(cases, rc.starts([len(c.data) for c in cases])):
        assert out[at:at + len(c.data)] == c.data, c.name
    assert m == len(cases) and len(out) == sum(len(c.data) for c in cases)


def test_kernel_body_interleaved_with_encoder_streams(mixed, emu):
    parts, streams = mixed
    assert len(parts) >= 12 + 4
    out, m = _emu_decode_members(emu, b"".join(streams), 5)  # (fewer slots than members: state blobs are used again)
    assert out is not None, m
    assert m == len(parts) and out == b"".join(parts)


# ------------------------------------------------------------------------------------------------ the framing indexes
def test_indexes_agree_on_every_member(mixed):
    import test_decode_to_device_emu as t

    lib = rc.whole_lib()
    parts, streams = mixed
    blob = b"".join(streams)
    h = t.host_index(lib, blob)
    d = t.device_index(lib, blob)
    assert h[0] == "ok" and d == h
    assert h[4] == [len(p) for p in parts] and h[5] == sum(len(p) for p in parts)
    assert h[1] == rc.starts([len(s) for s in streams])
    table = [(o + 3, len(s)) for o, s in zip(rc.starts([len(s) + 5 for s in streams]), streams)]
    buf = bytearray(b"\xee" * (table[-1][0] + table[-1][1] + 4))
    for (o, n), s in zip(table, streams):
        buf[o:o + n] = s
    d = t.device_index(lib, bytes(buf), table)
    assert d[0] == "ok" and d[4] == [len(p) for p in parts]


# ------------------------------------------------------------------------------------------------ the range reader
@pytest.fixture(scope="module")
def rounds(mixed, suites):
    return fp.read_rounds(mixed[0], suites)


@pytest.mark.parametrize("cache", ["no cache", "cursor cache"])
def test_range_reads(mixed, rounds, cache):
    parts, streams = mixed
    whole = b"".join(parts)
    r = cc.CachedEmuReader(cc.emu_lib(), b"".join(streams))
    assert r.h, r.err
    try:
        assert r.total == len(whole) and r.member_offsets == rc.starts([len(p) for p in parts])
        if cache == "cursor cache":
            r.set_cache(len(parts) * cc.cost(6400, r.state_bytes))
        seen = dict.fromkeys(cc.STAT_NAMES, 0)
        for k, batch in enumerate(rounds):
            got = r.read([(o, ln) for o, ln, _ in batch])
            assert got.rc == 0, (k, got.err)
            assert got.canary_ok and got.rest_ok
            at = 0
            for o, ln, what in batch:
                assert got.out[at:at + ln] == whole[o:o + ln], (k, what, o, ln)
                at += ln
            for key, v in r.cache_stats().items():  # (of this read)
                seen[key] += v
        if cache == "cursor cache":  # every member got a cursor in round 0 and kept it: the later rounds went on inside and behind the overrun chunks
            assert seen["fresh"] == len(parts) and seen["resumed"] > 3 * len(parts) and seen["evicted"] == 0 and seen["uncached"] == 0, seen
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ members in buffers of their own
def test_scatter_leaves_the_guard_bands(mixed):
    parts, streams = mixed
    caps = [len(p) for p in parts]
    offs, total = sc.reverse_layout(caps)
    r = sc.scatter(sc.emu_lib(), b"".join(streams), None, list(zip(offs, caps)), total, slots=7)
    assert r.rc == 0, r.err
    assert r.out_lens == caps
    sc.check_arena(r.arena, offs, caps, parts)  # (every byte outside a member's own bytes is still 0xA5: no overrun stored anything)


# ------------------------------------------------------------------------------------------------ what must be refused
def _craft(kind):
    """(data, stream) by the same writer with one thing wrong"""
    import _data

    data = _data.text(1200, seed=5) + bytes(300) + _data.text(500, seed=6)
    knobs = dict(chunk_items=(40, 90), p_declared15=0.0)
    if kind == "a table of 16 bits":
        knobs["table_hook"] = lambda k, lens, declared: (lens, 16 if k == 1 else declared)
    elif kind == "an over-subscribed code":
        knobs["table_hook"] = lambda k, lens, declared: ([1 if x else 0 for x in lens], 1) if k == 1 else (lens, declared)
    elif kind == "a first-table symbol of 389 or above":
        knobs["bad_symbol"] = (1, 7, 400)
    elif kind == "a duplicate census entry":
        knobs["census"] = [300, 7, 65, 7]
    elif kind == "a match from a node never written":
        fired = []

        def plan(w, pos):  # once, in the run of zeros: a node far down the ring of a context that has seen a few items only
            if fired or pos < 8 or any(w.data[pos - 3:pos + 20]) or len(w.data) - pos < 20:
                return None
            src, mn, ex = w.node(w.hash1(pos - 1), 2000)
            assert src is None and (mn, ex) == (4, 4)
            fired.append(pos)
            return ("match", 2000, -1, 20, fp.enc_for(20, 4, 4))

        knobs["plan"] = plan
    stream, counters = fp.write(data, 77, **knobs)
    if kind == "a match from a node never written":
        assert fired
    return data, stream


def _host_decode(stream):
    import orz_amd

    try:
        return orz_amd.decode_bytes(stream)[0]
    except Exception:
        return None


CRAFTED = {  # kind: (the device's answer, may the oracle be asked)
    "a table of 16 bits": ("member with a 16-bit Huffman table: use the host decoder", True),
    "an over-subscribed code": ("status 1)", False),  # (the reference indexes past its table there and panics; the oracle is not asked)
    "a first-table symbol of 389 or above": ("status 1)", True),
    "a duplicate census entry": ("status 1)", True),
    "a match from a node never written": ("status 1)", True),  # the documented deviation: the reference copies from window offset 0
}


@pytest.mark.parametrize("kind", sorted(CRAFTED))
def test_crafted_streams_are_refused_not_misread(oracle, emu, kind):
    data, stream = _craft(kind)
    answer, ask = CRAFTED[kind]
    good = oracle.encode(b"framed by good members", 1)
    out, msg = _emu_decode_members(emu, good + stream + good, 2)
    assert out is None and msg.endswith(answer) and ("member 1," in msg or "16-bit" in msg), msg
    host = _host_decode(stream)
    if not ask:
        assert host is None
        return
    try:
        ref = oracle.decode(stream)[0]
    except ValueError:
        ref = None
    assert host is None or host == ref, kind  # never ok with other bytes
    if kind in ("a table of 16 bits", "a match from a node never written"):
        assert ref == data and host == data  # legal by the reference's rules: the host decoder follows it
    else:
        assert ref is None and host is None


# ------------------------------------------------------------------------------------------------ the kernel body under sanitizers
def test_standalone_program_under_address_and_undefined_sanitizers(mixed, rounds, oracle, tmp_path):
    """tests/emu/freeparse_main.cpp: member decode, range reads and scatter decode of the streams above, legal and crafted, in a
    program of its own built with -fsanitize=address,undefined (nothing is loaded into this process)"""
    exe = os.path.join(ROOT, "build", "freeparse_main_san")
    src = os.path.join(ROOT, "tests", "emu", "freeparse_main.cpp")
    srcs = [src] + [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_reader_cache.cpp", "emu_decode_range.cpp", "emu_backend.cpp", "simt.h")]
    srcs += [os.path.join(ROOT, "orz_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "orz_amd", "csrc"))]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-Wno-unknown-pragmas", "-o", exe, src])
    parts, streams = mixed
    (tmp_path / "legal.orz").write_bytes(b"".join(streams))
    (tmp_path / "legal.want").write_bytes(b"".join(parts))
    (tmp_path / "legal.ranges").write_text("".join("%d %d\n" % (o, ln) for batch in rounds[::3] for o, ln, _ in batch))
    good = oracle.encode(b"framed by good members", 1)
    for k, kind in enumerate(sorted(CRAFTED)):
        (tmp_path / ("crafted%d.orz" % k)).write_bytes(good + _craft(kind)[1] + good)
    r = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert "legal: decoded three ways" in lines and sum("refused three ways" in ln for ln in lines) == len(CRAFTED), r.stdout


# ------------------------------------------------------------------------------------------------ across the window's slide
@pytest.fixture(scope="module")
def slide(oracle):
    data, stream, c = fp.write_slide()
    oracle.assert_decodes_to(stream, data, "free-parse stream across the slide")
    # a free-parse chunk ends exactly where the block does, the window slid once, and behind the slide a match was taken from the
    # node of member offset 2 (window offset 1 by then) in a context that had seen one item
    assert len(data) > fp.NEW and c["slides"] == 1 and fp.NEW in c["map"]["chunk_ends"] and c["slide_match"] == [fp.NEW + 1000]
    assert 50_000 < c["matches"] + c["literals"] + c["words"] < 200_000
    return data, stream


def test_slide_host_decoder_and_kernel_body(slide, emu):
    import orz_amd

    data, stream = slide
    out, used = orz_amd.decode_bytes(stream)
    assert out == data and used == len(stream)
    good = b"in front of the long member"
    out, m = _emu_decode_members(emu, _oracle_member(good) + stream, 2)
    assert out is not None, m
    assert m == 2 and out == good + data


def _oracle_member(data):
    import _oracle

    return _oracle.encode(data, 1)


@pytest.mark.parametrize("cache", ["no cache", "cursor cache"])
def test_slide_range_reads(slide, cache):
    data, stream = slide
    again = fp.NEW + 1000
    ranges = [(again - 10, 60), (fp.NEW - 100, 200), (0, 50), (again + 20, 3000), (len(data) - 9, 9)]
    r = cc.CachedEmuReader(cc.emu_lib(), stream)
    assert r.h, r.err
    try:
        assert r.total == len(data)
        if cache == "cursor cache":
            r.set_cache(cc.cost(len(data), r.state_bytes))
            reads = [[x] for x in sorted(ranges)]  # (the cursor stops in front of the slide, then goes on across it)
        else:
            reads = [ranges]
        for batch in reads:
            got = r.read(batch)
            assert got.rc == 0, got.err
            assert got.out == b"".join(data[o:o + ln] for o, ln in batch) and got.canary_ok and got.rest_ok
    finally:
        r.close()


def test_slide_scatter(slide):
    data, stream = slide
    offs, total = sc.reverse_layout([len(data)])
    r = sc.scatter(sc.emu_lib(), stream, None, [(offs[0], len(data))], total)
    assert r.rc == 0, r.err
    sc.check_arena(r.arena, offs, [len(data)], [data])
