"""A list of buffers in, one member each; a list of buffers out, one member each (orz_members_encode_segments[_to_device],
orz_decode_members_scatter) on the GPU.  Member k's stream must be byte for byte what MemberEncoder.encode writes for segment k
alone, whichever worker takes it; the scatter decode must write each member into its own tensor and nowhere else, and must agree
with its emulation twin (tests/emu/emu_decode_scatter.cpp) on sizes and verdicts."""
import pytest

import _data
import _scattercases as sc

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 479, 4097, 70_000, 0, 300_000]
POISON = 0xA5
GUARD = 64


def _segments():
    gens = [_data.text, _data.zeros_noise, lambda n: _data.mixed(n, seed=4)]
    return [bytes(gens[k % 3](n)) if n else b"" for k, n in enumerate(LENGTHS)]


@pytest.fixture(scope="module")
def segs():
    return _segments()


@pytest.fixture(scope="module")
def encoders():
    """MemberEncoders by number of jobs, shared by the module"""
    import orz_amd

    cache = {}

    def get(jobs):
        if jobs not in cache:
            cache[jobs] = orz_amd.MemberEncoder(device=0, level=1, jobs=jobs)
        return cache[jobs]

    yield get
    for e in cache.values():
        e.close()


@pytest.fixture(scope="module")
def ref(encoders):
    """the stream of a segment alone: MemberEncoder.encode(segment, member_bytes=max(len, 1))[0], remembered per segment.  How an
    encoder was made is part of what makes a stream's bytes (the one encoder of a one-job object parses a block in two
    units, the encoders of a job with several take whole blocks), so the reference comes from an object of the same kind as the one
    under test: the one-job object for jobs == 1, the three-job object for every other number of jobs."""
    memo = {}

    def get(seg, jobs):
        key = (jobs == 1, seg)
        if key not in memo:
            memo[key] = encoders(1 if jobs == 1 else 3).encode(seg, member_bytes=max(len(seg), 1))[0]
        return memo[key]

    return get


def _odd_slices(torch, segs):
    """the segments as slices at odd offsets of ONE device tensor: no pointer is 16-byte aligned"""
    at, places = 1, []
    for s in segs:
        places.append(at)
        at += len(s) + (2 if (at + len(s)) % 2 else 3)  # the next start is odd again
    pool = torch.zeros(at + 16, dtype=torch.uint8, device="cuda:0")
    views = []
    for s, p in zip(segs, places):
        if s:
            pool[p:p + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).to("cuda:0")
        views.append(pool[p:p + len(s)])
    assert all(v.data_ptr() % 2 == 1 for v in views if v.numel())
    return pool, views


def _check_table(members, cap):
    spans = sorted((o, o + ln) for o, ln in members)
    assert all(ln > 0 for _, ln in members)  # (an empty member still has its EOF byte)
    assert spans[0][0] >= 0 and spans[-1][1] <= cap
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans


@pytest.fixture(scope="module")
def first_container(encoders, segs):
    """(container tensor, members) of the segments encoded from device memory by three workers: what the scatter tests decode"""
    import torch

    pool, views = _odd_slices(torch, segs)
    container, members = encoders(3).encode_tensors(views)
    return container, members


@pytest.mark.parametrize("jobs", [1, 3, 8])
@pytest.mark.parametrize("where", ["device", "host"])
def test_each_segment_is_a_member_of_its_own(encoders, ref, oracle, segs, jobs, where):
    import torch

    enc = encoders(jobs)
    if where == "device":
        pool, tensors = _odd_slices(torch, segs)
    else:
        tensors = [torch.frombuffer(bytearray(s), dtype=torch.uint8) if s else torch.empty(0, dtype=torch.uint8) for s in segs]
    cap = enc.bound_segments([len(s) for s in segs])
    out = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device="cuda:0")
    container, members = enc.encode_tensors(tensors, out=out[:cap])
    assert container.data_ptr() == out.data_ptr() and len(members) == len(segs)
    _check_table(members, cap)
    host = bytes(out.cpu().numpy())
    assert host[cap:] == bytes([POISON]) * GUARD
    streams = [host[o:o + ln] for o, ln in members]
    for k, (s, seg) in enumerate(zip(streams, segs)):
        assert s == ref(seg, jobs), "member %d (%d bytes in) differs from the segment encoded alone" % (k, len(seg))
    # the concatenation in member order, through the oracle's decoder, stream by stream
    cat, at = b"".join(streams), 0
    for seg in segs:
        back, used = oracle.decode(cat[at:])
        assert back == seg
        at += used
    assert at == len(cat)
    if where == "host":  # the host-output variant: the same streams, concatenated
        blob, lens = enc.encode_segments(segs)
        assert lens == [len(s) for s in streams] and blob == cat


def test_a_member_of_two_blocks_that_is_not_first(encoders, ref, segs):
    import orz_amd
    import torch

    big = _data.text((16 << 20) + 5, seed=8)  # two blocks, one slide
    parts = [segs[3], big, segs[2]]
    tensors = [torch.frombuffer(bytearray(p), dtype=torch.uint8).to("cuda:0") for p in parts]
    container, members = encoders(3).encode_tensors(tensors)
    _check_table(members, container.numel())
    host = bytes(container.cpu().numpy())
    streams = [host[o:o + ln] for o, ln in members]
    assert streams[0] == ref(parts[0], 3) and streams[2] == ref(parts[2], 3)
    assert streams[1] == ref(big, 3)
    back, n = orz_amd.decode_members(b"".join(streams))  # (the host decoder: a fraction of a second)
    assert n == 3 and back == b"".join(parts)


def test_no_segments(encoders):
    import torch

    enc = encoders(3)
    assert enc.encode_segments([]) == (b"", [])
    assert enc.encode_segments_to_device([], [], 0, 0) == []
    container, members = enc.encode_tensors([])
    assert container.numel() == 0 and members == []
    out = torch.full((32,), POISON, dtype=torch.uint8, device="cuda:0")
    container, members = enc.encode_tensors([], out=out)
    assert members == [] and bytes(out.cpu().numpy()) == bytes([POISON]) * 32


def test_output_one_byte_short(encoders, ref, segs):
    import orz_amd
    import torch

    tensors = [torch.frombuffer(bytearray(s), dtype=torch.uint8).to("cuda:0") if s else torch.empty(0, dtype=torch.uint8, device="cuda:0")
               for s in segs]
    for jobs in (1, 3):
        need = sum(len(ref(s, jobs)) for s in segs)
        out = torch.empty(need, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(orz_amd.OrzError, match=r"\(-12\)"):
            encoders(jobs).encode_tensors(tensors, out=out[:need - 1])
        container, members = encoders(jobs).encode_tensors(tensors, out=out)  # exactly enough: the members fill it
        _check_table(members, need)
        assert sum(ln for _, ln in members) == need


def test_a_segment_inside_the_output_is_refused(encoders, segs):
    import orz_amd
    import torch

    enc = encoders(3)
    buf = torch.zeros(200_000, dtype=torch.uint8, device="cuda:0")
    other = torch.zeros(5000, dtype=torch.uint8, device="cuda:0")
    for seg in (buf[100_000:104_097], buf[:1], buf[199_999:]):
        with pytest.raises(orz_amd.OrzError, match=r"\(-22\).*overlaps"):
            enc.encode_tensors([other, seg], out=buf)
    # null arrays and null segments of some length are refused on the host too
    with pytest.raises(orz_amd.OrzError, match=r"\(-22\)"):
        enc.encode_segments_to_device([0], [5], buf.data_ptr(), buf.numel())
    container, members = enc.encode_tensors([other, buf[100_000:104_097]], out=torch.empty(70_000, dtype=torch.uint8, device="cuda:0"))
    assert len(members) == 2


def test_small_members_behind_one_that_fills_the_arena(encoders, ref, segs):
    """one 300,000-byte segment, then six of 4,097 bytes: whatever the large member does to the arena's counter, the streams are
    those of the segments alone (where they were staged is not observable here: correctness only)"""
    import orz_amd
    import torch

    big, small = segs[6], [_data.mixed(4097, seed=20 + k) for k in range(6)]
    parts = [big] + small
    for jobs in (1, 3):
        want = [ref(p, jobs) for p in parts]
        blob, lens = encoders(jobs).encode_segments(parts)
        assert lens == [len(w) for w in want] and blob == b"".join(want)
    # a caller's buffer the large member cannot enter fails the job whatever the small ones would need
    tensors = [torch.frombuffer(bytearray(p), dtype=torch.uint8).to("cuda:0") for p in parts]
    with pytest.raises(orz_amd.OrzError, match=r"\(-12\)"):
        encoders(1).encode_tensors(tensors, out=torch.empty(len(want[0]) - 1 + sum(lens[1:]), dtype=torch.uint8, device="cuda:0"))


# ------------------------------------------------------------------------------------------------ scatter
def _destinations(torch, segs, order):
    """a tensor per segment of a dtype its length divides by (int32, float16, uint8), carved in REVERSE order out of one poisoned
    arena with guard gaps (16-byte aligned starts, as typed tensors need)"""
    dtypes = []
    for k, s in enumerate(segs):
        dtypes.append(torch.int32 if len(s) % 4 == 0 and k % 2 == 0 else (torch.float16 if len(s) % 2 == 0 else torch.uint8))
    caps = [len(s) for s in segs]
    at, offs = GUARD, [0] * len(segs)
    for k in reversed(order):
        offs[k] = at
        at += (caps[k] + GUARD + 15) // 16 * 16
    arena = torch.full((at,), POISON, dtype=torch.uint8, device="cuda:0")
    outs = [arena[o:o + c].view(dt) for o, c, dt in zip(offs, caps, dtypes)]
    assert {torch.int32, torch.float16, torch.uint8} <= set(dtypes)
    return arena, outs, offs, caps


def _emulated(container, members, segs):
    lib = sc.emu_lib()
    blob = bytes(container.cpu().numpy())
    caps = [len(s) for s in segs]
    offs, total = sc.reverse_layout(caps)
    return sc.scatter(lib, blob, members, [(o if c else None, c) for o, c in zip(offs, caps)], total)


@pytest.mark.parametrize("order", ["member order", "permuted"])
def test_scatter_into_tensors_of_mixed_dtypes(first_container, segs, order):
    import orz_amd
    import torch

    container, members = first_container
    perm = list(range(len(segs))) if order == "member order" else [4, 6, 0, 2, 5, 1, 3]
    want = [segs[k] for k in perm]
    table = [members[k] for k in perm]
    arena, outs, offs, caps = _destinations(torch, want, list(range(len(want))))
    sizes, st = orz_amd.decode_members_into(container, outs, device=0, members=table, stats=True)
    assert sizes == [len(s) for s in want]
    sc.check_arena(bytes(arena.cpu().numpy()), offs, caps, want, fill=POISON)
    for t, s in zip(outs, want):
        assert bytes(t.view(torch.uint8).cpu().numpy()) == s
    assert st["host_waits"] == 5 and st["members"] == len(segs) and st["launches"] == 1
    emu = _emulated(container, table, want)
    assert emu.rc == 0 and emu.out_lens == sizes and emu.host_waits == st["host_waits"] and emu.launches == st["launches"]


def test_scatter_of_a_concatenation_from_host_memory(first_container, segs):
    import orz_amd
    import torch

    container, members = first_container
    host = bytes(container.cpu().numpy())
    cat = b"".join(host[o:o + ln] for o, ln in members)
    arena, outs, offs, caps = _destinations(torch, segs, list(range(len(segs))))
    sizes, st = orz_amd.decode_members_into(cat, outs, device=0, stats=True)
    assert sizes == [len(s) for s in segs] and st["host_waits"] == 5
    sc.check_arena(bytes(arena.cpu().numpy()), offs, caps, segs, fill=POISON)


def test_a_tensor_one_byte_short_leaves_every_tensor_untouched(first_container, segs):
    import orz_amd
    import torch

    container, members = first_container
    arena, outs, offs, caps = _destinations(torch, segs, list(range(len(segs))))
    short = list(outs)
    short[4] = outs[4].view(torch.uint8)[:-1]
    with pytest.raises(orz_amd.OrzError, match=r"\(-12\).*member 4 "):
        orz_amd.decode_members_into(container, short, device=0, members=members)
    assert bytes(arena.cpu().numpy()) == bytes([POISON]) * arena.numel()
    emu_caps = [len(s) for s in segs]
    emu_caps[4] -= 1
    eo, total = sc.reverse_layout(emu_caps)
    emu = sc.scatter(sc.emu_lib(), bytes(container.cpu().numpy()), members, [(o if c else None, c) for o, c in zip(eo, emu_caps)], total)
    assert emu.rc == sc.ENOMEM and "member 4 " in emu.err


def test_overlapping_tensors_and_a_wrong_count_are_refused(first_container, segs):
    import orz_amd
    import torch

    container, members = first_container
    arena, outs, offs, caps = _destinations(torch, segs, list(range(len(segs))))
    over = list(outs)
    over[3] = arena[offs[4] + 10:offs[4] + 10 + caps[3]]  # inside tensor 4
    with pytest.raises(orz_amd.OrzError, match=r"\(-22\).*overlap"):
        orz_amd.decode_members_into(container, over, device=0, members=members)
    with pytest.raises(orz_amd.OrzError, match=r"\(-22\).*6 destinations for 7 members"):
        orz_amd.decode_members_into(container, outs[:-1], device=0, members=members)
    inside = list(outs)
    inside[6] = container[:caps[6]] if container.numel() >= caps[6] else container
    with pytest.raises(orz_amd.OrzError, match=r"\(-22\)"):
        orz_amd.decode_members_into(container, inside, device=0, members=members)
    assert bytes(arena.cpu().numpy()) == bytes([POISON]) * arena.numel()


def test_tensors_round_trip(encoders):
    import orz_amd
    import torch

    g = torch.Generator().manual_seed(5)
    tensors = [torch.randint(0, 50, (n,), generator=g, dtype=dt).to("cuda:0")
               for n, dt in [(1000, torch.int32), (333, torch.uint8), (0, torch.int64), (4096, torch.int16), (77, torch.int64),
                             (2500, torch.uint8), (1, torch.int32), (640, torch.int16)]]
    tensors[3] = tensors[3].view(torch.float16)
    container, members = encoders(3).encode_tensors(tensors)
    assert container.numel() == max(o + ln for o, ln in members)
    outs = [torch.full_like(t, 7) for t in tensors]
    sizes = orz_amd.decode_members_into(container, outs, device=0, members=members)
    assert sizes == [t.numel() * t.element_size() for t in tensors]
    for t, o in zip(tensors, outs):
        assert torch.equal(t.view(torch.uint8), o.view(torch.uint8))
    # the table composes with the reader: tensor k's bytes are a range of the decoded data
    rd = orz_amd.MemberReader(container, device=0, members=members)
    try:
        starts = rd.member_offsets
        for k in (0, 3, 4, 7):
            got = rd.read(starts[k], sizes[k])
            assert torch.equal(got, tensors[k].view(torch.uint8).reshape(-1))
    finally:
        rd.close()
