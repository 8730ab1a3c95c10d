"""Tensors as byte planes on the GPU (orz_members_encode_planes_to_device, orz_decode_members_planes): every plane member's
stream must be byte for byte what an encoder of the same kind writes for that plane's numpy bytes alone, the decode must merge
the planes back into the tensors and write nowhere else, and it must agree with its emulation twin (tests/emu/emu_planes.cpp) on
sizes, verdicts, messages, launches and host waits.  (Planes of several blocks are not tested again: a plane is an ordinary
segment, test_gpu_segments.py::test_a_member_of_two_blocks_that_is_not_first covers those.)"""
import pytest

import _planecases as pc

pytestmark = pytest.mark.gpu

POISON, GUARD = pc.POISON, pc.GUARD


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
    """the stream of some bytes alone, from an object of the same kind as the one under test (tests/test_gpu_segments.py: the
    one-job object for jobs == 1, the three-job object for every other number of jobs), remembered"""
    memo = {}

    def get(data, jobs):
        key = (jobs == 1, data)
        if key not in memo:
            memo[key] = encoders(1 if jobs == 1 else 3).encode(data, member_bytes=max(len(data), 1))[0]
        return memo[key]

    return get


def _dev(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0") if data else torch.empty(0, dtype=torch.uint8, device="cuda:0")


def _typed(torch, data, e):
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[e]
    return _dev(torch, data).view(dt) if data else torch.empty(0, dtype=dt, device="cuda:0")


def _streams(container, members):
    host = bytes(container.cpu().numpy())
    return [host[o:o + ln] for o, ln in members]


def _check_table(members, cap):
    spans = sorted((o, o + ln) for o, ln in members)
    assert all(ln > 0 for _, ln in members)  # (an empty member still has its EOF byte)
    assert spans[0][0] >= 0 and spans[-1][1] <= cap
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans


@pytest.fixture(scope="module")
def cases():
    """the shared cases: every element size at every count in ONE call, empty tensors between them"""
    return pc.mixed_tensors()


# ------------------------------------------------------------------------------------------------ streams
@pytest.mark.parametrize("jobs", [1, 3])
def test_each_plane_is_a_member_of_its_own(encoders, ref, oracle, cases, jobs):
    import torch

    tensors = [_typed(torch, d, e) for d, e in cases]
    container, members, elems = encoders(jobs).encode_tensor_planes(tensors)
    assert elems == [e for _, e in cases] and len(members) == sum(elems)
    _check_table(members, container.numel())
    planes = pc.planes_of(cases)
    for k, (s, pl) in enumerate(zip(_streams(container, members), planes)):
        assert s == ref(pl, jobs), "member %d (a plane of %d bytes) differs from the plane encoded alone" % (k, len(pl))
        back, used = oracle.decode(s)
        assert back == pl and used == len(s)


def test_host_tensors_give_the_same_streams(encoders, cases):
    import torch

    dev = [_typed(torch, d, e) for d, e in cases]
    host = [t.cpu() for t in dev]
    a, ma, _ = encoders(3).encode_tensor_planes(dev)
    b, mb, _ = encoders(3).encode_tensor_planes(host)
    assert _streams(a, ma) == _streams(b, mb)


def test_raw_call_with_segments_at_odd_addresses(encoders, oracle, cases):
    """the segments as slices at odd offsets of ONE device tensor: no pointer is even 2-byte aligned, every unit goes byte by byte"""
    import torch

    at, places = 1, []
    for d, _ in cases:
        places.append(at)
        at += len(d) + (2 if (at + len(d)) % 2 else 3)
    pool = torch.zeros(at + 16, dtype=torch.uint8, device="cuda:0")
    for (d, _), p in zip(cases, places):
        if d:
            pool[p:p + len(d)] = _dev(torch, d)
    ptrs = [pool.data_ptr() + p for p in places]
    assert all(p % 2 == 1 for p in ptrs)
    enc = encoders(3)
    lengths, elems = [len(d) for d, _ in cases], [e for _, e in cases]
    cap = enc.bound_planes(lengths, elems)
    out = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    members = enc.encode_planes_to_device(ptrs, lengths, elems, out.data_ptr(), cap)
    assert len(members) == sum(elems)
    _check_table(members, cap)
    host = bytes(out.cpu().numpy())
    assert host[cap:] == bytes([POISON]) * GUARD
    for (o, ln), pl in zip(members, pc.planes_of(cases)):
        assert oracle.decode(host[o:o + ln]) == (pl, ln)
    assert enc.encode_planes_to_device([], [], [], 0, 0) == []
    assert enc.encode_tensor_planes([])[1:] == ([], [])


def test_what_the_encode_refuses(encoders):
    import orz_amd
    import torch

    enc = encoders(3)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    out = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda:0")
    for lens, elems in (([30], [3]), ([30], [0]), ([30], [16]), ([30], [4]), ([32, 7], [4, 2])):
        with pytest.raises(orz_amd.OrzError, match=r"\(-22\)"):
            enc.encode_planes_to_device([buf.data_ptr()] * len(lens), lens, elems, out.data_ptr(), out.numel())
    with pytest.raises(orz_amd.OrzError, match=r"\(-22\).*overlaps"):
        enc.encode_planes_to_device([out.data_ptr() + 64], [32], [4], out.data_ptr(), out.numel())
    with pytest.raises(ValueError):
        enc.encode_tensor_planes([torch.zeros(4, dtype=torch.complex128, device="cuda:0")])
    small = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(orz_amd.OrzError, match=r"\(-12\)"):
        enc.encode_tensor_planes([buf.view(torch.int32)], out=small)


# ------------------------------------------------------------------------------------------------ round trip
def _originals(torch):
    g = torch.Generator().manual_seed(5)

    def ints(n, dt):
        return torch.randint(0, 50, (n,), generator=g, dtype=dt)

    return [
        (torch.randn(4097, generator=g) * 0.02).to(torch.bfloat16),
        torch.randn(1029, generator=g) * 0.02,
        torch.arange(333, dtype=torch.int64) * 3 + ints(333, torch.int64),
        ints(640, torch.int16),
        ints(2500, torch.uint8),
        torch.empty(0, dtype=torch.int64),
        ints(1, torch.int32), ints(1, torch.int64), ints(1, torch.uint8),
        (torch.randn(17, generator=g)).to(torch.bfloat16), torch.randn(17, generator=g), ints(17, torch.int64),
        ints(16, torch.int16), ints(15, torch.int64),
    ]


@pytest.fixture(scope="module")
def packed(encoders):
    """(tensors on the device, container, members, elems) of the round trip's tensors, encoded by three workers"""
    import torch

    tensors = [t.to("cuda:0") for t in _originals(torch)]
    container, members, elems = encoders(3).encode_tensor_planes(tensors)
    return tensors, container, members, elems


def _destinations(torch, tensors, room=0):
    """a tensor like each of `tensors`, carved in REVERSE order out of one poisoned arena with guard gaps (16-byte aligned starts, as
    typed tensors need): (arena, outs, offsets, sizes)"""
    sizes = [t.numel() * t.element_size() for t in tensors]
    at, offs = GUARD, [0] * len(tensors)
    for k in reversed(range(len(tensors))):
        offs[k] = at
        at += (sizes[k] + room + GUARD + 15) // 16 * 16
    arena = torch.full((at,), POISON, dtype=torch.uint8, device="cuda:0")
    outs = [arena[o:o + s].view(t.dtype) for o, s, t in zip(offs, sizes, tensors)]
    return arena, outs, offs, sizes


def _bytes_of(torch, t):
    return bytes(t.contiguous().view(torch.uint8).reshape(-1).cpu().numpy())


def test_tensors_round_trip(packed):
    import orz_amd
    import torch

    tensors, container, members, elems = packed
    assert elems == [t.element_size() for t in tensors] and {1, 2, 4, 8} == set(elems)
    arena, outs, offs, sizes = _destinations(torch, tensors)
    got, st = orz_amd.decode_planes_into(container, outs, device=0, members=members, stats=True)
    assert got == sizes
    for t, o in zip(tensors, outs):
        assert torch.equal(t.view(torch.uint8), o.view(torch.uint8))
    pc.same(bytes(arena.cpu().numpy()), pc.expect_arena(arena.numel(), [(o, _bytes_of(torch, t)) for o, t in zip(offs, tensors)]), "the arena")
    assert st["host_waits"] == 5 and st["members"] == sum(elems) and st["launches"] == 1
    # a concatenation from host memory, element sizes given: the same bytes, one wait for the upload instead of the table's
    cat = b"".join(_streams(container, members))
    arena2, outs2, offs2, _ = _destinations(torch, tensors)
    got2, st2 = orz_amd.decode_planes_into(cat, [o.view(torch.uint8) for o in outs2], device=0, elems=elems, stats=True)
    assert got2 == sizes and st2["host_waits"] == 5
    assert torch.equal(arena2, arena)


def test_gpu_equals_emulation(packed):
    import orz_amd
    import torch

    tensors, container, members, elems = packed
    lib = pc.emu_lib()
    blob = bytes(container.cpu().numpy())
    sizes = [t.numel() * t.element_size() for t in tensors]

    def both(places_caps, el, table=members):
        """the call on the GPU and on the emulation with the same capacities: (OrzError text or None, sizes / stats, emulation)"""
        arena, outs, offs, _ = _destinations(torch, tensors, room=16)
        views = [arena[o:o + c] for o, c in zip(offs, places_caps)]
        eo, total = pc.layout(places_caps, [0] * len(places_caps), reverse=True)
        emu = pc.decode_planes(lib, blob, table, list(zip(eo, places_caps)), el, total)
        try:
            got = orz_amd.decode_planes_into(container, views, device=0, members=table, elems=el, stats=True)
            return None, got, emu, arena
        except orz_amd.OrzError as e:
            return str(e), None, emu, arena

    err, got, emu, _ = both(sizes, elems)
    assert err is None and emu.rc == 0, (err, emu.err)
    assert got[0] == emu.out_lens == sizes
    assert (got[1]["launches"], got[1]["host_waits"], got[1]["members"]) == (emu.launches, emu.host_waits, emu.members)
    # verdicts and messages: the destination and member numbers agree because the whole message does
    short = list(sizes)
    short[3] -= 1
    wrong = list(elems)
    wrong[0], wrong[1] = 1, 1  # 3 planes fewer
    unequal = list(elems)
    unequal[0], unequal[1] = 4, 2  # bf16 x 4097 and fp32 x 1029 read as 4 + 2 planes: members 0 (4097 bytes) and 2 (1029) differ
    for caps, el, code in ((short, elems, pc.ENOMEM), (sizes, wrong, pc.EINVAL), (sizes, unequal, pc.EINVAL), (sizes, elems[:-1] + [3], pc.EINVAL)):
        err, got, emu, arena = both(caps, el)
        assert emu.rc == code and err is not None and "(%d)" % code in err, (err, emu.err)
        assert err.split("): ", 1)[1] == emu.err, (err, emu.err)
        assert emu.launches == 0 and bytes(arena.cpu().numpy()) == bytes([POISON]) * arena.numel()


def test_reader_reads_planes(packed):
    import orz_amd
    import torch

    tensors, container, members, elems = packed
    rd = orz_amd.MemberReader(container, device=0, members=members)
    try:
        starts = rd.member_offsets
        m = 0
        for k, (t, e) in enumerate(zip(tensors, elems)):
            planes = pc.np_split(_bytes_of(torch, t), e)
            for p in (0, e - 1):
                if k in (0, 2, 4, 10) and planes[p]:
                    got = rd.read(starts[m + p], len(planes[p]))
                    assert bytes(got.cpu().numpy()) == planes[p], "plane %d of tensor %d" % (p, k)
            m += e
        assert m == len(members)
    finally:
        rd.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_what_the_decode_refuses(packed):
    import orz_amd
    import torch

    tensors, container, members, elems = packed

    def fresh():
        arena, outs, offs, sizes = _destinations(torch, tensors)
        return arena, [o.view(torch.uint8) for o in outs], offs, sizes

    def refused(arena, outs, el, pattern, table=members):
        with pytest.raises(orz_amd.OrzError, match=pattern):
            orz_amd.decode_planes_into(container, outs, device=0, members=table, elems=el)
        assert bytes(arena.cpu().numpy()) == bytes([POISON]) * arena.numel()

    total = sum(elems)
    arena, outs, offs, sizes = fresh()
    refused(arena, outs[:-1], elems[:-1], r"\(-22\).*%d planes for %d members" % (total - elems[-1], total))  # a wrong plane count
    refused(arena, outs, [1] + elems[1:], r"\(-22\).*%d planes for %d members" % (total - 1, total))
    refused(arena, outs, elems[:4] + [3] + elems[5:], r"\(-22\).*destination 4 .* 3 bytes")  # an element size of 3
    refused(arena, outs, [4, 2] + elems[2:], r"\(-22\).*destination 0 .*member 2 ")  # planes of unequal size
    short = list(outs)
    short[2] = outs[2][:-1]
    refused(arena, short, elems, r"\(-12\).*destination 2 ")  # a capacity one byte short
    short[0] = outs[0][:-1]
    refused(arena, short, elems, r"\(-12\).*destination 0 ")  # the FIRST short one is named
    over = list(outs)
    over[3] = arena[offs[4] + 10:offs[4] + 10 + sizes[3]]  # inside tensor 4
    refused(arena, over, elems, r"\(-22\).*overlap")
    inside = list(outs)
    inside[4] = container[:sizes[4]]
    with pytest.raises(orz_amd.OrzError, match=r"\(-22\).*container"):
        orz_amd.decode_planes_into(container, inside, device=0, members=members, elems=elems)
    assert bytes(arena.cpu().numpy()) == bytes([POISON]) * arena.numel()
    with pytest.raises(ValueError):
        orz_amd.decode_planes_into(container, outs, device=0, members=members, elems=elems[:-1])


# ------------------------------------------------------------------------------------------------ size
def test_planes_are_smaller_than_whole_tensors(encoders):
    """The oracle's encoder at level 1 gives planes / whole = 0.879 for the bf16 input and 0.202 for the int64 input; the
    fast parse is held to half a percent of the oracle per stream, so both thresholds keep several percent of slack."""
    import torch

    enc = encoders(1)
    g = torch.Generator().manual_seed(1)
    weights = (torch.randn(1 << 19, generator=g) * 0.02).to(torch.bfloat16).to("cuda:0")
    g = torch.Generator().manual_seed(2)
    ids = (torch.arange(1 << 17, dtype=torch.int64) * 3 + torch.randint(0, 3, (1 << 17,), generator=g, dtype=torch.int64)).to("cuda:0")
    for t, limit in ((weights, 0.95), (ids, 0.5)):
        assert t.numel() * t.element_size() == 1 << 20
        whole = sum(ln for _, ln in enc.encode_tensors([t])[1])
        planes = sum(ln for _, ln in enc.encode_tensor_planes([t])[1])
        print("%s: %d bytes in, whole %d, planes %d, planes / whole %.3f" % (t.dtype, 1 << 20, whole, planes, planes / whole))
        assert planes <= limit * whole, (t.dtype, whole, planes)
