"""GPU tier: members decoded from and into device memory (orz_decode_members_to_device, orz_amd.decode_members_to_device).  Bars:
the members MemberEncoder / StreamEncoder leave in HBM come back equal to the input tensor, oracle-made containers decode to what
the host decoder writes from HBM and from host memory alike, nothing outside the output is written and nothing in it is read
before it is written, ENOMEM / EINVAL come before any decode and leave the library usable."""
import ctypes

import pytest

import _data

pytestmark = pytest.mark.gpu


def _dev(data, device=0):
    import torch

    return torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8)[: len(data)].to("cuda:%d" % device)


def _host(t):
    return t.cpu().numpy().tobytes()


def _parts():
    return [(_data.mixed(120_000, seed=1), 1), (b"", 1), (_data.zeros_noise(90_000), 2), (b"x", 1), (_data.random_bytes(30_000), 0),
            (_data.periodic(40_000, 3), 1), (_data.mixed(50_000, seed=9), 0)]


@pytest.fixture(scope="module")
def container(oracle):
    parts = _parts()
    return b"".join(p for p, _ in parts), b"".join(oracle.encode(p, lv) for p, lv in parts), len(parts)


def test_members_left_in_hbm_decode_to_the_input():
    """finish order, offs / lens: straight from MemberEncoder.encode_to_device; the first member is more than one block"""
    import corpus
    import torch

    import orz_amd

    data = corpus.enwik_like(17_600_000)
    src = _dev(data)
    mb = (1 << 24) + 400_000
    cap = 2 * orz_amd.stream_bound(mb)
    streams = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    enc = orz_amd.MemberEncoder(device=0, level=1, jobs=2)
    try:
        members = enc.encode_to_device(src.data_ptr(), len(data), streams.data_ptr(), cap, member_bytes=mb)
    finally:
        enc.close()
    assert len(members) == 2
    out, m, offs, st = orz_amd.decode_members_to_device(streams, members=members, offsets=True, stats=True)
    assert m == 2 and offs == [0, mb] and out.device == src.device
    assert torch.equal(out, src)
    assert st["members"] == 2 and st["launches"] == 1 and st["kernel_ms"] > 0


def test_a_single_stream_left_in_hbm():
    import torch

    import orz_amd

    data = _data.text(700_000, seed=9)
    src = _dev(data)
    cap = orz_amd.stream_bound(len(data))
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    enc = orz_amd.StreamEncoder(device=0, level=1)
    try:
        n = enc.encode_to_device(src.data_ptr(), len(data), dst.data_ptr(), cap)
    finally:
        enc.close()
    out, m = orz_amd.decode_members_to_device(dst[:n])
    assert m == 1 and torch.equal(out, src)


def test_oracle_containers_from_hbm_and_from_host(container):
    import orz_amd

    data, blob, k = container
    want, m = orz_amd.decode_members(blob)
    assert want == data and m == k
    out, m = orz_amd.decode_members_to_device(_dev(blob))
    assert m == k and _host(out) == want
    out, m = orz_amd.decode_members_to_device(blob)  # host memory: src_on_device = 0
    assert m == k and _host(out) == want
    import torch

    out, m = orz_amd.decode_members_to_device(torch.frombuffer(bytearray(blob), dtype=torch.uint8))  # a CPU tensor
    assert m == k and _host(out) == want


def test_poisoned_destination_canaries_capacity_and_sizing(container):
    import torch

    import orz_amd
    from orz_amd import _native

    data, blob, k = container
    src = _dev(blob)
    lib = _native.load()
    dlen, nm = ctypes.c_size_t(), ctypes.c_size_t()
    offs = (ctypes.c_size_t * k)()
    rc = lib.orz_decode_members_to_device(0, ctypes.c_void_p(src.data_ptr()), len(blob), 1, None, None, 0, None, 0, ctypes.byref(dlen),
                                          ctypes.byref(nm), offs, None)
    assert rc == 0 and dlen.value == len(data) and nm.value == k
    sizes = [len(p) for p, _ in _parts()]
    assert list(offs) == [sum(sizes[:i]) for i in range(k)]
    total = len(data)
    buf = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    buf[total:] = 0x5A
    with pytest.raises(orz_amd.OrzError, match=r"\(-12\)"):  # one byte short: nothing written
        orz_amd.decode_members_to_device(src, out=buf[: total - 1])
    assert bool((buf[:total] == 0xA5).all()) and bool((buf[total:] == 0x5A).all())
    out, m = orz_amd.decode_members_to_device(src, out=buf[:total])
    assert m == k and _host(out) == data
    assert bool((buf[total:] == 0x5A).all())


def test_bad_data_is_reported_and_the_library_lives_on(container, oracle):
    import orz_amd

    data, blob, k = container
    good = [oracle.encode(p, lv) for p, lv in _parts()]
    bad = b"".join(good[:3]) + good[3][:-1]  # member 3 lost its EOF byte
    with pytest.raises(orz_amd.OrzError, match=r"\(-22\).*member 3"):
        orz_amd.decode_members_to_device(_dev(bad))
    members = [(0, len(good[0])), (len(good[0]), len(good[1]) + 1)]  # member 1's entry runs past its EOF byte
    with pytest.raises(orz_amd.OrzError, match=r"\(-22\).*EOF byte \(member 1\)"):
        orz_amd.decode_members_to_device(_dev(good[0] + good[1] + good[2]), members=members)
    flipped = bytearray(good[0])
    for i in range(200, len(flipped), 997):  # a corrupted payload: the decode kernel reports it
        flipped[i] ^= 0x5A
    try:
        out, m = orz_amd.decode_members_to_device(_dev(bytes(flipped)))
        assert m == 1
    except orz_amd.OrzError as e:
        assert "(-22)" in str(e)
    out, m = orz_amd.decode_members_to_device(_dev(blob))
    assert m == k and _host(out) == data


def test_decode_slots(container, monkeypatch):
    import orz_amd

    data, blob, k = container
    monkeypatch.setenv("ORZ_DECODE_SLOTS", "3")
    out, m, st = orz_amd.decode_members_to_device(_dev(blob), stats=True)
    assert m == k == 7 and st["launches"] == 3 and _host(out) == data


def test_nothing_to_decode():
    import torch

    import orz_amd

    out, m = orz_amd.decode_members_to_device(b"")
    assert m == 0 and out.numel() == 0
    out, m = orz_amd.decode_members_to_device(torch.empty(0, dtype=torch.uint8, device="cuda:0"))
    assert m == 0 and out.numel() == 0


def test_two_devices(container):
    """the decode kernel's LDS attribute is set per (kernel, device): a process that decodes on device 0 and then on device 1
    launches on device 1 with it too.  Skipped on a one-GPU box."""
    import orz_amd
    from orz_amd import _native

    if _native.load().orz_device_count() < 2:
        pytest.skip("needs two HIP devices")
    data, blob, k = container
    for device in (0, 1):
        out, m = orz_amd.decode_members_to_device(_dev(blob, device), device=device)
        assert m == k and out.device.index == device and _host(out) == data
