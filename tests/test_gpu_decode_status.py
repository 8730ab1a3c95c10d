"""GPU tier: the library's four ways of decoding members on the device name a damaged member as their emulation twins do.  The
container of test_decode_status_agreement.py -- a good member, the damaged member of _rangecases, a good member -- goes through
orz_decode_members_device, orz_decode_members_to_device, orz_decode_members_scatter and a MemberReader without and with a cursor
cache; the text of each OrzError is the twin's, and the good members' bytes lie where the twin leaves them."""
import pytest

import _cachecases as cc
import test_decode_status_agreement as twin

pytestmark = pytest.mark.gpu

FILL = twin.FILL
CALLS = dict(zip(twin.DRIVERS, ("orz_decode_members_device", "orz_decode_members_to_device", "orz_decode_members_scatter", "orz_reader_read",
                                "orz_reader_read")))


def _host(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def case(oracle):
    return twin.Case(oracle)


@pytest.fixture(scope="module")
def src(case):
    import torch

    return torch.frombuffer(bytearray(case.blob(True)), dtype=torch.uint8).to("cuda:0")


def _run(name, case, src):
    """the driver on the damaged container: (the text of its OrzError or None, what lies where the members' bytes go afterwards
    -- None where nothing is handed back)"""
    import torch

    import orz_amd

    err = None
    if name == "decode_members_device":
        try:
            orz_amd.decode_members_device(case.blob(True))
        except orz_amd.OrzError as e:
            err = str(e)
        return err, None
    if name == "decode_members_scatter":
        outs = [torch.full((len(p) + 9,), FILL, dtype=torch.uint8, device="cuda:0") for p in case.plain]
        try:
            orz_amd.decode_members_into(src, outs)
        except orz_amd.OrzError as e:
            err = str(e)
        got = [_host(t) for t in outs]
        assert all(g[len(p):] == bytes([FILL]) * 9 for g, p in zip(got, case.plain))
        return err, [g[:len(p)] for g, p in zip(got, case.plain)]
    out = torch.full((case.total + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    if name == "decode_members_to_device":
        try:
            orz_amd.decode_members_to_device(src, out=out)
        except orz_amd.OrzError as e:
            err = str(e)
    else:
        cached = name == "reader with a cache"
        budget = sum(cc.cost(len(p), orz_amd.MemberReader.cursor_state_bytes()) for p in case.plain) if cached else 0
        rd = orz_amd.MemberReader(src, cache_bytes=budget)
        try:
            rd.read(0, case.total, out=out[:case.total])
        except orz_amd.OrzError as e:
            err = str(e)
            assert rd.cache_stats()["cursors"] == (2 if cached else 0)  # (the member whose decode failed lost its cursor)
        finally:
            rd.close()
    got = _host(out)
    assert got[case.total:] == bytes([FILL]) * 16
    return err, [got[s:s + len(p)] for s, p in zip(case.starts, case.plain)]


@pytest.mark.parametrize("name", twin.DRIVERS)
def test_the_error_text_is_the_emulation_twins(emu, case, src, name):
    want = twin.RUN[name](case, case.blob(True))
    assert want.err.startswith("invalid orz data (member 1, status "), want.err
    err, members = _run(name, case, src)
    assert err == "%s failed (-22): %s" % (CALLS[name], want.err)
    if members is None:
        assert want.members is None
    else:  # the good members' bytes, and for the readers the untouched place of the failed one, as on the emulation
        assert members[0] == want.members[0] == case.plain[0] and members[2] == want.members[2] == case.plain[2]
        if name.startswith("reader"):
            assert members[1] == want.members[1]
