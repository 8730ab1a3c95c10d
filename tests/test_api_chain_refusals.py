"""What decode_planes_into(links=) and join_links refuse BEFORE any GPU work: the exception type and the whole message, and their
place among the other refusals.  And which ABI call decode_planes_into makes: the library is replaced by a recorder, so no device
is needed -- links=None makes the call it made before there was a chain, with the same arguments."""
import ctypes

import pytest
import torch

import orz_amd
from orz_amd import api

LINKS = "links is None or the number of links of a chain, an integer from 1 to 2^32 - 1"
OK = torch.arange(6, dtype=torch.int16)


def refused(message, fn, *args, kind=ValueError, **kw):
    with pytest.raises(kind) as e:
        fn(*args, **kw)
    assert type(e.value) is kind and str(e.value) == message


@pytest.fixture
def no_library(monkeypatch):
    def load():
        raise AssertionError("the library is touched")

    monkeypatch.setattr(api._native, "load", load)


@pytest.mark.parametrize("links", [0, -1, 1 << 32, 2.0, "2", True, [2], 1.5])
def test_what_is_no_number_of_links_is_refused_before_the_library_is_touched(no_library, links):
    refused(LINKS, orz_amd.decode_planes_into, b"", [], links=links)
    # ... and before every other refusal
    refused(LINKS, orz_amd.decode_planes_into, OK, [OK], elems=[2, 2], bases=[None, None], links=links)


def test_the_other_refusals_stay_as_they_are_with_links():
    for links in (1, 3):
        refused("src must be a contiguous uint8 tensor", orz_amd.decode_planes_into, OK, [], links=links)
        refused("outs must be contiguous tensors on cuda:0", orz_amd.decode_planes_into, b"", [OK], links=links)
        refused("one element size per tensor", orz_amd.decode_planes_into, b"", [], elems=[2], links=links)
        refused("one number of pieces per tensor, unsigned 32-bit", orz_amd.decode_planes_into, b"", [], pieces=[1], links=links)
        refused("one base (or None) per tensor: 1 bases for 0 outs", orz_amd.decode_planes_into, b"", [], bases=[None], links=links)
        refused("one digest per tensor, unsigned 32-bit", orz_amd.decode_planes_into, b"", [], digests=[1], links=links)


# ------------------------------------------------------------------------------------------------ join_links
def test_join_links_shifts_the_offsets():
    a, b, c = b"aaaa", b"bbbbbbb", b""
    blob, table = orz_amd.join_links([(a, [(0, 3), (3, 1)]), (bytearray(b), [(4, 3), (0, 4)]), (c, []), (a, iter([(1, 2)]))])
    assert blob == a + b + c + a and table == [(0, 3), (3, 1), (8, 3), (4, 4), (12, 2)]
    t = [torch.tensor(list(x), dtype=torch.uint8) for x in (a, b)]
    blob, table = orz_amd.join_links([(t[0], [(0, 4)]), (t[1], [(2, 5), (0, 2)])])
    assert isinstance(blob, torch.Tensor) and blob.dtype == torch.uint8 and bytes(blob.numpy()) == a + b
    assert table == [(0, 4), (6, 5), (4, 2)]
    one = orz_amd.join_links([(a, [(0, 4)])])
    assert one == (a, [(0, 4)])


def test_join_links_refusals():
    t = torch.zeros(4, dtype=torch.uint8)
    refused("a chain has at least one link", orz_amd.join_links, [])
    refused("the containers of a chain are all tensors or all bytes", orz_amd.join_links, [(t, []), (b"abcd", [])])
    refused("the containers of a chain are all tensors or all bytes", orz_amd.join_links, [(b"abcd", []), (t, [])])
    refused("a container is a uint8 tensor of one dimension", orz_amd.join_links, [(t, []), (t.to(torch.int16), [])])
    refused("a container is a uint8 tensor of one dimension", orz_amd.join_links, [(t.reshape(2, 2), [])])
    refused("the containers of a chain lie on one device", orz_amd.join_links, [(t, []), (t.to("meta"), [])])


# ------------------------------------------------------------------------------------------------ the ABI call that is made
class Recorder:
    """stands where the library stands: every function answers 0 and notes its name and arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            if not name.endswith("_host_waits"):
                self.calls.append((name, args))
            return 0

        return fn


@pytest.fixture
def recorded(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(api._native, "load", lambda: rec)
    monkeypatch.setattr(api, "_sync", lambda dev: None)
    return rec


def _plain(args):
    """the arguments as plain values: ctypes arrays as lists, byref() as its type's name"""
    out = []
    for a in args:
        if isinstance(a, ctypes.Array):
            out.append(list(a))
        elif isinstance(a, (int, type(None))):
            out.append(a)
        else:
            out.append(type(a).__name__)
    return out


@pytest.mark.parametrize("kw,name", [
    (dict(), "orz_decode_members_planes"),
    (dict(pieces=[]), "orz_decode_members_planes_pieces"),
    (dict(digests=[]), "orz_decode_tensors_verified"),
    (dict(pieces=[], digests=[]), "orz_decode_tensors_verified"),
    (dict(bases=[]), "orz_decode_tensors_delta"),
    (dict(bases=[], pieces=[], digests=[]), "orz_decode_tensors_delta"),
])
def test_links_none_makes_the_call_it_made_before(recorded, kw, name):
    assert orz_amd.decode_planes_into(b"abc", [], members=[(0, 3)], **kw) == []
    without = recorded.calls
    assert [n for n, _ in without] == [name]
    recorded.calls = []
    assert orz_amd.decode_planes_into(b"abc", [], members=[(0, 3)], links=None, **kw) == []
    assert [n for n, _ in recorded.calls] == [name]
    assert _plain(recorded.calls[0][1]) == _plain(without[0][1])


@pytest.mark.parametrize("links", [1, 2, 7])
@pytest.mark.parametrize("kw", [dict(), dict(pieces=[]), dict(digests=[]), dict(bases=[]), dict(bases=[], pieces=[], digests=[])])
def test_an_integer_makes_the_chain_call(recorded, kw, links):
    res, st = orz_amd.decode_planes_into(b"abc", [], members=[(0, 3)], links=links, stats=True, **kw)
    assert res == [] and st["host_waits"] == 0
    (name, args), = recorded.calls
    assert name == "orz_decode_tensors_chain" and len(args) == 19
    assert args[0] == 0 and args[2] == 3 and args[3] == 0 and args[6] == 1 and args[12] == 0 and args[14] == links
    # what was not given goes as NULL: bases (9), pieces (11), digests (13) and the computed digests (16)
    assert (args[9] is None) == ("bases" not in kw) and (args[11] is None) == ("pieces" not in kw)
    assert (args[13] is None) == ("digests" not in kw) and (args[16] is None) == ("digests" not in kw)
