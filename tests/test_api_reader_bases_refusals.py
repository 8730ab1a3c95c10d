"""What MemberReader(bases=) and MemberReader.set_bases refuse BEFORE any GPU work: the exception type and the whole message.  No
device is needed, as in test_api_delta_refusals.py: `bases` without `elems` is refused in front of everything else, and for the
rest the reader is an object made without __init__ that holds just what the checks read -- a declaration, and the CPU as the place
where its tensors lie, so that CPU tensors get as far as the checks of their sizes --; every case stops at a ValueError in front
of the first call into the library.

Left out, because the input cannot be built without a device: a base on the CPU, or on another GPU, for a reader on a GPU."""
import pytest
import torch

import orz_amd


def refused(message, fn, *args, kind=ValueError, **kw):
    with pytest.raises(kind) as e:
        fn(*args, **kw)
    assert type(e.value) is kind and str(e.value) == message


OK = torch.arange(6, dtype=torch.int16)
BYTES = torch.arange(5, dtype=torch.uint8)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


@pytest.fixture
def reader():
    r = object.__new__(orz_amd.MemberReader)
    r._h, r._lib, r._dev = 1, _NoLibrary(), torch.device("cpu")
    r._tensors, r._bases = [(6, 2), (5, 1), (0, 4)], None
    yield r
    r._h = None


def test_bases_without_elems():
    refused("bases are those of declared tensors: give elems", orz_amd.MemberReader, b"", bases=[None])
    refused("bases are those of declared tensors: give elems", orz_amd.MemberReader, OK, bases=[], pieces=[1])
    with pytest.raises(TypeError):
        orz_amd.MemberReader(b"", base=[None])


def test_the_number_of_bases(reader):
    refused("one base (or None) per tensor: 2 bases for 3 tensors", reader.set_bases, [OK, BYTES])
    refused("one base (or None) per tensor: 4 bases for 3 tensors", reader.set_bases, iter([OK, BYTES, None, None]))
    refused("one base (or None) per tensor: 1 bases for 3 tensors", reader.set_bases, [None])


def test_what_is_no_contiguous_tensor(reader):
    refused("base 1 must be a contiguous torch tensor or None", reader.set_bases, [OK, b"abcde", None])
    refused("base 0 must be a contiguous torch tensor or None", reader.set_bases, [OK.numpy(), None, None])
    strided = torch.zeros(6, 2, dtype=torch.int16).t()[0]
    assert not strided.is_contiguous() and strided.numel() == 6
    refused("base 0 must be a contiguous torch tensor or None", reader.set_bases, [strided, None, None])


def test_a_base_of_another_size(reader):
    refused("base 0 has 6 elements of 4 bytes, its tensor 6 of 2", reader.set_bases, [OK.to(torch.int32), BYTES, None])
    refused("base 0 has 5 elements of 2 bytes, its tensor 6 of 2", reader.set_bases, [OK[:5], BYTES, None])
    refused("base 0 has 12 elements of 1 bytes, its tensor 6 of 2", reader.set_bases, [OK.view(torch.uint8), None, None])  # the same bytes
    refused("base 1 has 6 elements of 1 bytes, its tensor 5 of 1", reader.set_bases, [OK, torch.zeros(6, dtype=torch.uint8), None])
    refused("base 2 has 1 elements of 4 bytes, its tensor 0 of 4", reader.set_bases, [None, None, torch.zeros(1, dtype=torch.int32)])
    assert reader._bases is None  # nothing was kept


def test_a_closed_reader(reader):
    reader._h = None
    refused("the reader is closed", reader.set_bases, [None, None, None], kind=orz_amd.OrzError)
