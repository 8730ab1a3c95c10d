"""What MemberEncoder.encode_tensor_deltas and decode_planes_into(bases=) refuse BEFORE any GPU work, on CPU tensors: the exception
type and the whole message.  No device is needed, as in test_api_refusals.py: the encoder is an object made without __init__ that
holds just what the checks read, and every case stops at a ValueError in front of the first call that would touch a GPU.

Left out, because the input cannot be built without a device: a base on a GPU beside tensors on the CPU, or on another GPU; and,
in decode_planes_into, every refusal of a base that stands behind `outs` that pass ("outs must be contiguous tensors on cuda:0"
refuses every tensor a CPU can make) -- the same checks, in the same function, are covered through encode_tensor_deltas."""
import pytest
import torch

import orz_amd
from orz_amd import _native


def refused(message, fn, *args, kind=ValueError, **kw):
    with pytest.raises(kind) as e:
        fn(*args, **kw)
    assert type(e.value) is kind and str(e.value) == message


def strided(dtype=torch.int16):
    t = torch.zeros(4, 4, dtype=dtype).t()
    assert not t.is_contiguous()
    return t


OK = torch.arange(6, dtype=torch.int16)


@pytest.fixture
def enc():
    e = object.__new__(orz_amd.MemberEncoder)
    e._lib, e._devices, e._h = _native.load(), [0], None
    return e


def test_the_number_of_bases(enc):
    refused("one base (or None) per tensor: 0 bases for 1 tensors", enc.encode_tensor_deltas, [OK], [])
    refused("one base (or None) per tensor: 2 bases for 1 tensors", enc.encode_tensor_deltas, [OK], [None, None])
    refused("one base (or None) per tensor: 1 bases for 0 tensors", enc.encode_tensor_deltas, [], iter([OK]))


def test_what_is_no_contiguous_tensor(enc):
    refused("base 1 must be a contiguous torch tensor or None", enc.encode_tensor_deltas, [OK, OK], [None, b"abc"])
    refused("base 0 must be a contiguous torch tensor or None", enc.encode_tensor_deltas, [torch.zeros(16, dtype=torch.int16)], [strided()])
    refused("base 0 must be a contiguous torch tensor or None", enc.encode_tensor_deltas, [OK], [OK.numpy()])


def test_a_base_of_another_size(enc):
    refused("base 0 has 6 elements of 4 bytes, its tensor 6 of 2", enc.encode_tensor_deltas, [OK], [OK.to(torch.int32)])
    refused("base 1 has 5 elements of 2 bytes, its tensor 6 of 2", enc.encode_tensor_deltas, [OK, OK], [OK, OK[:5]])
    refused("base 0 has 12 elements of 1 bytes, its tensor 6 of 2", enc.encode_tensor_deltas, [OK], [OK.view(torch.uint8)])  # the same bytes


def test_the_tensors_own_refusals_come_first(enc):
    refused("tensors must be contiguous torch tensors", enc.encode_tensor_deltas, [strided()], [None, None])
    refused("elements of more than 8 bytes have no byte planes here: view the tensor as a narrower dtype", enc.encode_tensor_deltas,
            [torch.zeros(3, dtype=torch.complex128)], [])
    refused("the piece size is a multiple of 16 elements", enc.encode_tensor_deltas, [OK], [], piece_elems=24)
    enc._devices = [0, 1]
    refused("device-resident output needs an encoder on one GPU", enc.encode_tensor_deltas, [OK], [])


def test_out_is_checked_behind_the_bases(enc):
    refused("base 0 has 5 elements of 2 bytes, its tensor 6 of 2", enc.encode_tensor_deltas, [OK], [OK[:5]], out=torch.zeros(64, dtype=torch.uint8))
    refused("out must be a contiguous uint8 tensor on cuda:0", enc.encode_tensor_deltas, [OK], [OK], out=torch.zeros(64, dtype=torch.uint8))


def test_decode_planes_into():
    # too many bases for no tensors: the one refusal of `bases` a CPU can reach
    refused("one base (or None) per tensor: 1 bases for 0 outs", orz_amd.decode_planes_into, b"", [], bases=[None])
    refused("one base (or None) per tensor: 1 bases for 0 outs", orz_amd.decode_planes_into, b"", [], bases=[OK], digests=[])
    # the refusals in front of it stay in front of it
    refused("outs must be contiguous tensors on cuda:0", orz_amd.decode_planes_into, b"", [OK], bases=[])
    refused("one element size per tensor", orz_amd.decode_planes_into, b"", [], elems=[2], bases=[None])
    refused("src must be a contiguous uint8 tensor", orz_amd.decode_planes_into, OK, [], bases=[None])
