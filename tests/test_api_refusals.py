"""What orz_amd/api.py refuses of the tensor-list calls BEFORE any GPU work: the exception type, the whole message and, for an input
that is wrong in two ways, which refusal wins.  No device is needed: the library loads without one, torch.device("cuda", 0) is only
a name, and every case stops at a ValueError in front of the first call that would touch a GPU.  A MemberEncoder and an open
MemberReader cannot be constructed without a device, so their methods run on objects made without __init__ that hold just what the
checks read.

Left out, because the input cannot be built without a device:
  * tensors on the CPU mixed with tensors on a GPU, and tensors on another GPU ("tensors must all lie on cuda:0 or all on the CPU");
  * a `src` tensor on another GPU ("src lies on cuda:1, not on cuda:0");
  * `outs` that pass ("outs must be contiguous tensors on cuda:0" refuses every tensor a CPU can make), and with them `pieces` and
    `digests` of the right length but out of range in decode_members_into / decode_planes_into -- the same range checks are
    covered through MemberReader.set_planes and through lists that are too long for no tensors."""
import zlib

import pytest
import torch

import orz_amd
from orz_amd import _native

CONTIGUOUS = "tensors must be contiguous torch tensors"
ONE_GPU = "device-resident output needs an encoder on one GPU"
WIDE = "elements of more than 8 bytes have no byte planes here: view the tensor as a narrower dtype"
PIECE = "the piece size is a multiple of 16 elements"
OUT0 = "out must be a contiguous uint8 tensor on cuda:0"
SRC = "src must be a contiguous uint8 tensor"
OUTS0 = "outs must be contiguous tensors on cuda:0"
ELEMS = "one element size per tensor"
PIECES = "one number of pieces per tensor, unsigned 32-bit"
DIGESTS = "one digest per tensor, unsigned 32-bit"
ELEMS32 = "element sizes are unsigned 32-bit numbers"
CLOSED = "the reader is closed"


def refused(message, fn, *args, kind=ValueError, **kw):
    with pytest.raises(kind) as e:
        fn(*args, **kw)
    assert type(e.value) is kind and str(e.value) == message


def strided(dtype=torch.uint8):
    t = torch.zeros(4, 4, dtype=dtype).t()
    assert not t.is_contiguous()
    return t


OK = torch.arange(6, dtype=torch.int16)
WIDE_T = torch.zeros(3, dtype=torch.complex128)  # elements of 16 bytes
CPU_OUT = torch.zeros(64, dtype=torch.uint8)  # contiguous and uint8, but not on the GPU


@pytest.fixture
def enc():
    e = object.__new__(orz_amd.MemberEncoder)
    e._lib, e._devices, e._h = _native.load(), [0], None
    return e


@pytest.fixture
def reader():
    r = object.__new__(orz_amd.MemberReader)
    r._lib, r._h = None, 1  # (a handle that only says "open": a case that got past the checks would fail on the missing library)
    yield r
    r._h = None


def encode_calls(e):
    return [e.encode_tensors, e.encode_tensor_planes, lambda *a, **kw: e.encode_tensor_pieces(*a, piece_elems=32, **kw)]


# ---- crc32_buffers
def test_crc32_buffers_refuses_what_is_no_contiguous_tensor():
    refused(CONTIGUOUS, orz_amd.crc32_buffers, [OK, b"abc"])
    refused(CONTIGUOUS, orz_amd.crc32_buffers, [OK, None])
    refused(CONTIGUOUS, orz_amd.crc32_buffers, [strided()])
    refused(CONTIGUOUS, orz_amd.crc32_buffers, [strided(), 5], device=1)  # (wrong in two ways: one refusal for both)


def test_crc32_buffers_digests_cpu_tensors_on_the_host():
    """what gets past the checks: lengths in bytes whatever the dtype, an empty tensor, an empty list; no device is asked for"""
    ts = [OK, torch.zeros(0, dtype=torch.float32), torch.arange(5, dtype=torch.float64)]
    assert orz_amd.crc32_buffers(ts) == [zlib.crc32(t.numpy().tobytes()) for t in ts]
    assert orz_amd.crc32_buffers([]) == []
    assert orz_amd.crc32_buffers(iter([OK]), device=3) == [zlib.crc32(OK.numpy().tobytes())]


# ---- MemberEncoder.encode_tensors / encode_tensor_planes / encode_tensor_pieces
def test_the_encode_calls_refuse_an_encoder_on_several_gpus(enc):
    enc._devices = [0, 1]
    for call in encode_calls(enc):
        refused(ONE_GPU, call, [OK])
        refused(ONE_GPU, call, [])
        refused(ONE_GPU, call, [OK, b"abc"], out=CPU_OUT)  # (before the tensors and `out` are looked at)
    refused(ONE_GPU, enc.encode_tensor_pieces, [WIDE_T], 7)  # (before the element and piece sizes)


def test_the_encode_calls_refuse_what_is_no_contiguous_tensor(enc):
    for call in encode_calls(enc):
        refused(CONTIGUOUS, call, [OK, b"abc"])
        refused(CONTIGUOUS, call, [strided(torch.float32), OK])
        refused(CONTIGUOUS, call, [strided()], out=CPU_OUT)  # (before `out`)
        refused(CONTIGUOUS, call, (t for t in [OK, 3]), digests=True)
    # before the element size, and before the piece size
    refused(CONTIGUOUS, enc.encode_tensor_planes, [strided(torch.complex128)])
    refused(CONTIGUOUS, enc.encode_tensor_pieces, [strided(torch.complex128)], 7)


def test_planes_and_pieces_refuse_elements_of_more_than_8_bytes(enc):
    refused(WIDE, enc.encode_tensor_planes, [OK, WIDE_T])
    refused(WIDE, enc.encode_tensor_planes, [WIDE_T], out=CPU_OUT)  # (before `out`)
    refused(WIDE, enc.encode_tensor_pieces, [OK, WIDE_T], 32)
    refused(WIDE, enc.encode_tensor_pieces, [WIDE_T], 7)  # (before the piece size)
    refused(WIDE, enc.encode_tensor_pieces, [WIDE_T], -16, out=CPU_OUT)
    # encode_tensors takes bytes: no element size to refuse, the next refusal is `out`'s
    refused(OUT0, enc.encode_tensors, [WIDE_T], out=CPU_OUT)


def test_pieces_refuse_a_piece_size_that_is_negative_or_no_multiple_of_16(enc):
    for bad in (-16, -1, 1, 15, 24, (1 << 20) + 8):
        refused(PIECE, enc.encode_tensor_pieces, [OK], bad)
    refused(PIECE, enc.encode_tensor_pieces, [], 8)  # (also of no tensors)
    refused(PIECE, enc.encode_tensor_pieces, [OK], 8, out=CPU_OUT)  # (before `out`)
    refused(PIECE, enc.encode_tensor_pieces, [OK], 8, out=torch.zeros(4), digests=True)
    for good in (0, 16, 1 << 20):  # what passes reaches `out`'s refusal
        refused(OUT0, enc.encode_tensor_pieces, [OK], good, out=CPU_OUT)


def test_the_encode_calls_refuse_an_out_that_is_not_uint8_contiguous_and_on_the_gpu(enc):
    for call in encode_calls(enc):
        refused(OUT0, call, [OK], out=CPU_OUT)
        refused(OUT0, call, [OK], out=torch.zeros(64, dtype=torch.int8))
        refused(OUT0, call, [OK], out=strided())
        refused(OUT0, call, [], out=CPU_OUT)  # (before the answer for no tensors)
        refused(OUT0, call, [], out=CPU_OUT, digests=True)
    enc._devices = [2]
    for call in encode_calls(enc):
        refused("out must be a contiguous uint8 tensor on cuda:2", call, [OK], out=CPU_OUT)


# ---- decode_members_to_device
def test_decode_members_to_device_refuses_src_then_out():
    call = orz_amd.decode_members_to_device
    refused(SRC, call, torch.zeros(4, dtype=torch.int32))
    refused(SRC, call, strided())
    refused(SRC, call, torch.zeros(4, dtype=torch.int8), out=CPU_OUT)  # (wrong src and wrong out: src first)
    refused(SRC, call, strided(), device=1, members=[(0, 1)], out=torch.zeros(4))
    refused(OUT0, call, torch.zeros(4, dtype=torch.uint8), out=CPU_OUT)
    refused(OUT0, call, b"", out=torch.zeros(4, dtype=torch.float32))
    refused(OUT0, call, bytearray(b"abc"), out=strided(), members=[(0, 3)], offsets=True)
    refused("out must be a contiguous uint8 tensor on cuda:1", call, b"abc", device=1, out=CPU_OUT)


# ---- decode_members_into
def test_decode_members_into_refuses_src_outs_digests_in_that_order():
    call = orz_amd.decode_members_into
    refused(SRC, call, torch.zeros(4, dtype=torch.int32), [])
    refused(SRC, call, strided(), [])
    refused(SRC, call, strided(), [OK])  # (wrong src and wrong outs: src first)
    refused(SRC, call, torch.zeros(4), [], digests=[1])  # (wrong src and wrong digests)
    refused(OUTS0, call, b"", [OK])  # (a tensor on the CPU)
    refused(OUTS0, call, b"", [b"abc"])
    refused(OUTS0, call, torch.zeros(4, dtype=torch.uint8), [strided()], members=[(0, 4)])
    refused(OUTS0, call, b"", [OK], digests=[1, 2])  # (wrong outs and wrong digests: outs first)
    refused("outs must be contiguous tensors on cuda:1", call, b"", [OK], device=1)
    refused(DIGESTS, call, b"", [], digests=[1])  # (one digest too many for no tensors)
    refused(DIGESTS, call, b"", [], members=[], digests=[1 << 32, -1], stats=True)


# ---- decode_planes_into
def test_decode_planes_into_refuses_src_outs_elems_pieces_digests_in_that_order():
    call = orz_amd.decode_planes_into
    refused(SRC, call, torch.zeros(4, dtype=torch.int16), [])
    refused(SRC, call, strided(), [OK], elems=[2, 2])  # (wrong src, outs and elems: src first)
    refused(OUTS0, call, b"", [OK])
    refused(OUTS0, call, b"", [OK, 7], elems=[2])  # (wrong outs and wrong elems: outs first)
    refused(OUTS0, call, b"", [strided()], pieces=[], digests=[])
    refused("outs must be contiguous tensors on cuda:3", call, b"", [OK], device=3)
    refused(ELEMS, call, b"", [], elems=[2])
    refused(ELEMS, call, b"", [], elems=[2], pieces=[1])  # (wrong elems and wrong pieces: elems first)
    refused(ELEMS, call, b"", [], elems=[2, 4], digests=[1])  # (wrong elems and wrong digests)
    refused(PIECES, call, b"", [], pieces=[1])
    refused(PIECES, call, b"", [], elems=[], pieces=[-1])
    refused(PIECES, call, b"", [], pieces=[1 << 32], digests=[1])  # (wrong pieces and wrong digests: pieces first)
    refused(DIGESTS, call, b"", [], digests=[0])
    refused(DIGESTS, call, b"", [], elems=[], pieces=[], members=[], digests=[-1], stats=True)


# ---- MemberReader
def test_a_reader_refuses_src_before_it_opens_anything():
    refused(SRC, orz_amd.MemberReader, torch.zeros(4, dtype=torch.int32))
    refused(SRC, orz_amd.MemberReader, strided(), device=1, members=[(0, 1)], elems=[1 << 40], pieces=[-1])


def test_set_planes_refuses_element_sizes_and_pieces_out_of_range(reader):
    refused(ELEMS32, reader.set_planes, [2, -1])
    refused(ELEMS32, reader.set_planes, [1 << 32])
    refused(ELEMS32, reader.set_planes, [-4], pieces=[1, 2])  # (wrong elems and wrong pieces: elems first)
    refused(ELEMS32, reader.set_planes, [2, 1 << 32], pieces=[1, -1])
    refused(PIECES, reader.set_planes, [2, 4], pieces=[1])  # (the wrong number)
    refused(PIECES, reader.set_planes, [], pieces=[1])
    refused(PIECES, reader.set_planes, None, pieces=[1])  # (no tensors: no pieces either)
    refused(PIECES, reader.set_planes, [2, 4], pieces=[1, -1])
    refused(PIECES, reader.set_planes, [2, 4], pieces=[1 << 32, 1])
    refused(PIECES, reader.set_planes, [2], pieces=[1, 1 << 32])  # (the wrong number and out of range: one refusal for both)


def test_a_closed_reader_refuses_set_planes_first(reader):
    reader._h = None
    refused(CLOSED, reader.set_planes, [2], kind=orz_amd.OrzError)
    refused(CLOSED, reader.set_planes, [-1], kind=orz_amd.OrzError)  # (closed and wrong elems: closed first)
    refused(CLOSED, reader.set_planes, [1 << 32], pieces=[], kind=orz_amd.OrzError)
