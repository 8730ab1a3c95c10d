"""Host-side mirror of the reference's encoder interface, driving liborz_hip.so.

  cfg_for_level   src/main.rs:97-102
  LZEncoder       src/lz.rs:69-95   (new / encode / forward, one chunk per encode() call)
  encode          src/lib.rs:58-92  (Read -> Write stream encode)
  StreamEncoder / encode_bytes : reusable whole-buffer encoder (what bench.py times)
"""
import ctypes

from . import _native
from ._native import EncodeStats, LZCfg


class OrzError(RuntimeError):
    pass


class OrzDigestError(OrzError):
    """decoded bytes whose CRC-32 digest differs from the one given (ORZ_EBADMSG): `.tensor` = the first such tensor, `.expected`
    and `.computed` = its two digests"""

    def __init__(self, message, tensor, expected, computed):
        super().__init__(message)
        self.tensor, self.expected, self.computed = tensor, expected, computed


EBADMSG = -74


def _check(rc, what):
    if rc != 0:
        raise OrzError("%s failed (%d): %s" % (what, rc, _native.last_error()))


# ---- what the calls on tensors share: each check and each piece of marshalling is written once, here
def _sync(dev):
    """the library works on streams of its own: what torch queued on `dev` must be done before a call"""
    import torch

    torch.cuda.current_stream(dev).synchronize()


def _container(src, dev):
    """`src` -- a uint8 tensor on `dev` or on the CPU, or bytes-like -- as (keep, on_dev, ptr, n): n bytes at `ptr`, which `keep`
    keeps alive"""
    import torch

    if isinstance(src, torch.Tensor):
        if src.dtype != torch.uint8 or not src.is_contiguous():
            raise ValueError("src must be a contiguous uint8 tensor")
        if src.is_cuda and src.device != dev:
            raise ValueError("src lies on %s, not on %s" % (src.device, dev))
        return src, src.is_cuda, (src.data_ptr() if src.numel() else None), src.numel()
    data = bytes(src)
    keep = ctypes.create_string_buffer(data, max(len(data), 1))
    return keep, False, ctypes.cast(keep, ctypes.c_void_p), len(data)


def _member_table(members):
    """`members` -- None, or [(offset, length)] per member -- as (offs, lens, nt) of the decode calls"""
    if members is None:
        return None, None, 0
    nt = len(members)
    return (ctypes.c_size_t * max(nt, 1))(*[int(o) for o, _ in members]), (ctypes.c_size_t * max(nt, 1))(*[int(ln) for _, ln in members]), nt


def _tensor_list(tensors, device):
    """(cuda:`device`, the tensors as a list, whether they lie on it, their lengths in bytes): contiguous, all there or all on the CPU"""
    import torch

    tensors = list(tensors)
    if any(not isinstance(t, torch.Tensor) or not t.is_contiguous() for t in tensors):
        raise ValueError("tensors must be contiguous torch tensors")
    on_dev = bool(tensors) and tensors[0].is_cuda
    dev = torch.device("cuda", int(device))
    if any(t.is_cuda != on_dev or (on_dev and t.device != dev) for t in tensors):
        raise ValueError("tensors must all lie on %s or all on the CPU" % dev)
    return dev, tensors, on_dev, [t.numel() * t.element_size() for t in tensors]


def _uint8_out(out, dev):
    import torch

    if out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor on %s" % dev)


def _plane_elems(tensors):
    elems = [t.element_size() for t in tensors]
    if any(e > 8 for e in elems):
        raise ValueError("elements of more than 8 bytes have no byte planes here: view the tensor as a narrower dtype")
    return elems


def _base_list(bases, tensors, dev, on_dev, what):
    """`bases` as a list, one per tensor of `tensors` (`what`: their name in a message): None, or a contiguous tensor where they
    lie -- on `dev`, or on the CPU when on_dev is false -- with the tensor's element size and number of elements"""
    import torch

    bases = list(bases)
    if len(bases) != len(tensors):
        raise ValueError("one base (or None) per tensor: %d bases for %d %s" % (len(bases), len(tensors), what))
    for k, (b, t) in enumerate(zip(bases, tensors)):
        if b is None:
            continue
        if not isinstance(b, torch.Tensor) or not b.is_contiguous():
            raise ValueError("base %d must be a contiguous torch tensor or None" % k)
        if b.is_cuda != on_dev or (on_dev and b.device != dev):
            raise ValueError("base %d lies on %s, not where the %s lie (%s)" % (k, b.device, what, dev if on_dev else "the CPU"))
        if b.element_size() != t.element_size() or b.numel() != t.numel():
            raise ValueError("base %d has %d elements of %d bytes, its tensor %d of %d" % (k, b.numel(), b.element_size(), t.numel(), t.element_size()))
    return bases


class _Declared:
    """a tensor a reader has declared, as far as _base_list asks a tensor: its number of elements and their size"""

    def __init__(self, count, size):
        self._count, self._size = count, size

    def numel(self):
        return self._count

    def element_size(self):
        return self._size


def crc32_buffers(tensors, device=0):
    """[zlib.crc32 of each tensor's bytes] (orz_crc32_buffers): contiguous tensors of any dtype, all on cuda:`device` -- digested
    there, where they lie, in three launches and two host waits however many they are -- or all on the CPU."""
    lib = _native.load()
    dev, tensors, on_dev, lengths = _tensor_list(tensors, device)
    n = len(tensors)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[(t.data_ptr() if ln else None) for t, ln in zip(tensors, lengths)])
    lens = (ctypes.c_size_t * max(n, 1))(*lengths)
    crcs = (ctypes.c_uint32 * max(n, 1))()
    if on_dev:
        _sync(dev)
    _check(lib.orz_crc32_buffers(int(device), ptrs, lens, n, 1 if on_dev else 0, crcs), "orz_crc32_buffers")
    return [int(crcs[k]) for k in range(n)]


def crc32_combine(a, b, len_b):
    """the digest of A + B from a = that of A, b = that of B and the length of B (orz_crc32_combine; host only)"""
    a, b, len_b = int(a), int(b), int(len_b)
    if not (0 <= a < 1 << 32 and 0 <= b < 1 << 32 and 0 <= len_b < 1 << 64):
        raise ValueError("digests are unsigned 32-bit numbers, the length an unsigned 64-bit one")
    return int(_native.load().orz_crc32_combine(a, b, len_b))


def _digest_array(digests, nd):
    digests = [int(c) for c in digests]
    if len(digests) != nd or any(c < 0 or c >= 1 << 32 for c in digests):
        raise ValueError("one digest per tensor, unsigned 32-bit")
    return digests, (ctypes.c_uint32 * max(nd, 1))(*digests)


def _check_verified(rc, digests, out_crcs, name="orz_decode_tensors_verified"):
    """raises what orz_decode_tensors_verified (or the call `name` with digests) answered"""
    if rc == EBADMSG:
        j = next((k for k, c in enumerate(digests) if out_crcs[k] != c), 0)
        raise OrzDigestError("%s failed (%d): %s" % (name, rc, _native.last_error()), j, digests[j], int(out_crcs[j]))
    _check(rc, name)


def cfg_for_level(level):
    """level -> LZCfg exactly as `orz encode -l` maps it (src/main.rs:97-102); other levels raise."""
    cfg = LZCfg()
    rc = _native.load().orz_lzcfg_from_level(int(level), ctypes.byref(cfg))
    if rc != 0:
        raise ValueError("invalid level")
    return cfg


def stream_bound(nbytes):
    """device bytes that always hold the stream of `nbytes` input bytes (orz_stream_bound)"""
    return int(_native.load().orz_stream_bound(int(nbytes)))


class OrzBuffer:
    """A stream the library returned (orz_stream_encode's own buffer), held without copying; released with orz_free."""

    def __init__(self, lib, ptr, n):
        self._lib, self._ptr, self._n = lib, ptr, int(n)

    def __len__(self):
        return self._n

    def __bytes__(self):
        return ctypes.string_at(self._ptr, self._n)

    def view(self):
        """memoryview over the buffer (valid while this object lives)"""
        return memoryview((ctypes.c_uint8 * self._n).from_address(ctypes.addressof(self._ptr.contents))).cast("B") if self._n else memoryview(b"")

    def close(self):
        if self._ptr is not None:
            self._lib.orz_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StreamEncoder:
    """One orz stream encoder bound to one GPU; reusable across inputs."""

    def __init__(self, device=0, level=1, cfg=None, mode=None, tile_bytes=0, rounds=0):
        """mode: "fast" (GPU-native parse: reference-decodable, size within +-0.5 %), "exact" (the reference's
        parse item for item: byte-identical stream) or None = the library default (fast unless ORZ_MODE=exact)."""
        self._lib = _native.load()
        self.cfg = cfg if cfg is not None else cfg_for_level(level)
        self._h = self._lib.orz_stream_new(int(device), ctypes.byref(self.cfg))
        if not self._h:
            raise OrzError("orz_stream_new failed: " + _native.last_error())
        if mode is not None or tile_bytes or rounds:
            if mode is None:
                mode = "fast" if self.config()["mode"] == 1 else "exact"
            if mode not in ("fast", "exact"):
                raise ValueError("mode must be 'fast' or 'exact'")
            _check(self._lib.orz_stream_set_mode(self._h, 1 if mode == "fast" else 0, int(tile_bytes), int(rounds)),
                   "orz_stream_set_mode")

    def set_mode(self, mode, tile_bytes=0, rounds=0):
        """switch the parse mode / fast-mode schedule of this encoder (rebuilds its device state)"""
        if mode not in ("fast", "exact"):
            raise ValueError("mode must be 'fast' or 'exact'")
        _check(self._lib.orz_stream_set_mode(self._h, 1 if mode == "fast" else 0, int(tile_bytes), int(rounds)), "orz_stream_set_mode")

    def config(self):
        """What the encoder runs with (orz_stream_get_config)."""
        c = _native.StreamConfig()
        _check(self._lib.orz_stream_get_config(self._h, ctypes.byref(c)), "orz_stream_get_config")
        return c.as_dict()

    def set_profile(self, on=True):
        """bracket the kernels inside the round loop too (no hipGraph replay then): for the roofline leg only"""
        _check(self._lib.orz_stream_set_profile(self._h, 1 if on else 0), "orz_stream_set_profile")

    def kernel_times(self):
        """[(ms, launches)] x 4 of the last encode(stats=True): parse kernel, symbol ranking, candidate tables, path maps"""
        ms = (ctypes.c_double * 4)()
        n = (ctypes.c_uint64 * 4)()
        _check(self._lib.orz_stream_get_kernel_times(self._h, ms, n), "orz_stream_get_kernel_times")
        return [(ms[i], n[i]) for i in range(4)]

    def kernel_table(self):
        """[(name, ms, launches)] of EVERY kernel of the last encode(stats=True) made in profile mode, largest first"""
        n = self._lib.orz_stream_get_kernel_table(self._h, None, 0)
        if n <= 0:
            return []
        rows = (_native.KernelRow * n)()
        self._lib.orz_stream_get_kernel_table(self._h, ctypes.cast(rows, ctypes.c_void_p), n)
        return [(r.name.decode(), r.ms, int(r.launches)) for r in rows]

    def set_tuning(self, seg_bytes=0, window_segs=0):
        _check(self._lib.orz_stream_set_tuning(self._h, seg_bytes, window_segs), "orz_stream_set_tuning")

    def _encode(self, ptr, n, on_device, want_stats, raw=False):
        dst = ctypes.POINTER(ctypes.c_uint8)()
        dlen = ctypes.c_size_t()
        st = EncodeStats()
        rc = self._lib.orz_stream_encode(
            self._h, ptr, n, 1 if on_device else 0, ctypes.byref(dst), ctypes.byref(dlen),
            ctypes.byref(st) if want_stats else None,
        )
        _check(rc, "orz_stream_encode")
        if raw:  # the library's buffer itself, no copy (released with the object)
            return OrzBuffer(self._lib, dst, dlen.value), (st.as_dict() if want_stats else None)
        try:
            out = ctypes.string_at(dst, dlen.value)
        finally:
            self._lib.orz_free(dst)
        return out, (st.as_dict() if want_stats else None)

    def encode(self, data, stats=False):
        """bytes -> orz stream (same bytes `orz encode` writes)."""
        data = bytes(data)
        buf = ctypes.create_string_buffer(data, len(data)) if data else ctypes.create_string_buffer(1)
        out, st = self._encode(ctypes.cast(buf, ctypes.c_void_p), len(data), False, stats)
        return (out, st) if stats else out

    def encode_device(self, dev_ptr, nbytes, stats=False, raw=False):
        """Encode `nbytes` already resident in this GPU's HBM at address `dev_ptr`.  raw=True returns the library's own
        host buffer (an OrzBuffer: len(), bytes(), .view() -> memoryview; it does not implement the buffer protocol itself)
        instead of a bytes copy of it."""
        out, st = self._encode(ctypes.c_void_p(int(dev_ptr)), int(nbytes), True, stats, raw)
        return (out, st) if stats else out

    def encode_to_device(self, src_ptr, nbytes, dst_ptr, dst_cap, src_on_device=True, stats=False):
        """Encode into DEVICE memory the caller owns (orz_stream_encode_to_device): the finished stream -- framed on the
        device -- is left at `dst_ptr` (`dst_cap` bytes on this encoder's GPU; `stream_bound(nbytes)` always suffices).
        Returns its length (and the stats dict).  What the multi-GPU gather sends from where it lies."""
        dlen = ctypes.c_size_t()
        st = EncodeStats()
        rc = self._lib.orz_stream_encode_to_device(self._h, ctypes.c_void_p(int(src_ptr)), int(nbytes), 1 if src_on_device else 0,
                                                   ctypes.c_void_p(int(dst_ptr)), int(dst_cap), ctypes.byref(dlen),
                                                   ctypes.byref(st) if stats else None)
        _check(rc, "orz_stream_encode_to_device")
        return (dlen.value, st.as_dict()) if stats else dlen.value

    def set_item_trace(self, on=True):
        _check(self._lib.orz_stream_set_item_trace(self._h, 1 if on else 0), "orz_stream_set_item_trace")

    def item_trace(self):
        """numpy structured array of the items of the last encode() (needs set_item_trace(True))."""
        import numpy as np

        n = self._lib.orz_stream_get_item_trace(self._h, None, 0)
        buf = (_native.Item * max(n, 1))()
        self._lib.orz_stream_get_item_trace(self._h, buf, n)
        dt = np.dtype([("block", "<u4"), ("pos", "<u4"), ("symbol", "<u2"), ("rank", "<u2"), ("ctx", "<u2"),
                       ("robits", "<u2"), ("unlikely", "u1"), ("enc_len", "u1"), ("after_literal", "u1"), ("match_len", "u1"),
                       ("src", "<u4")])
        return np.frombuffer(buf, dtype=dt, count=n).copy()

    PATCH_FIELDS = {"TYPE": 0, "LEN": 1, "SRC": 2, "SYM": 3, "CTX": 4, "AL": 5, "ENC": 6, "ROB": 7, "UNL": 8, "ORD": 9, "LMV": 10}

    def set_item_patches(self, patches):
        """FOR TESTS of the validity gate (orz_stream_set_item_patches): [(block, pos, field, value)], field a name of PATCH_FIELDS
        or its number, overwrite those fields of those items in the next encode() only.  An empty list clears."""
        import numpy as np

        arr = np.array([(b, p, self.PATCH_FIELDS.get(f, f), v) for b, p, f, v in patches], dtype="<u4").reshape(-1, 4)
        _check(self._lib.orz_stream_set_item_patches(self._h, arr.ctypes.data if len(arr) else None, len(arr)),
               "orz_stream_set_item_patches")

    # the tables orz_stream_fast_tables hands out, and what they hold
    FAST_TABLES = {"hpos": "<u4", "wsnap": "u1", "epos": "<u4", "keys": "<u4", "idx": "<u4", "runstart": "<u4", "rlen": "u1", "vbits": "<u8",
                   "stext": "<u8", "cl": "<u8", "ccnt": "<u4", "rows": "u1", "rdist": "<u8", "kpos": "<u4", "kkeys": "<u4", "krun": "<u4",
                   "kw": "<u2", "wmask": "<u8", "kmeta": "<u2", "hcm": "<u4", "hpre": "<u4"}

    def arm_fast_tables(self, block):
        """FOR TESTS: the next encode() keeps the static tables of its `block`-th encode_block call (None: disarm)."""
        rc = self._lib.orz_stream_fast_tables(self._h, -1 if block is None else int(block), None, None, 0)
        if rc < 0:
            _check(rc, "orz_stream_fast_tables")

    def fast_tables(self):
        """FOR TESTS: the tables of the captured block: {name: numpy array} plus the scalars n, nhist, nent, nk, K, stream_off."""
        import numpy as np

        def get(name, dtype):
            size = self._lib.orz_stream_fast_tables(self._h, 0, name.encode(), None, 0)
            if size < 0:
                _check(size, "orz_stream_fast_tables")
            buf = np.empty(size, dtype=np.uint8)
            self._lib.orz_stream_fast_tables(self._h, 0, name.encode(), buf.ctypes.data, size)
            return buf.view(dtype)

        sc = get("scalars", "<u8")
        out = {k: int(sc[i]) for i, k in enumerate(("n", "nhist", "nent", "nk", "K", "stream_off", "block", "new_at"))}
        for name, dtype in self.FAST_TABLES.items():
            out[name] = get(name, dtype)
        return out

    def arm_repair_probe(self, block, ty=None, nl=None):
        """FOR TESTS: the next encode() records the repair stage of its `block`-th encode_block call pass by pass (None: disarm);
        ty / nl (uint8 arrays, one entry per position of that block): a decision field that replaces the rounds' there."""
        import numpy as np

        if ty is None and nl is None:
            rc = self._lib.orz_stream_arm_repair_probe(self._h, -1 if block is None else int(block), None, None, 0)
        else:
            ty = np.ascontiguousarray(ty, dtype=np.uint8)
            nl = np.ascontiguousarray(nl, dtype=np.uint8)
            if ty.shape != nl.shape or ty.ndim != 1:
                raise ValueError("ty and nl must be one-dimensional and of the same size")
            rc = self._lib.orz_stream_arm_repair_probe(self._h, int(block), ty.ctypes.data, nl.ctypes.data, len(ty))
        _check(rc, "orz_stream_arm_repair_probe")

    def repair_probe(self, name, dtype="u1"):
        """FOR TESTS: one table of the probed block (orz_stream_repair_probe) as a numpy array; the names are in include/orz_hip.h"""
        import numpy as np

        size = self._lib.orz_stream_repair_probe(self._h, name.encode(), None, 0)
        if size < 0:
            _check(size, "orz_stream_repair_probe")
        buf = np.empty(size, dtype=np.uint8)
        self._lib.orz_stream_repair_probe(self._h, name.encode(), buf.ctypes.data, size)
        return buf.view(dtype)

    def close(self):
        if self._h:
            self._lib.orz_stream_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def encode_bytes(data, level=1, device=0):
    enc = StreamEncoder(device=device, level=level)
    try:
        return enc.encode(data)
    finally:
        enc.close()


def encode(src, dst, cfg, progress=None, device=0):
    """orz::encode (src/lib.rs:58-92): read everything from file-like `src`, write the stream to `dst`.

    `progress(is_finish, in_bytes, out_bytes)` mirrors ProgressLogger (src/progress.rs:9-13).
    Returns (bytes_read, bytes_written) like the reference's CountRead/CountWrite totals."""
    lib = _native.load()
    counts = [0, 0]

    def _rd(_ctx, buf, cap):
        try:
            chunk = src.read(cap)
        except Exception:
            return -1
        n = len(chunk)
        if n:
            ctypes.memmove(buf, chunk, n)
            counts[0] += n
        return n

    def _wr(_ctx, buf, n):
        try:
            dst.write(ctypes.string_at(buf, n))
        except Exception:
            return -1
        counts[1] += n
        return 0

    def _pg(_ctx, fin, a, b):
        if progress:
            progress(bool(fin), a, b)

    rd, wr, pg = _native.READ_FN(_rd), _native.WRITE_FN(_wr), _native.PROGRESS_FN(_pg)
    _check(lib.orz_encode(rd, None, wr, None, ctypes.byref(cfg), pg, None, int(device)), "orz_encode")
    return tuple(counts)


class MemberEncoder:
    """`jobs` stream encoders on one GPU; encode() cuts the input into members of `member_bytes`, encodes
    them concurrently (one host thread per encoder inside the library) and returns the members' streams
    concatenated in order -- each a complete orz stream the reference decoder reads."""

    def __init__(self, device=0, level=1, jobs=4, devices=None):
        """devices: list of HIP ordinals for a multi-GPU job (`jobs` encoders on each); default = [device]"""
        self._lib = _native.load()
        self.cfg = cfg_for_level(level)
        devs = [int(device)] if devices is None else [int(d) for d in devices]
        arr = (ctypes.c_int * len(devs))(*devs)
        self._devices = devs
        self._h = self._lib.orz_members_new_multi(arr, len(devs), ctypes.byref(self.cfg), int(jobs))
        if not self._h:
            raise OrzError("orz_members_new_multi failed: " + _native.last_error())

    def _run(self, ptr, n, on_device, member_bytes):
        dst = ctypes.POINTER(ctypes.c_uint8)()
        dlen, nm = ctypes.c_size_t(), ctypes.c_size_t()
        rc = self._lib.orz_members_encode(self._h, ptr, n, 1 if on_device else 0, int(member_bytes), ctypes.byref(dst),
                                          ctypes.byref(dlen), ctypes.byref(nm))
        _check(rc, "orz_members_encode")
        try:
            return ctypes.string_at(dst, dlen.value), nm.value
        finally:
            self._lib.orz_free(dst)

    def encode(self, data, member_bytes=1 << 26):
        """member_bytes: 64 MiB by default -- a member starts with empty rings and a flat symbol order, and that cold start
        costs about 1.5 % of the size at 16 MiB members, a quarter of that at 64 MiB.  Members larger than one
        block (16 MiB) decode with the reference decoder, with `decode_members` (host) and with the device decoder
        (`decode_members_device`: its window slides as a counter, round 4)."""
        data = bytes(data)  # (no copy when it is `bytes` already; the library reads the object's own buffer)
        ptr = ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p) if data else ctypes.cast(ctypes.create_string_buffer(1), ctypes.c_void_p)
        return self._run(ptr, len(data), False, member_bytes)

    def encode_device(self, dev_ptr, nbytes, member_bytes=1 << 26):
        return self._run(ctypes.c_void_p(int(dev_ptr)), int(nbytes), True, member_bytes)

    def encode_to_device(self, src_ptr, nbytes, dst_ptr, dst_cap, member_bytes=1 << 26, src_on_device=True):
        """The members' streams left in DEVICE memory the caller owns (orz_members_encode_to_device; one GPU): returns
        [(offset, length)] per member, in member order, into the buffer at `dst_ptr`."""
        nm = 1 if nbytes == 0 else (int(nbytes) + int(member_bytes) - 1) // int(member_bytes)
        offs, lens = (ctypes.c_size_t * nm)(), (ctypes.c_size_t * nm)()
        got = ctypes.c_size_t()
        rc = self._lib.orz_members_encode_to_device(self._h, ctypes.c_void_p(int(src_ptr)), int(nbytes), 1 if src_on_device else 0,
                                                    int(member_bytes), ctypes.c_void_p(int(dst_ptr)), int(dst_cap), offs, lens,
                                                    ctypes.byref(got))
        _check(rc, "orz_members_encode_to_device")
        return [(offs[k], lens[k]) for k in range(got.value)]

    def bound_segments(self, lengths):
        """device bytes that always hold the members of segments of these lengths (orz_members_bound_segments)"""
        n = len(lengths)
        arr = (ctypes.c_size_t * max(n, 1))(*[int(x) for x in lengths])
        return int(self._lib.orz_members_bound_segments(arr, n))

    @staticmethod
    def _segment_arrays(ptrs, lengths):
        n = len(ptrs)
        return (ctypes.c_void_p * max(n, 1))(*[p or None for p in ptrs]), (ctypes.c_size_t * max(n, 1))(*lengths), n

    def encode_segments(self, segments):
        """One member per bytes-like object of `segments`, in that order (orz_members_encode_segments): no boundary falls inside
        a segment and none is packed with another.  Returns (the members' streams concatenated, [each stream's length])."""
        keep = [bytes(b) for b in segments]  # (no copy of what is `bytes` already; the library reads the objects' own buffers)
        ptrs, lengths, n = self._segment_arrays([ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value if b else None for b in keep],
                                                [len(b) for b in keep])
        dst = ctypes.POINTER(ctypes.c_uint8)()
        dlen = ctypes.c_size_t()
        lens = (ctypes.c_size_t * max(n, 1))()
        rc = self._lib.orz_members_encode_segments(self._h, ptrs, lengths, n, 0, ctypes.byref(dst), ctypes.byref(dlen), lens)
        _check(rc, "orz_members_encode_segments")
        del keep
        try:
            return ctypes.string_at(dst, dlen.value), [lens[k] for k in range(n)]
        finally:
            self._lib.orz_free(dst)

    def encode_segments_to_device(self, seg_ptrs, seg_lens, dst_ptr, dst_cap, src_on_device=True):
        """orz_members_encode_segments_to_device on raw addresses: segment k is the seg_lens[k] bytes at seg_ptrs[k]; returns
        [(offset, length)] per member, in segment order, into the buffer at `dst_ptr`."""
        ptrs, lengths, n = self._segment_arrays([int(p) for p in seg_ptrs], [int(x) for x in seg_lens])
        offs, lens = (ctypes.c_size_t * max(n, 1))(), (ctypes.c_size_t * max(n, 1))()
        rc = self._lib.orz_members_encode_segments_to_device(self._h, ptrs, lengths, n, 1 if src_on_device else 0,
                                                             ctypes.c_void_p(int(dst_ptr)), int(dst_cap), offs, lens)
        _check(rc, "orz_members_encode_segments_to_device")
        return [(offs[k], lens[k]) for k in range(n)]

    def _digests_of(self, tensors, on_dev):
        """the digests of the INPUT tensors, taken before the encode: they vouch for the source, not for anything the encoder touched"""
        return crc32_buffers(tensors, device=self._devices[0]) if tensors else []

    def _checked_tensors(self, tensors):
        if len(self._devices) != 1:
            raise ValueError("device-resident output needs an encoder on one GPU")
        return _tensor_list(tensors, self._devices[0])

    def _encode_tensor_list(self, checked, out, digests, n_extra, bound, encode):
        """What the three encode_tensor* calls do behind their own checks.  `checked`: what _checked_tensors returned; `bound(lengths)`:
        the bytes of a container that always suffices; `encode(ptrs, lengths, dst_ptr, dst_cap, src_on_device)`: the call on raw
        addresses, which returns (members, and `n_extra` lists more).  Returns (container, what `encode` returned[, digests])."""
        import torch

        dev, tensors, on_dev, lengths = checked
        trim = out is None
        if trim:
            out = torch.empty(bound(lengths), dtype=torch.uint8, device=dev)
        else:
            _uint8_out(out, dev)
        if not tensors:
            return ((out[:0] if trim else out),) + tuple([] for _ in range(1 + n_extra)) + (([],) if digests else ())
        crcs = (self._digests_of(tensors, on_dev),) if digests else ()
        _sync(dev)
        res = encode([t.data_ptr() if n else 0 for t, n in zip(tensors, lengths)], lengths, out.data_ptr(), out.numel(), on_dev)
        return ((out[: max(o + ln for o, ln in res[0])] if trim else out),) + tuple(res) + crcs

    def encode_tensors(self, tensors, out=None, digests=False):
        """One member per tensor of `tensors` (contiguous, any dtype, encoded as their bytes; all on this encoder's GPU or all on
        the CPU), left in device memory: returns (container, members).  `container`: a uint8 tensor on the GPU -- `out` when given,
        else one of bound_segments() bytes trimmed to the furthest byte used; `members`: [(offset, length)] per tensor, what
        MemberReader, decode_members_to_device and decode_members_into take as `members=`.  digests=True: the tuple gains a last
        element, [CRC-32 of each input tensor's bytes] (crc32_buffers on the inputs, before the encode): what
        decode_members_into takes as `digests=`."""
        return self._encode_tensor_list(self._checked_tensors(tensors), out, digests, 0, self.bound_segments,
                                        lambda *a: (self.encode_segments_to_device(*a),))

    def bound_planes(self, lengths, elems):
        """device bytes that always hold the plane members of segments of these lengths and element sizes
        (orz_members_bound_planes).  About 1 MiB a member for small segments: with many small tensors pass an `out` of your own."""
        n = len(lengths)
        if len(elems) != n:
            raise ValueError("one element size per length")
        arr = (ctypes.c_size_t * max(n, 1))(*[int(x) for x in lengths])
        el = (ctypes.c_uint32 * max(n, 1))(*[int(e) for e in elems])
        return int(self._lib.orz_members_bound_planes(arr, el, n))

    def encode_planes_to_device(self, seg_ptrs, seg_lens, seg_elems, dst_ptr, dst_cap, src_on_device=True):
        """orz_members_encode_planes_to_device on raw addresses: segment k is the seg_lens[k] bytes at seg_ptrs[k], elements of
        seg_elems[k] bytes (1, 2, 4 or 8); it becomes seg_elems[k] members, one per byte plane, plane 0 first.  Returns
        [(offset, length)] per member, segment by segment, into the buffer at `dst_ptr`."""
        if len(seg_elems) != len(seg_ptrs) or len(seg_lens) != len(seg_ptrs):
            raise ValueError("one length and one element size per segment")
        ptrs, lengths, n = self._segment_arrays([int(p) for p in seg_ptrs], [int(x) for x in seg_lens])
        el = (ctypes.c_uint32 * max(n, 1))(*[int(e) for e in seg_elems])
        nm = sum(int(e) for e in seg_elems if 0 < int(e) <= 8)
        offs, lens = (ctypes.c_size_t * max(nm, 1))(), (ctypes.c_size_t * max(nm, 1))()
        rc = self._lib.orz_members_encode_planes_to_device(self._h, ptrs, lengths, el, n, 1 if src_on_device else 0,
                                                           ctypes.c_void_p(int(dst_ptr)), int(dst_cap), offs, lens)
        _check(rc, "orz_members_encode_planes_to_device")
        return [(offs[k], lens[k]) for k in range(nm)]

    def encode_tensor_planes(self, tensors, out=None, digests=False):
        """Each tensor of `tensors` as the byte planes of its elements, a member per plane (plane p = byte p of every element):
        tensor k contributes element_size() consecutive members, plane 0 first.  For typed data -- weights shrink by about a
        tenth against encode_tensors, ids and counts severalfold -- and a tensor's planes decode side by side.  Tensors, devices
        and `out` as for encode_tensors; an element size above 8 raises ValueError.  Returns (container, members, elems):
        `members` [(offset, length)] per plane, `elems` [element size of each tensor]: what decode_planes_into takes.
        digests=True: the tuple gains a last element, [CRC-32 of each input tensor's bytes], as for encode_tensors."""
        checked = self._checked_tensors(tensors)
        elems = _plane_elems(checked[1])
        return self._encode_tensor_list(checked, out, digests, 1, lambda lengths: self.bound_planes(lengths, elems),
                                        lambda ptrs, lengths, *to: (self.encode_planes_to_device(ptrs, lengths, elems, *to), elems))

    def bound_planes_pieces(self, lengths, elems, piece_elems):
        """(device bytes that always hold the members, the number of members) of segments of these lengths and element sizes with
        their planes cut into pieces of `piece_elems` elements (orz_members_bound_planes_pieces)"""
        n = len(lengths)
        if len(elems) != n:
            raise ValueError("one element size per length")
        arr = (ctypes.c_size_t * max(n, 1))(*[int(x) for x in lengths])
        el = (ctypes.c_uint32 * max(n, 1))(*[int(e) for e in elems])
        nm = ctypes.c_size_t()
        return int(self._lib.orz_members_bound_planes_pieces(arr, el, n, int(piece_elems), ctypes.byref(nm))), nm.value

    def encode_planes_pieces_to_device(self, seg_ptrs, seg_lens, seg_elems, piece_elems, dst_ptr, dst_cap, src_on_device=True):
        """orz_members_encode_planes_pieces_to_device on raw addresses: encode_planes_to_device with every plane cut into pieces
        of `piece_elems` elements (a multiple of 16; 0 = never), a member per piece, plane-major.  Returns ([(offset, length)]
        per member, [pieces per plane of each segment])."""
        if len(seg_elems) != len(seg_ptrs) or len(seg_lens) != len(seg_ptrs):
            raise ValueError("one length and one element size per segment")
        piece_elems = int(piece_elems)
        if piece_elems < 0 or piece_elems >= 1 << 64:
            raise ValueError("the piece size is an unsigned 64-bit number")
        ptrs, lengths, n = self._segment_arrays([int(p) for p in seg_ptrs], [int(x) for x in seg_lens])
        el = (ctypes.c_uint32 * max(n, 1))(*[int(e) for e in seg_elems])
        nm = self.bound_planes_pieces([int(x) for x in seg_lens], [int(e) if 0 < int(e) <= 8 else 0 for e in seg_elems], piece_elems)[1]
        offs, lens = (ctypes.c_size_t * max(nm, 1))(), (ctypes.c_size_t * max(nm, 1))()
        pieces = (ctypes.c_size_t * max(n, 1))()
        rc = self._lib.orz_members_encode_planes_pieces_to_device(self._h, ptrs, lengths, el, n, piece_elems, 1 if src_on_device else 0,
                                                                  ctypes.c_void_p(int(dst_ptr)), int(dst_cap), offs, lens, pieces)
        _check(rc, "orz_members_encode_planes_pieces_to_device")
        pieces = [pieces[k] for k in range(n)]
        return [(offs[k], lens[k]) for k in range(sum(int(e) * q for e, q in zip(seg_elems, pieces)))], pieces

    def encode_tensor_pieces(self, tensors, piece_elems, out=None, digests=False):
        """encode_tensor_planes with every plane cut into pieces of `piece_elems` elements (a multiple of 16), a member per piece:
        tensor k contributes element_size() x Q consecutive members, Q = ceil(numel / piece_elems), plane 0's pieces first.  A
        member decodes on one lane, so pieces are what lets ONE large tensor decode in parallel and a read of its last rows skip
        what lies in front of them; each piece restarts the model and costs an encoder pass, so it costs size and encode time.
        Measured: 2^18 elements a piece is a good default -- a 4 Mi-element bf16 weight decodes in a fourteenth of the
        time for 0.5 % of size and 1.1 x the encode time (ids: 2 %, 1.7 x); 2^16 where latency matters more (1.6 to 5.7 % of
        size, 1.8 to 2.9 x the encode time); 2^20 costs nothing and takes a quarter of the time.  piece_elems == 0, or at least a tensor's elements: that tensor's planes stay whole.
        Returns (container, members, elems, pieces): `pieces` [pieces per plane of each tensor], what decode_planes_into and
        MemberReader take beside `elems`.  digests=True: the tuple gains a last element, [CRC-32 of each input tensor's bytes],
        as for encode_tensors: a tensor's digest is the same however it is cut."""
        checked = self._checked_tensors(tensors)
        elems = _plane_elems(checked[1])
        piece_elems = int(piece_elems)
        if piece_elems < 0 or piece_elems % 16:
            raise ValueError("the piece size is a multiple of 16 elements")

        def encode(ptrs, lengths, *to):
            members, pieces = self.encode_planes_pieces_to_device(ptrs, lengths, elems, piece_elems, *to)
            return members, elems, pieces

        return self._encode_tensor_list(checked, out, digests, 2, lambda lengths: self.bound_planes_pieces(lengths, elems, piece_elems)[0], encode)

    def encode_deltas_to_device(self, seg_ptrs, base_ptrs, seg_lens, seg_elems, piece_elems, dst_ptr, dst_cap, src_on_device=True):
        """orz_members_encode_deltas_to_device on raw addresses: encode_planes_pieces_to_device of segment XOR base, base k being
        the seg_lens[k] bytes at base_ptrs[k] (0 or None: no base), resident where the segments are.  Returns what that call returns."""
        if len(seg_elems) != len(seg_ptrs) or len(seg_lens) != len(seg_ptrs) or len(base_ptrs) != len(seg_ptrs):
            raise ValueError("one base, one length and one element size per segment")
        piece_elems = int(piece_elems)
        if piece_elems < 0 or piece_elems >= 1 << 64:
            raise ValueError("the piece size is an unsigned 64-bit number")
        ptrs, lengths, n = self._segment_arrays([int(p) for p in seg_ptrs], [int(x) for x in seg_lens])
        bases = (ctypes.c_void_p * max(n, 1))(*[int(p) if p else None for p in base_ptrs])
        el = (ctypes.c_uint32 * max(n, 1))(*[int(e) for e in seg_elems])
        nm = self.bound_planes_pieces([int(x) for x in seg_lens], [int(e) if 0 < int(e) <= 8 else 0 for e in seg_elems], piece_elems)[1]
        offs, lens = (ctypes.c_size_t * max(nm, 1))(), (ctypes.c_size_t * max(nm, 1))()
        pieces = (ctypes.c_size_t * max(n, 1))()
        rc = self._lib.orz_members_encode_deltas_to_device(self._h, ptrs, bases, lengths, el, n, piece_elems, 1 if src_on_device else 0,
                                                           ctypes.c_void_p(int(dst_ptr)), int(dst_cap), offs, lens, pieces)
        _check(rc, "orz_members_encode_deltas_to_device")
        pieces = [pieces[k] for k in range(n)]
        return [(offs[k], lens[k]) for k in range(sum(int(e) * q for e, q in zip(seg_elems, pieces)))], pieces

    def encode_tensor_deltas(self, tensors, bases, piece_elems=0, out=None, digests=False):
        """encode_tensor_pieces of `tensors[k]` XOR `bases[k]`, bit pattern by bit pattern, the XOR made on the GPU on the way into
        the planes (orz_members_encode_deltas_to_device): for a tensor whose reader already holds an almost equal one -- the
        previous step of a run, the base model of a fine-tune.  Measured: the steps of a bf16 run come to 0.12 to 0.5
        of the tensor's size where plain planes come to 0.70; a tensor equal to its base costs almost nothing.  `bases[k]`: None
        (tensor k is encoded as encode_tensor_pieces encodes it) or a contiguous tensor where the tensors are (all on this
        encoder's GPU or all on the CPU) with tensor k's element size and number of elements; anything else raises ValueError.
        Neither is written.  piece_elems, `out` and the members' layout as for encode_tensor_pieces (0: planes stay whole).
        Returns (container, members, elems, pieces): what decode_planes_into takes WITH THE SAME `bases=`; nothing in the container
        says which tensors are deltas, or of what: that travels beside it, like elems and pieces.  digests=True: the tuple gains
        [CRC-32 of each INPUT tensor's bytes], not of the deltas: decode_planes_into(bases=, digests=) holds the restored tensors
        to them, so a delta applied to another base raises OrzDigestError.
        MemberReader(..., bases=) reads element ranges of this container RESTORED, the XOR made in the read's own launch; a reader
        that has not been told the bases returns the DELTA's elements, and its read_tensor(..., digest=) of a tensor that has a
        base raises.
        CHAINS: the deltas of consecutive steps, each against the step before and all with the same piece_elems, are the links of
        a chain: join_links puts them (and a keyframe, if any) into one container, and decode_planes_into(..., links=K) restores
        the last step in ONE decode and ONE merge launch, with the host waits of one call and digests of the last step alone.
        The order of the links does not matter; staging memory is K times the tensors' bytes, freed before the call returns;
        a reader on a chain container still sees single links."""
        checked = self._checked_tensors(tensors)
        dev, tensors, on_dev, lengths = checked
        elems = _plane_elems(tensors)
        piece_elems = int(piece_elems)
        if piece_elems < 0 or piece_elems % 16:
            raise ValueError("the piece size is a multiple of 16 elements")
        bases = _base_list(bases, tensors, dev, on_dev, "tensors")  # (kept alive until the call returns)

        def encode(ptrs, lengths, *to):
            base_ptrs = [b.data_ptr() if b is not None and n else 0 for b, n in zip(bases, lengths)]
            members, pieces = self.encode_deltas_to_device(ptrs, base_ptrs, lengths, elems, piece_elems, *to)
            return members, elems, pieces

        return self._encode_tensor_list(checked, out, digests, 2, lambda lengths: self.bound_planes_pieces(lengths, elems, piece_elems)[0], encode)

    def close(self):
        if self._h:
            self._lib.orz_members_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_members(container):
    """decode every stream of a concatenation of orz streams -> (bytes, n_members)"""
    lib = _native.load()
    container = bytes(container)
    dst = ctypes.POINTER(ctypes.c_uint8)()
    n, nm = ctypes.c_size_t(), ctypes.c_size_t()
    buf = ctypes.create_string_buffer(container, len(container)) if container else ctypes.create_string_buffer(1)
    rc = lib.orz_decode_members_mem(ctypes.cast(buf, ctypes.c_void_p), len(container), ctypes.byref(dst), ctypes.byref(n),
                                    ctypes.byref(nm))
    _check(rc, "orz_decode_members_mem")
    try:
        return ctypes.string_at(dst, n.value), nm.value
    finally:
        lib.orz_free(dst)


def decode_members_device(container, device=0, stats=False):
    """decode every member of a concatenation of orz streams ON THE GPU (one member per wavefront; members of any number
    of blocks below 4 GiB -- the window slides as a counter, round 4) -> (bytes, n_members[, stats dict]).  Same bytes as
    `decode_members`."""
    lib = _native.load()
    container = bytes(container)
    dst = ctypes.POINTER(ctypes.c_uint8)()
    n, nm = ctypes.c_size_t(), ctypes.c_size_t()
    st = _native.DecodeStats()
    buf = ctypes.create_string_buffer(container, len(container)) if container else ctypes.create_string_buffer(1)
    rc = lib.orz_decode_members_device(device, ctypes.cast(buf, ctypes.c_void_p), len(container), ctypes.byref(dst),
                                       ctypes.byref(n), ctypes.byref(nm), ctypes.byref(st))
    _check(rc, "orz_decode_members_device")
    try:
        out = ctypes.string_at(dst, n.value)
    finally:
        lib.orz_free(dst)
    return (out, nm.value, st.as_dict()) if stats else (out, nm.value)


def decode_members_to_device(src, device=0, members=None, out=None, offsets=False, stats=False):
    """decode members ON THE GPU from device (or host) memory into device memory (orz_decode_members_to_device): the framing is
    indexed on the GPU, nothing passes through the host.  `src`: a uint8 torch tensor on cuda:`device` or on the CPU, or
    bytes-like.  `members`: None = `src` is one concatenation of members; else [(offset, length)] per member in member order, in
    any order and with gaps in `src` (what MemberEncoder.encode_to_device returns).  `out`: a uint8 tensor on the device to
    decode into (its first dst_len bytes are written, nothing else); by default one of the exact size is allocated.  Returns
    (tensor of dst_len bytes on the device, n_members[, offsets: where each member's bytes start][, stats dict])."""
    import torch

    lib = _native.load()
    dev = torch.device("cuda", int(device))
    keep, on_dev, ptr, n = _container(src, dev)
    if out is not None:
        _uint8_out(out, dev)
    offs, lens, nt = _member_table(members)
    _sync(dev)
    dlen, nm = ctypes.c_size_t(), ctypes.c_size_t()

    def call(dst, cap, oo, st):
        rc = lib.orz_decode_members_to_device(int(device), ptr, n, 1 if on_dev else 0, offs, lens, nt, dst, cap, ctypes.byref(dlen),
                                              ctypes.byref(nm), oo, ctypes.byref(st) if st is not None else None)
        _check(rc, "orz_decode_members_to_device")

    if out is None or (offsets and members is None):
        call(None, 0, None, None)  # the sizing call: total size and member count
    if out is None:
        out = torch.empty(dlen.value, dtype=torch.uint8, device=dev)
    # (an empty output still gets a real buffer of capacity 0: members that are all empty are decoded, and so checked)
    dst = out if out.numel() else torch.empty(1, dtype=torch.uint8, device=dev)
    oo = (ctypes.c_size_t * max(nm.value if members is None else nt, 1))() if offsets else None
    st = _native.DecodeStats()
    call(ctypes.c_void_p(dst.data_ptr()), out.numel(), oo, st)
    del keep
    res = [out[: dlen.value], nm.value]
    if offsets:
        res.append([oo[k] for k in range(nm.value)])
    if stats:
        res.append(st.as_dict())
    return tuple(res)


def _decode_into(planes, src, outs, device, members, elems, pieces, digests, stats, bases=None, links=None):
    """decode_members_into (planes False: member k into outs[k]) and decode_planes_into: their checks in one order, the one ABI
    call that serves the arguments, and that call's own count of host waits"""
    import torch

    if links is not None:
        if isinstance(links, bool) or not isinstance(links, int) or not 1 <= links < 1 << 32:
            raise ValueError("links is None or the number of links of a chain, an integer from 1 to 2^32 - 1")

    lib = _native.load()
    dev = torch.device("cuda", int(device))
    keep, on_dev, ptr, n = _container(src, dev)
    outs = list(outs)
    if any(not isinstance(t, torch.Tensor) or t.device != dev or not t.is_contiguous() for t in outs):
        raise ValueError("outs must be contiguous tensors on %s" % dev)
    nd = len(outs)
    el = pc = None
    if planes:
        elems = [t.element_size() for t in outs] if elems is None else [int(e) for e in elems]
        if len(elems) != nd:
            raise ValueError("one element size per tensor")
        el = (ctypes.c_uint32 * max(nd, 1))(*[e & 0xFFFFFFFF for e in elems])
    if pieces is not None:
        pieces = [int(q) for q in pieces]
        if len(pieces) != nd or any(q < 0 or q >= 1 << 32 for q in pieces):
            raise ValueError("one number of pieces per tensor, unsigned 32-bit")
        pc = (ctypes.c_uint32 * max(nd, 1))(*pieces)
    offs, lens, nt = _member_table(members)
    caps = (ctypes.c_size_t * max(nd, 1))(*[t.numel() * t.element_size() for t in outs])
    dsts = (ctypes.c_void_p * max(nd, 1))(*[(t.data_ptr() if t.numel() else None) for t in outs])
    sizes = (ctypes.c_size_t * max(nd, 1))()
    nm = ctypes.c_size_t()
    st = _native.DecodeStats()
    if bases is not None:
        bases = _base_list(bases, outs, dev, True, "outs")
    if digests is not None:
        digests, want = _digest_array(digests, nd)
        got = (ctypes.c_uint32 * max(nd, 1))()
    bs = None
    if bases is not None:
        bs = (ctypes.c_void_p * max(nd, 1))(*[(b.data_ptr() if b is not None and b.numel() else None) for b in bases])
    if links is not None:
        name = "orz_decode_tensors_chain"
        layout = (bs, el, pc, nd, want if digests is not None else None, links, sizes, got if digests is not None else None)
    elif bases is not None:
        name, layout = "orz_decode_tensors_delta", (bs, el, pc, nd, want if digests is not None else None, sizes, got if digests is not None else None)
    elif digests is not None:
        name, layout = "orz_decode_tensors_verified", (el, pc, nd, want, sizes, got)
    elif not planes:
        name, layout = "orz_decode_members_scatter", (nd, sizes)
    elif pieces is None:
        name, layout = "orz_decode_members_planes", (el, nd, sizes)
    else:
        name, layout = "orz_decode_members_planes_pieces", (el, pc, nd, sizes)
    _sync(dev)
    rc = getattr(lib, name)(int(device), ptr, n, 1 if on_dev else 0, offs, lens, nt, dsts, caps, *layout, ctypes.byref(nm), ctypes.byref(st))
    if digests is not None:
        _check_verified(rc, digests, got, name)
    else:
        _check(rc, name)
    del keep, bases
    res = [sizes[k] for k in range(nd)]
    if stats:
        d = st.as_dict()
        d["host_waits"] = int(getattr(lib, name + "_host_waits")())
        return res, d
    return res


def decode_members_into(src, outs, device=0, members=None, stats=False, digests=None):
    """decode members ON THE GPU, member k into the storage of `outs[k]` (orz_decode_members_scatter): no concatenation is made
    and nothing is copied afterwards.  `src` and `members` as for decode_members_to_device; `outs`: contiguous tensors of any
    dtype on cuda:`device`, one per member, each at least as large as its member (a member of no bytes takes an empty tensor).
    Raises OrzError, with nothing written to any tensor, when a size does not fit, the count differs from the members' or two
    tensors overlap.  `digests`: [CRC-32 of each tensor's bytes] (MemberEncoder.encode_tensors(..., digests=True)): the decoded
    bytes are digested on the GPU and held to them (orz_decode_tensors_verified, one host wait more); the first tensor that
    differs raises OrzDigestError.  Returns [decoded size of each member] (and the stats dict, with `host_waits`)."""
    return _decode_into(False, src, outs, device, members, None, None, digests, stats)


def decode_planes_into(src, outs, device=0, members=None, elems=None, stats=False, pieces=None, digests=None, bases=None, links=None):
    """decode plane members ON THE GPU and merge them (orz_decode_members_planes): `outs[k]` takes the next elems[k] members as
    the byte planes of its elements -- what MemberEncoder.encode_tensor_planes wrote.  `src` and `members` as for
    decode_members_into; `outs`: contiguous tensors on cuda:`device`, each at least as large as its planes together; `elems`:
    the element size of each (1, 2, 4 or 8), by default that of the tensors.  Raises OrzError, with nothing written to any tensor,
    when a size does not fit, the planes are not as many as the members, a tensor's planes differ in size or two tensors overlap.
    `pieces`: what MemberEncoder.encode_tensor_pieces returned beside `elems` (orz_decode_members_planes_pieces): `outs[k]` takes
    the next elems[k] x pieces[k] members, pieces[k] to a plane, and all pieces decode side by side.
    `digests`: [CRC-32 of each tensor's bytes] (what the encode calls return with digests=True): the merged bytes are digested on
    the GPU and held to them (orz_decode_tensors_verified, with or without `pieces`; one host wait more) -- a flipped payload bit,
    a member table whose entries are mixed up and a piece in the wrong place all decode without an error otherwise; the first
    tensor that differs raises OrzDigestError (.tensor, .expected, .computed), the tensors keeping what was decoded.
    `bases`: the container holds DELTAS (MemberEncoder.encode_tensor_deltas): one entry per tensor, None or the base that tensor
    was encoded against -- a contiguous tensor on cuda:`device` with the element size and number of elements of `outs[k]` --, and
    `outs[k]` gets planes XOR base, the XOR made in the merge's launch (orz_decode_tensors_delta, with or without `pieces` and
    `digests`; the same host waits as without bases).  `bases[k] is outs[k]` (or the same storage and offset) restores IN PLACE:
    the tensor holds the base on entry and the restored tensor on return.  A base that overlaps its own tensor any other way, or
    another of `outs`, raises OrzError with nothing written.  `digests` are those of the restored tensors, so a wrong base raises
    OrzDigestError.  After payload damage or a digest error a base given out of place is untouched; a tensor restored in place
    holds neither its base nor the tensor.  The default, None, changes nothing: the same call and the same waits as before.
    `links`: the container is a CHAIN of that many links (join_links), each what encode_tensor_pieces or encode_tensor_deltas
    wrote for the same list of tensors with the same piece size -- a keyframe and the deltas of the steps behind it, or deltas
    alone -- and `elems`, `pieces` are those of ONE link.  `outs[k]` gets `bases[k]` (if any) XOR tensor k of every link
    (orz_decode_tensors_chain, with or without `pieces`, `bases`, `digests`, `members` and `stats`): all links' members decode
    side by side, ONE merge launch XORs them, and the host waits are those of one call whatever the number of links.  The order
    of the links does not matter to the result.  Without `bases` the result is the XOR of the links: a chain that starts with a
    plain keyframe restores without one.  `digests` are those of the final tensors.  In place and after a failure as for `bases`.
    It costs staging memory of `links` times the tensors' bytes, freed before the call returns.  links=1 is the call without
    `links`; None (the default) changes nothing: the same ABI call and the same host waits as before; anything but None or an
    integer >= 1 raises ValueError.  A MemberReader on a chain container still sees single links: it knows nothing of chains.
    Returns [decoded size of each tensor] (and the stats dict, with `host_waits`)."""
    return _decode_into(True, src, outs, device, members, elems, pieces, digests, stats, bases, links)


def join_links(links):
    """one chain container of the links of a chain: `links` is a list of (container, members) pairs as the encode_tensor_* calls
    return them -- containers all uint8 tensors on one device, or all bytes-like -- in any order (XOR commutes).  Returns (container,
    members): the containers one behind the other and ONE member table, link-major, each link's offsets shifted by what lies in
    front of it -- what decode_planes_into(..., members=, links=len(links)) takes.  Mixed residency or no links raises ValueError."""
    import torch

    links = [(c, list(m)) for c, m in links]
    if not links:
        raise ValueError("a chain has at least one link")
    tensors = [isinstance(c, torch.Tensor) for c, _ in links]
    if any(tensors) and not all(tensors):
        raise ValueError("the containers of a chain are all tensors or all bytes")
    if tensors[0]:
        if any(c.dtype != torch.uint8 or c.dim() != 1 for c, _ in links):
            raise ValueError("a container is a uint8 tensor of one dimension")
        if any(c.device != links[0][0].device for c, _ in links):
            raise ValueError("the containers of a chain lie on one device")
        sizes = [c.numel() for c, _ in links]
        joined = torch.cat([c for c, _ in links])
    else:
        blobs = [bytes(c) for c, _ in links]
        sizes = [len(b) for b in blobs]
        joined = b"".join(blobs)
    table, at = [], 0
    for (_, members), size in zip(links, sizes):
        table += [(int(o) + at, int(ln)) for o, ln in members]
        at += size
    return joined, table


class MemberReader:
    """A members container opened ONCE for reads of byte ranges of its decoded data (orz_reader_*).  `src`: a uint8 torch tensor
    on cuda:`device` (borrowed: the reader keeps a reference, do not change it while the reader lives) or on the CPU, or
    bytes-like (uploaded).  `members`: None = `src` is one concatenation; else the [(offset, length)] list
    MemberEncoder.encode_to_device returns.  A read decodes only the members its ranges touch, each only as far as the furthest
    byte asked of it.  Reads are serial: not thread-safe.
    `cache_bytes`: a budget of device memory for CURSORS (0 = none, the default): a member's decoded prefix kept with the decoder's
    state at its end, so that a later read decodes only what is not there yet -- walking through a member window by window
    decodes it once, reading a range again or seeking backwards decodes nothing.  A cursor costs the member's decoded size
    rounded up to 256 plus MemberReader.cursor_state_bytes().
    `elems`: the container holds PLANE-ENCODED tensors (MemberEncoder.encode_tensor_planes): the element size of each tensor, as
    that call returns them (see set_planes).  read_elements / read_tensor then serve ranges of ELEMENTS, their planes merged on the
    device, and decode each plane only as far as the furthest element asked of its tensor.
    `pieces`: beside `elems`, what MemberEncoder.encode_tensor_pieces returned: the tensors' planes are cut into pieces, and a
    read decodes only the pieces its ranges touch, side by side.
    `bases`: beside `elems`, the container holds DELTAS (MemberEncoder.encode_tensor_deltas): one entry per tensor, None or the
    base that tensor was encoded against (see set_bases).  read_elements / read_tensor then return RESTORED elements, planes XOR
    base, the XOR made in the launch that ends the read: no temporary, the same launches and host waits as without bases, and
    read_tensor(j, digest=) holds the restored tensor to its digest.  A reader of such a container that has not been told the
    bases returns the DELTA's elements, and its read_tensor(..., digest=) of a tensor that has a base raises OrzDigestError,
    since the digest is the tensor's, not the delta's."""

    def __init__(self, src, device=0, members=None, cache_bytes=0, elems=None, pieces=None, bases=None):
        import torch

        self._h = None
        if bases is not None and elems is None:
            raise ValueError("bases are those of declared tensors: give elems")
        self._lib = _native.load()
        self._dev = torch.device("cuda", int(device))
        keep, on_dev, ptr, n = _container(src, self._dev)
        offs, lens, nt = _member_table(members)
        _sync(self._dev)
        self._h = self._lib.orz_reader_open(int(device), ptr, n, 1 if on_dev else 0, offs, lens, nt)
        if not self._h:
            raise OrzError("orz_reader_open failed: %s" % _native.last_error())
        self._keep = keep if on_dev else None  # (a host container was copied)
        m, tot = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._lib.orz_reader_info(self._h, ctypes.byref(m), ctypes.byref(tot), None, 0), "orz_reader_info")
        self.members, self.total = m.value, tot.value
        self._offsets = None
        self._tensors = []
        self._bases = None
        try:
            if cache_bytes:
                self.set_cache(cache_bytes)
            if elems is not None:
                self.set_planes(elems, pieces)
            if bases is not None:
                self.set_bases(bases)
        except Exception:
            self.close()
            raise

    @staticmethod
    def cursor_state_bytes():
        """what a cursor costs of the budget beyond its member's decoded bytes"""
        return _native.load().orz_reader_cursor_state_bytes()

    def set_cache(self, nbytes):
        """the budget for cursors in bytes; 0 switches the cache off and frees every cursor, a smaller budget evicts the least
        recently touched ones"""
        if not self._h:
            raise OrzError("the reader is closed")
        if int(nbytes) < 0 or int(nbytes) >= 1 << 64:
            raise ValueError("the budget is an unsigned 64-bit number")
        _check(self._lib.orz_reader_set_cache(self._h, int(nbytes)), "orz_reader_set_cache")

    def cache_stats(self):
        """{hits, resumed, fresh, uncached, evicted} of the last read in members, and {cursors, bytes, budget} now"""
        if not self._h:
            raise OrzError("the reader is closed")
        st = _native.CacheStats()
        _check(self._lib.orz_reader_cache_stats(self._h, ctypes.byref(st)), "orz_reader_cache_stats")
        return st.as_dict()

    @property
    def member_offsets(self):
        """where each member's bytes start in the decoded data"""
        if self._offsets is None:
            oo = (ctypes.c_uint64 * max(self.members, 1))()
            _check(self._lib.orz_reader_info(self._h, None, None, oo, self.members), "orz_reader_info")
            self._offsets = [oo[k] for k in range(self.members)]
        return list(self._offsets)

    def read_ranges(self, ranges, out=None, stats=False):
        """the bytes of [(offset, length), ...] of the decoded data, back to back in that order, as a uint8 tensor on the device
        (the first bytes of `out` when given: nothing else of it is written)[, stats dict]"""
        import torch

        if not self._h:
            raise OrzError("the reader is closed")
        if out is not None:
            _uint8_out(out, self._dev)
        ranges = [(int(o), int(ln)) for o, ln in ranges]
        if any(o < 0 or ln < 0 or o >= 1 << 64 or ln >= 1 << 64 for o, ln in ranges):
            raise ValueError("offsets and lengths are unsigned 64-bit numbers")
        nr = len(ranges)
        off = (ctypes.c_uint64 * max(nr, 1))(*[o for o, _ in ranges])
        ln = (ctypes.c_uint64 * max(nr, 1))(*[l for _, l in ranges])
        if out is None:
            # (ranges the library will refuse get a buffer of one byte: the refusal comes from the library, with its message)
            want = sum(l for o, l in ranges) if all(o + l <= self.total for o, l in ranges) else 0
            out = torch.empty(want, dtype=torch.uint8, device=self._dev)
        dst = out if out.numel() else torch.empty(1, dtype=torch.uint8, device=self._dev)
        _sync(self._dev)
        dlen = ctypes.c_uint64()
        st = _native.ReadStats()
        rc = self._lib.orz_reader_read(self._h, off, ln, nr, ctypes.c_void_p(dst.data_ptr()), out.numel(), ctypes.byref(dlen),
                                       ctypes.byref(st))
        _check(rc, "orz_reader_read")
        res = out[: dlen.value]
        return (res, st.as_dict()) if stats else res

    def read(self, offset, length, out=None, stats=False):
        """`length` decoded bytes from `offset` (read_ranges of one range)"""
        return self.read_ranges([(offset, length)], out=out, stats=stats)

    def set_planes(self, elems, pieces=None):
        """declare the container as plane-encoded tensors: tensor j is the next elems[j] members, plane 0 first -- the element sizes
        MemberEncoder.encode_tensor_planes returns.  None or an empty list withdraws the declaration.  With `pieces`, what
        encode_tensor_pieces returns beside them, tensor j is the next elems[j] x pieces[j] members, pieces[j] to a plane
        (orz_reader_set_planes_pieces).  Raises OrzError, with nothing changed, for an element size other than 1, 2, 4, 8, planes
        that are not as many as the members, planes of one tensor that differ in size, or pieces that do not fit together.
        Cursors are kept and read_ranges does what it did.  A declaration that succeeds withdraws the bases (set_bases), as the
        library does: they were those of the tensors declared before."""
        if not self._h:
            raise OrzError("the reader is closed")
        elems = [] if elems is None else [int(e) for e in elems]
        if any(e < 0 or e >= 1 << 32 for e in elems):
            raise ValueError("element sizes are unsigned 32-bit numbers")
        nt = len(elems)
        el = (ctypes.c_uint32 * max(nt, 1))(*elems)
        if pieces is None:
            _check(self._lib.orz_reader_set_planes(self._h, el, nt), "orz_reader_set_planes")
        else:
            pieces = [int(q) for q in pieces]
            if len(pieces) != nt or any(q < 0 or q >= 1 << 32 for q in pieces):
                raise ValueError("one number of pieces per tensor, unsigned 32-bit")
            pc = (ctypes.c_uint32 * max(nt, 1))(*pieces)
            _check(self._lib.orz_reader_set_planes_pieces(self._h, el, pc, nt), "orz_reader_set_planes_pieces")
        n = ctypes.c_uint64()
        counts = (ctypes.c_uint64 * max(nt, 1))()
        sizes = (ctypes.c_uint32 * max(nt, 1))()
        _check(self._lib.orz_reader_tensor_info(self._h, ctypes.byref(n), counts, sizes, nt), "orz_reader_tensor_info")
        self._tensors = [(counts[j], sizes[j]) for j in range(min(n.value, nt))]
        self._bases = None

    def set_bases(self, bases):
        """the container holds DELTAS (orz_reader_set_bases): `bases` has one entry per declared tensor, None or the base the tensor
        was encoded against -- a contiguous tensor on the reader's device with the tensor's element size and number of elements;
        anything else raises ValueError.  read_elements / read_tensor then return planes XOR base for the tensors that have one.
        None or an empty list withdraws the bases.  The reader keeps references to the bases while they are set and only reads
        them.  Nothing is launched and cursors are kept: the same range read against another base decodes nothing anew."""
        if not self._h:
            raise OrzError("the reader is closed")
        bases = [] if bases is None else list(bases)
        if bases:
            bases = _base_list(bases, [_Declared(c, e) for c, e in self._tensors], self._dev, self._dev.type == "cuda", "tensors")
        nb = len(bases)
        bs = (ctypes.c_void_p * max(nb, 1))(*[(b.data_ptr() if b is not None and b.numel() else None) for b in bases])
        _check(self._lib.orz_reader_set_bases(self._h, bs, nb), "orz_reader_set_bases")
        self._bases = bases or None

    @property
    def tensors(self):
        """[(element count, element size)] of the tensors declared ([] when none are)"""
        return list(self._tensors)

    def read_elements(self, ranges, out=None, stats=False):
        """the elements of [(tensor, first, count), ...], their interleaved bytes back to back in that order, as a uint8 tensor on
        the device (the first bytes of `out` when given: nothing else of it is written)[, stats dict].  Unverified: a part of a
        tensor has no digest -- read_tensor(j, digest=...) checks a whole one.  With bases set, the ranges of tensors that have a
        base come back restored; such a range's slice of its base must lie apart from the bytes of `out` that are written, or be
        exactly where the range's own bytes go (in place), else OrzError naming the range."""
        import torch

        if not self._h:
            raise OrzError("the reader is closed")
        if out is not None:
            _uint8_out(out, self._dev)
        ranges = [(int(j), int(f), int(c)) for j, f, c in ranges]
        if any(v < 0 or v >= 1 << 64 for r in ranges for v in r):
            raise ValueError("tensor numbers, first elements and counts are unsigned 64-bit numbers")
        nr = len(ranges)
        tj = (ctypes.c_uint64 * max(nr, 1))(*[r[0] for r in ranges])
        tf = (ctypes.c_uint64 * max(nr, 1))(*[r[1] for r in ranges])
        tc = (ctypes.c_uint64 * max(nr, 1))(*[r[2] for r in ranges])
        if out is None:
            # (ranges the library will refuse get a buffer of one byte: the refusal comes from the library, with its message)
            t = self._tensors
            ok = all(j < len(t) and f + c <= t[j][0] for j, f, c in ranges)
            out = torch.empty(sum(c * t[j][1] for j, f, c in ranges) if ok else 0, dtype=torch.uint8, device=self._dev)
        dst = out if out.numel() else torch.empty(1, dtype=torch.uint8, device=self._dev)
        _sync(self._dev)
        dlen = ctypes.c_uint64()
        st = _native.ReadStats()
        rc = self._lib.orz_reader_read_elements(self._h, tj, tf, tc, nr, ctypes.c_void_p(dst.data_ptr()), out.numel(), ctypes.byref(dlen),
                                                ctypes.byref(st))
        _check(rc, "orz_reader_read_elements")
        res = out[: dlen.value]
        return (res, st.as_dict()) if stats else res

    def _hold_to(self, j, digest, got):
        """raises OrzDigestError unless the bytes of `got` (tensor j, whole) have the digest"""
        computed = crc32_buffers([got], device=self._dev.index)[0]
        if computed != digest:
            raise OrzDigestError("digest mismatch: tensor %d should have CRC-32 0x%08x, its decoded bytes have 0x%08x" % (j, digest, computed),
                                 j, digest, computed)

    def read_tensor(self, j, first=0, count=None, out=None, dtype=None, digest=None):
        """`count` elements of tensor `j` from element `first` (by default all that follow it): read_elements of one range.  With
        `out`, a contiguous tensor on the device whose element size is the tensor's, the elements are written into it and the
        written slice is returned; otherwise the bytes, viewed as `dtype` when given.  `digest`: the CRC-32 of the WHOLE tensor's
        bytes -- only with first == 0 and count None or all of it, else ValueError: after the read the result is digested on the
        GPU (crc32_buffers) and OrzDigestError raised when it differs.  With bases set the elements are the restored ones, and
        `out=B[first:first + count]`, B being tensor j's base, restores those elements IN PLACE."""
        import torch

        j, first = int(j), int(first)
        if j < 0 or first < 0 or j >= 1 << 64 or first >= 1 << 64:
            raise ValueError("the tensor number and the first element are unsigned 64-bit numbers")
        if count is None:
            count = max(self._tensors[j][0] - first, 0) if j < len(self._tensors) else 0
        count = int(count)
        if count < 0 or count >= 1 << 64:
            raise ValueError("the count is an unsigned 64-bit number")
        if digest is not None:
            digest = int(digest)
            if digest < 0 or digest >= 1 << 32:
                raise ValueError("a digest is an unsigned 32-bit number")
            if first != 0 or (j < len(self._tensors) and count != self._tensors[j][0]):
                raise ValueError("a digest vouches for a whole tensor: a partial read has none")
        if out is None:
            res = self.read_elements([(j, first, count)])
            if digest is not None:
                self._hold_to(j, digest, res)
            return res.view(dtype) if dtype is not None else res
        if not isinstance(out, torch.Tensor) or out.device != self._dev or not out.is_contiguous():
            raise ValueError("out must be a contiguous tensor on %s" % self._dev)
        if j < len(self._tensors) and out.element_size() != self._tensors[j][1]:
            raise ValueError("out has elements of %d bytes, tensor %d of %d" % (out.element_size(), j, self._tensors[j][1]))
        flat = out.reshape(-1)
        got = self.read_elements([(j, first, count)], out=flat.view(torch.uint8))
        if digest is not None:
            self._hold_to(j, digest, got)
        return flat[: got.numel() // out.element_size()]

    def close(self):
        if self._h:
            self._lib.orz_reader_close(self._h)
            self._h = None
            self._keep = None
            self._bases = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def huffman_tables(weights, device=0):
    """Huffman code lengths and canonical codes of every table of `weights` ON THE GPU -- an array of shape
    [nchunks, orz_huffman_stride()] of symbol weights below 2^23 in the encoder's layout (389 + 389 + 240 symbols a chunk;
    HuffmanTable::new_from_sym_weights + HuffmanEncoding::from_huffman_table, src/huffman.rs:27-141)
    -> (lens uint8 array, codes uint16 array, microseconds of the kernel launch)."""
    import numpy as np

    lib = _native.load()
    w0 = np.asarray(weights)
    if w0.size and (not np.issubdtype(w0.dtype, np.integer) or (w0 < 0).any() or (w0 >= (1 << 23)).any()):
        raise ValueError("weights must be integers in [0, 2^23)")  # (before the cast: a negative or huge weight must not wrap into range)
    w = np.ascontiguousarray(w0, dtype=np.uint32)
    stride = lib.orz_huffman_stride()
    if w.ndim != 2 or w.shape[1] != stride:
        raise ValueError("weights must have shape [nchunks, %d]" % stride)
    lens = np.zeros(w.shape, dtype=np.uint8)
    codes = np.zeros(w.shape, dtype=np.uint16)
    us = ctypes.c_double()
    rc = lib.orz_huffman_tables(device, w.ctypes.data, w.shape[0], lens.ctypes.data, codes.ctypes.data, ctypes.byref(us))
    _check(rc, "orz_huffman_tables")
    return lens, codes, us.value


SYMRANK_WORDS = 389 * 2 + 4  # a context's table in the encoder's layout: value[389], index[389], cnt lo/hi, sum lo/hi (u16)
SYMRANK_MAX_SUM = 1000000 + 390 * 388  # the largest idx_sum the reference reaches (src/symrank.rs:22-29,63-66)


def _symrank_inputs(tables, gsym, rstart):
    """validated, contiguous copies of symrank_chains' arguments; ValueError for what the library would refuse"""
    import numpy as np

    t = np.asarray(tables)
    if t.shape != (512, SYMRANK_WORDS) or not np.issubdtype(t.dtype, np.integer) or (t < 0).any() or (t > 0xFFFF).any():
        raise ValueError("tables must be u16 values of shape [512, %d]" % SYMRANK_WORDS)
    t = np.array(t, dtype=np.uint16, order="C", copy=True)  # (the library writes the final tables into it: never the caller's array)
    g0 = np.asarray(gsym).reshape(-1)
    if g0.size and (not np.issubdtype(g0.dtype, np.integer) or (g0 < 0).any() or (g0 >= (1 << 32)).any()):
        raise ValueError("gsym must be integers symbol | excluded symbol << 16")
    g = np.ascontiguousarray(g0, dtype=np.uint32)
    if ((g & 0xFFFF) >= 389).any() or ((g >> 16) >= 389).any():
        raise ValueError("symbols and excluded symbols must be below 389")
    r0 = np.asarray(rstart).reshape(-1)
    if r0.shape != (513,) or not np.issubdtype(r0.dtype, np.integer) or (r0 < 0).any():
        raise ValueError("rstart must hold 513 non-negative integers")
    r = np.ascontiguousarray(r0, dtype=np.int64)
    if r[0] != 0 or r[512] != g.size or (np.diff(r) < 0).any():
        raise ValueError("rstart must be monotone from 0 to len(gsym)")
    val, idx = t[:, :389].astype(np.int64), t[:, 389:778].astype(np.int64)
    if (val >= 389).any() or (np.take_along_axis(idx, val, axis=1) != np.arange(389)).any():
        raise ValueError("value[] and index[] of every context must be inverse permutations")
    cnt = t[:, 778].astype(np.int64) | (t[:, 779].astype(np.int64) << 16)
    sm = t[:, 780].astype(np.int64) | (t[:, 781].astype(np.int64) << 16)
    if (cnt > 390).any() or (sm > SYMRANK_MAX_SUM).any():
        raise ValueError("count must be at most 390 and sum at most %d" % SYMRANK_MAX_SUM)
    return t, g, r.astype(np.uint32)


def symrank_chains(tables, gsym, rstart, device=0):
    """The encoder's symbol-ranking sequence (HipBackend::symrank: backup, kernel, check, guarded rerun) ON THE GPU for one
    launch -- SymRankCoder::encode (src/symrank.rs:38-97) over each context's items.  `tables`: [512, 782] u16 in the
    encoder's layout; `gsym`: symbol | excluded symbol << 16 for every item, grouped by context; `rstart`: 513 offsets
    -> (ranks uint16 array, tables as the chains left them, (flags[0], flags[1]) of the guard, microseconds of the sequence)."""
    import numpy as np

    t, g, r = _symrank_inputs(tables, gsym, rstart)
    lib = _native.load()
    ranks = np.zeros(g.size, dtype=np.uint16)
    flags = np.zeros(2, dtype=np.uint32)
    us = ctypes.c_double()
    rc = lib.orz_symrank_chains(device, t.ctypes.data, g.ctypes.data, r.ctypes.data, g.size, ranks.ctypes.data, flags.ctypes.data,
                                ctypes.byref(us))
    _check(rc, "orz_symrank_chains")
    return ranks, t, (int(flags[0]), int(flags[1])), us.value


def decode_bytes(stream):
    """orz stream -> (bytes, consumed).  Host decoder of the library (orz::decode, src/lib.rs:94-129);
    stops after the first stream's EOF chunk like the reference."""
    lib = _native.load()
    stream = bytes(stream)
    dst = ctypes.POINTER(ctypes.c_uint8)()
    n, used = ctypes.c_size_t(), ctypes.c_size_t()
    buf = ctypes.create_string_buffer(stream, len(stream)) if stream else ctypes.create_string_buffer(1)
    rc = lib.orz_decode_mem(ctypes.cast(buf, ctypes.c_void_p), len(stream), ctypes.byref(dst), ctypes.byref(n), ctypes.byref(used))
    _check(rc, "orz_decode_mem")
    try:
        return ctypes.string_at(dst, n.value), used.value
    finally:
        lib.orz_free(dst)


def decode(src, dst, progress=None):
    """orz::decode (src/lib.rs:94-129) between file-like objects; returns (bytes_read, bytes_written)."""
    lib = _native.load()
    counts = [0, 0]

    def _rd(_ctx, buf, cap):
        try:
            chunk = src.read(cap)
        except Exception:
            return -1
        if chunk:
            ctypes.memmove(buf, chunk, len(chunk))
            counts[0] += len(chunk)
        return len(chunk)

    def _wr(_ctx, buf, n):
        try:
            dst.write(ctypes.string_at(buf, n))
        except Exception:
            return -1
        counts[1] += n
        return 0

    def _pg(_ctx, fin, a, b):
        if progress:
            progress(bool(fin), a, b)

    rd, wr, pg = _native.READ_FN(_rd), _native.WRITE_FN(_wr), _native.PROGRESS_FN(_pg)
    _check(lib.orz_decode(rd, None, wr, None, pg, None), "orz_decode")
    return tuple(counts)


class LZEncoder:
    """Object-level mirror of the reference's LZEncoder (src/lz.rs:69-95).

    `encode(cfg, window, sbuf_len, spos)` takes the caller's window allocation INCLUDING the two
    480-byte sentinel pads (i.e. `window[480]` is sbuf[0], as `orz::encode` lays it out,
    src/lib.rs:67-69) and returns (spos_out, chunk_bytes)."""

    def __init__(self, device=0):
        self._lib = _native.load()
        self._h = self._lib.orz_lz_encoder_new(int(device))
        if not self._h:
            raise OrzError("orz_lz_encoder_new failed: " + _native.last_error())
        self._tbuf = ctypes.create_string_buffer(3 * 16777215)

    def encode(self, cfg, window, sbuf_len, spos):
        base = ctypes.addressof(window) if not isinstance(window, int) else window
        so, tl = ctypes.c_size_t(), ctypes.c_size_t()
        rc = self._lib.orz_lz_encoder_encode(
            self._h, ctypes.byref(cfg), ctypes.c_void_p(base + 480), sbuf_len, self._tbuf, len(self._tbuf), spos,
            ctypes.byref(so), ctypes.byref(tl),
        )
        _check(rc, "orz_lz_encoder_encode")
        return so.value, self._tbuf.raw[: tl.value]

    def forward(self, forward_len):
        _check(self._lib.orz_lz_encoder_forward(self._h, forward_len), "orz_lz_encoder_forward")

    def close(self):
        if self._h:
            self._lib.orz_lz_encoder_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
