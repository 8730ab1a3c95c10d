"""dev: what the list-of-buffers entry points cost beside the contiguous ones they stand next to.  Four legs, each in a child
process of its own (one library per process), one JSON line per leg into --out (default profiles/segments_bench.jsonl):

  encode, segments     64 separate device allocations of 4 MiB of the text workload -> orz_members_encode_segments_to_device
  encode, packed       the same bytes in one allocation -> orz_members_encode_to_device at member_bytes = 4 MiB
  decode, scatter      64 members of 256 KiB -> orz_decode_members_scatter into 64 tensors
  decode, then split   the same members -> orz_decode_members_to_device, then 64 device-to-device copies into the 64 tensors

The packed / split legs go through the C ABI alone (ctypes), so --baseline-lib may name the liborz_hip.so of an older commit,
which has none of the new symbols; without it they measure this tree's library and say so.  Every leg runs three times after a
warm-up and reports each wall time, the median, the spread (max - min) and MB/s of the median; the decode legs check their
bytes."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
sys.path.insert(0, os.getcwd())
sys.path.insert(0, "tools")

ENC_SEGS, ENC_BYTES = 64, 4 << 20
DEC_SEGS, DEC_BYTES = 64, 256 << 10
JOBS, RUNS = 8, 3
LEGS = ["encode, segments", "encode, packed", "decode, scatter", "decode, then split"]


def workload(nseg, nbytes):
    import corpus

    base = corpus.enwik_like(min(nseg * nbytes, 1 << 26))
    return (base * (nseg * nbytes // len(base) + 1))[: nseg * nbytes]


def timed(fn, sync):
    fn()  # warm-up: buffers, the kernels' code
    sync()
    walls = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        sync()
        walls.append(time.perf_counter() - t0)
    return sorted(walls)


def row(leg, lib, nbytes, walls, **more):
    med = walls[len(walls) // 2]
    r = {"leg": leg, "library": lib, "in_bytes": nbytes, "runs": len(walls), "wall_ms": [round(w * 1e3, 2) for w in walls],
         "median_ms": round(med * 1e3, 2), "spread_ms": round((walls[-1] - walls[0]) * 1e3, 2), "MBps": round(nbytes / med / 1e6, 1)}
    r.update(more)
    return r


class Abi:
    """the few calls the baseline legs need, bound by hand: any liborz_hip.so that has them will do"""

    class Cfg(ctypes.Structure):
        _fields_ = [("a", ctypes.c_size_t), ("b", ctypes.c_size_t), ("c", ctypes.c_size_t)]

    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        lib.orz_members_new.restype = ctypes.c_void_p
        lib.orz_stream_bound.restype = ctypes.c_size_t
        lib.orz_stream_bound.argtypes = [ctypes.c_size_t]
        lib.orz_last_error.restype = ctypes.c_char_p
        self.cfg = self.Cfg()
        assert lib.orz_lzcfg_from_level(1, ctypes.byref(self.cfg)) == 0
        self.h = lib.orz_members_new(0, ctypes.byref(self.cfg), JOBS)
        assert self.h, lib.orz_last_error()

    def encode_to_device(self, src, dst, member_bytes):
        nm = (src.numel() + member_bytes - 1) // member_bytes
        offs, lens, got = (ctypes.c_size_t * nm)(), (ctypes.c_size_t * nm)(), ctypes.c_size_t()
        rc = self.lib.orz_members_encode_to_device(ctypes.c_void_p(self.h), ctypes.c_void_p(src.data_ptr()), ctypes.c_size_t(src.numel()), 1,
                                                   ctypes.c_size_t(member_bytes), ctypes.c_void_p(dst.data_ptr()), ctypes.c_size_t(dst.numel()),
                                                   offs, lens, ctypes.byref(got))
        assert rc == 0, self.lib.orz_last_error()
        return [(offs[k], lens[k]) for k in range(got.value)]

    def decode_to_device(self, src, members, out):
        nm = len(members)
        offs = (ctypes.c_size_t * nm)(*[o for o, _ in members])
        lens = (ctypes.c_size_t * nm)(*[n for _, n in members])
        dlen, got = ctypes.c_size_t(), ctypes.c_size_t()
        rc = self.lib.orz_decode_members_to_device(0, ctypes.c_void_p(src.data_ptr()), ctypes.c_size_t(src.numel()), 1, offs, lens,
                                                   ctypes.c_size_t(nm), ctypes.c_void_p(out.data_ptr()), ctypes.c_size_t(out.numel()),
                                                   ctypes.byref(dlen), ctypes.byref(got), None, None)
        assert rc == 0, self.lib.orz_last_error()
        return dlen.value

    def close(self):
        self.lib.orz_members_free(ctypes.c_void_p(self.h))


def run_leg(leg, baseline):
    import torch

    sync = torch.cuda.synchronize
    if leg.startswith("encode"):
        nseg, nbytes = ENC_SEGS, ENC_BYTES
    else:
        nseg, nbytes = DEC_SEGS, DEC_BYTES
    data = workload(nseg, nbytes)
    total = nseg * nbytes
    if leg in ("encode, segments", "decode, scatter"):
        import orz_amd

        tensors = [torch.frombuffer(bytearray(data[k * nbytes:(k + 1) * nbytes]), dtype=torch.uint8).to("cuda:0") for k in range(nseg)]
        enc = orz_amd.MemberEncoder(device=0, level=1, jobs=JOBS)
        out = torch.empty(enc.bound_segments([nbytes] * nseg), dtype=torch.uint8, device="cuda:0")
        if leg == "encode, segments":
            walls = timed(lambda: enc.encode_tensors(tensors, out=out), sync)
            members = enc.encode_tensors(tensors, out=out)[1]
            r = row(leg, "this tree", total, walls, members=len(members), out_bytes=sum(n for _, n in members), host_waits=None)
        else:
            container, members = enc.encode_tensors(tensors, out=out)
            outs = [torch.empty(nbytes, dtype=torch.uint8, device="cuda:0") for _ in range(nseg)]
            stats = []
            walls = timed(lambda: stats.append(orz_amd.decode_members_into(container, outs, members=members, stats=True)[1]), sync)
            exact = all(bool(torch.equal(a, b)) for a, b in zip(outs, tensors))
            r = row(leg, "this tree", total, walls, members=len(members), exact=exact, host_waits=stats[-1]["host_waits"],
                    kernel_ms=round(stats[-1]["kernel_ms"], 2))
        enc.close()
    else:
        import orz_amd._native as native  # (for the path alone: nothing of it is loaded)

        abi = Abi(baseline or native.LIB_PATH)
        lib = "baseline (--baseline-lib)" if baseline else "this tree"
        src = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
        out = torch.empty(nseg * abi.lib.orz_stream_bound(nbytes), dtype=torch.uint8, device="cuda:0")
        if leg == "encode, packed":
            walls = timed(lambda: abi.encode_to_device(src, out, nbytes), sync)
            members = abi.encode_to_device(src, out, nbytes)
            r = row(leg, lib, total, walls, members=len(members), out_bytes=sum(n for _, n in members), host_waits=None)
        else:
            members = abi.encode_to_device(src, out, nbytes)
            whole = torch.empty(total, dtype=torch.uint8, device="cuda:0")
            outs = [torch.empty(nbytes, dtype=torch.uint8, device="cuda:0") for _ in range(nseg)]

            def decode_and_split():
                assert abi.decode_to_device(out, members, whole) == total
                for k, t in enumerate(outs):
                    t.copy_(whole[k * nbytes:(k + 1) * nbytes])

            walls = timed(decode_and_split, sync)
            exact = all(bool(torch.equal(t, src[k * nbytes:(k + 1) * nbytes])) for k, t in enumerate(outs))
            r = row(leg, lib, total, walls, members=len(members), exact=exact, host_waits=None, copies=nseg)
        abi.close()
    r["device"] = torch.cuda.get_device_name(0)
    print("ROW " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "segments_bench.jsonl"))
    ap.add_argument("--baseline-lib", default="")
    ap.add_argument("--leg", default="")
    args = ap.parse_args()
    if args.leg:
        run_leg(args.leg, args.baseline_lib)
        return
    rows = []
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg]
        if args.baseline_lib:
            cmd += ["--baseline-lib", args.baseline_lib]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=240)
        if p.returncode != 0:  # (whatever failed on the device: nothing more is started on it)
            sys.exit("leg %r failed with status %d" % (leg, p.returncode))
        rows += [json.loads(ln[4:]) for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
        print(json.dumps(rows[-1]), flush=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
