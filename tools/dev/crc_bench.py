"""dev: what the digests cost (orz_crc.h).  Three legs, each once, in a child process of its own under its own time limit, one JSON
line per leg into --out (default profiles/crc_bench.jsonl); a leg that fails ends the run:

  kernels             orz_crc32_buffers over ONE buffer of 256 MiB: events around 5 calls after a warming one, beside Tensor.copy_ of
                      the same bytes in the same process (events around 5 copies after a warming one).  A call is the whole entry
                      point -- a backend of its own, the table's upload, three launches, the read of the digest --, not the kernels
                      alone.  The digest is checked against zlib's.
  decode              64 tensors of 256 KiB of the text workload as planes (the container of segments_bench.py), decode_planes_into
                      with and without `digests`, three runs each, interleaved after a warm-up, in one process: both sets of wall
                      times and kernel_ms.  The rule of the range reader: the verified set should lie within the unverified set's
                      own range widened by its width.
  decode, baseline    the unverified half of that leg alone with the library --baseline-lib names (an older commit's: it has none
                      of the new symbols), judged by the same rule against the `decode` leg's unverified set.  Skipped without it."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time
import zlib

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
sys.path.insert(0, os.getcwd())
sys.path.insert(0, "tools")

KERNEL_BYTES, REPS = 256 << 20, 5
SEGS, SEG_BYTES, JOBS, RUNS = 64, 256 << 10, 8, 3
LEGS = ["kernels", "decode", "decode, baseline"]
LIMIT_S = 240


def kernels():
    import torch

    import orz_amd

    g = torch.Generator(device="cuda:0").manual_seed(5)
    buf = torch.randint(0, 256, (KERNEL_BYTES,), generator=g, dtype=torch.uint8, device="cuda:0")
    back = torch.empty_like(buf)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    got = orz_amd.crc32_buffers([buf])
    a.record()
    t0 = time.perf_counter()
    for _ in range(REPS):
        got = orz_amd.crc32_buffers([buf])
    wall = (time.perf_counter() - t0) / REPS
    b.record()
    torch.cuda.synchronize()
    crc_ms = a.elapsed_time(b) / REPS
    back.copy_(buf)
    a.record()
    for _ in range(REPS):
        back.copy_(buf)
    b.record()
    torch.cuda.synchronize()
    copy_ms = a.elapsed_time(b) / REPS
    return {"bytes": KERNEL_BYTES, "crc_call_ms": round(crc_ms, 4), "crc_call_wall_ms": round(wall * 1e3, 4), "copy_ms": round(copy_ms, 4),
            "crc_over_copy": round(crc_ms / copy_ms, 2), "crc_GBps": round(KERNEL_BYTES / crc_ms / 1e6, 1),
            "copy_GBps_each_way": round(KERNEL_BYTES / copy_ms / 1e6, 1), "exact": got == [zlib.crc32(buf.cpu().numpy().tobytes())]}


def within(walls, ref):
    """the rule: every wall time inside ref's own range widened by its width; else by how much the worst lies outside"""
    lo, hi = min(ref), max(ref)
    w = hi - lo
    out = max(max(walls) - (hi + w), (lo - w) - min(walls), 0.0)
    return {"inside": out == 0.0, "outside_by_ms": round(out, 3), "range_ms": [round(lo - w, 3), round(hi + w, 3)]}


def decode(baseline):
    import torch

    from orz_amd import _native

    if baseline:  # an older library has none of the new symbols: bind what it has
        _native.LIB_PATH = os.path.abspath(baseline)
        old = ctypes.CDLL(_native.LIB_PATH)
        _native.SYMBOLS = [s for s in _native.SYMBOLS if hasattr(old, s[0])]
    import corpus
    import orz_amd

    base = corpus.enwik_like(SEGS * SEG_BYTES)
    tensors = [torch.frombuffer(bytearray(base[k * SEG_BYTES:(k + 1) * SEG_BYTES]), dtype=torch.uint8).to("cuda:0").view(torch.int16) for k in range(SEGS)]
    enc = orz_amd.MemberEncoder(device=0, level=1, jobs=JOBS)
    res = enc.encode_tensor_planes(tensors) if baseline else enc.encode_tensor_planes(tensors, digests=True)
    container, members, elems = res[:3]
    crcs = None if baseline else res[3]
    outs = [torch.empty_like(t) for t in tensors]
    sets = {"unverified": [], "verified": []}
    kern = {"unverified": [], "verified": []}
    waits = {}

    def run(which):
        kw = {"digests": crcs} if which == "verified" else {}
        t0 = time.perf_counter()
        _, st = orz_amd.decode_planes_into(container, outs, device=0, members=members, elems=elems, stats=True, **kw)
        torch.cuda.synchronize()
        sets[which].append((time.perf_counter() - t0) * 1e3)
        kern[which].append(st["kernel_ms"])
        waits[which] = st["host_waits"]

    order = ["unverified"] if baseline else ["unverified", "verified"]
    for which in order:  # the warm-up
        run(which)
    for which in order:
        sets[which].clear()
        kern[which].clear()
    for _ in range(RUNS):
        for which in order:
            run(which)
    enc.close()
    r = {"bytes": SEGS * SEG_BYTES, "members": len(members), "library": "baseline (--baseline-lib)" if baseline else "this tree",
         "exact": all(bool(torch.equal(a, b)) for a, b in zip(outs, tensors))}
    for which in order:
        r[which + "_wall_ms"] = [round(w, 3) for w in sets[which]]
        r[which + "_kernel_ms"] = [round(k, 3) for k in kern[which]]
        r[which + "_host_waits"] = waits[which]
    if not baseline:
        r["verified_within_unverified"] = within(sets["verified"], sets["unverified"])
    return r


def run_leg(leg, baseline):
    import torch

    r = {"leg": leg}
    r.update(kernels() if leg == "kernels" else decode(baseline if leg.endswith("baseline") else ""))
    r["device"] = torch.cuda.get_device_name(0)
    print("ROW " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "crc_bench.jsonl"))
    ap.add_argument("--baseline-lib", default="")
    ap.add_argument("--leg", default="")
    args = ap.parse_args()
    if args.leg:
        run_leg(args.leg, args.baseline_lib)
        return
    rows = []
    for leg in LEGS:
        if leg.endswith("baseline") and not args.baseline_lib:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--baseline-lib", args.baseline_lib]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT_S)
        if p.returncode != 0:  # (whatever failed on the device: nothing more is started on it)
            sys.exit("leg %r failed with status %d" % (leg, p.returncode))
        rows += [json.loads(ln[4:]) for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
        if leg.endswith("baseline"):
            ours = next(r for r in rows if r["leg"] == "decode")
            rows[-1]["this_tree_within_baseline"] = within(ours["unverified_wall_ms"], rows[-1]["unverified_wall_ms"])
        print(json.dumps(rows[-1]), flush=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
