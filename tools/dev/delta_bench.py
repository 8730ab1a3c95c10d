"""dev: what the delta layout costs and buys (orz_planes.h: PlaneSplitDelta / PlaneMergeDelta; orz_read_elements.h:
ElementGatherDelta).  Nine legs, each once, in a child process of its own under its own time limit, one JSON line per leg into
--out (default profiles/delta_bench.jsonl; --only PREFIX runs the legs whose names begin with it and APPENDS their lines):

  kernels, e = 1 / 2 / 4 / 8   PlaneSplitDelta and PlaneMergeDelta over ONE tensor of 256 MiB and its base, all at 16-aligned
                               addresses (orz_plane_delta_move_time: events around 5 launches after a warming one); beside them, in
                               the same process, PlaneSplit and PlaneMerge over the same tensor (orz_plane_move_time; not for e = 1,
                               which the plain kernels do not move) and a device-to-device copy of the same 256 MiB (Tensor.copy_).
                               A delta move carries three bytes per byte of tensor where the plain one carries two: about 1.5 x
                               the plain kernel is what bandwidth predicts.  Split, merge and the merge in place are checked.
  bf16 16 Mi, plain and delta  w = randn * 0.02 and its successor w + randn * 1e-4, 16 Mi bf16 elements, as pieces of 2^18:
                               the successor through encode_tensor_pieces / decode_planes_into and through encode_tensor_deltas /
                               decode_planes_into(bases=) in ONE process -- container bytes, encode wall time (median of 3 after a
                               warm-up) and the decode's kernel_ms, the delta's each against the plain one's.
  gather, e = 1 / 2 / 4 / 8    the launch that ends ONE whole-tensor element read of a 256 MiB tensor (orz_element_gather_time: events
                               around 5 launches after a warming one): ElementGatherDelta against ElementGather over the same planes,
                               all at 16-aligned addresses.  Three bytes carried where the plain gather carries two: about 1.5 x
                               is what bandwidth predicts.  Both results, and the gather in place, are checked."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
sys.path.insert(0, os.getcwd())

KERNEL_BYTES, REPS = 256 << 20, 5
ELEMENTS, PIECE, JOBS, LR = 16 << 20, 1 << 18, 4, 1e-4
LEGS = ["kernels, e = 1", "kernels, e = 2", "kernels, e = 4", "kernels, e = 8", "bf16 16 Mi, plain and delta", "gather, e = 1", "gather, e = 2",
        "gather, e = 4", "gather, e = 8"]
LIMIT_S = 240


def kernels(e):
    import torch

    from orz_amd import _native

    lib = _native.load()
    count = KERNEL_BYTES // e
    g = torch.Generator(device="cuda:0").manual_seed(e)
    inter = torch.randint(0, 256, (KERNEL_BYTES,), generator=g, dtype=torch.uint8, device="cuda:0")
    base = torch.randint(0, 256, (KERNEL_BYTES,), generator=g, dtype=torch.uint8, device="cuda:0")
    planes = torch.empty(KERNEL_BYTES, dtype=torch.uint8, device="cuda:0")  # (count is a multiple of 16: the pitch is count)
    back = torch.empty_like(inter)
    assert all(t.data_ptr() % 16 == 0 for t in (inter, base, planes, back))
    torch.cuda.synchronize()
    ms = ctypes.c_double()

    def move(buf, b, merge):
        if b is None:
            rc = lib.orz_plane_move_time(0, ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(planes.data_ptr()), count, e, merge, REPS, ctypes.byref(ms))
        else:
            rc = lib.orz_plane_delta_move_time(0, ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(planes.data_ptr()), count,
                                               e, merge, REPS, ctypes.byref(ms))
        assert rc == 0, _native.last_error()
        return ms.value

    r = {"bytes": KERNEL_BYTES, "elem": e}
    if e > 1:
        r["split_ms"] = round(move(inter, None, 0), 4)
        r["merge_ms"] = round(move(back, None, 1), 4)
        exact = bool(torch.equal(inter, back))
    else:
        exact = True
    r["split_delta_ms"] = round(move(inter, base, 0), 4)
    exact = exact and bool(torch.equal(planes[:count], (inter ^ base)[0::e]))
    r["merge_delta_ms"] = round(move(back, base, 1), 4)
    exact = exact and bool(torch.equal(inter, back))
    # in place, checked and not timed: back := base, merged over itself.  The hook launches twice (the warming launch and one
    # rep): the first leaves the tensor, the second XORs the delta in again and leaves the base
    back.copy_(base)
    torch.cuda.synchronize()
    rc = lib.orz_plane_delta_move_time(0, ctypes.c_void_p(back.data_ptr()), ctypes.c_void_p(back.data_ptr()), ctypes.c_void_p(planes.data_ptr()), count, e, 1,
                                       1, ctypes.byref(ms))
    assert rc == 0, _native.last_error()
    r["in_place_twice_is_the_base"] = bool(torch.equal(back, base))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    back.copy_(inter)
    a.record()
    for _ in range(REPS):
        back.copy_(inter)
    b.record()
    torch.cuda.synchronize()
    copy_ms = a.elapsed_time(b) / REPS
    r.update(copy_ms=round(copy_ms, 4), exact=exact)
    for k in ("split", "merge"):
        if e > 1:
            r[k + "_delta_over_plain"] = round(r[k + "_delta_ms"] / r[k + "_ms"], 3)
        r[k + "_delta_over_copy"] = round(r[k + "_delta_ms"] / copy_ms, 3)
        r[k + "_delta_GBps_of_tensor"] = round(KERNEL_BYTES / r[k + "_delta_ms"] / 1e6, 1)
    return r


def gather(e):
    import torch

    from orz_amd import _native

    lib = _native.load()
    count = KERNEL_BYTES // e
    g = torch.Generator(device="cuda:0").manual_seed(10 + e)
    planes = torch.randint(0, 256, (KERNEL_BYTES,), generator=g, dtype=torch.uint8, device="cuda:0")  # plane p: bytes [p count, (p + 1) count)
    base = torch.randint(0, 256, (KERNEL_BYTES,), generator=g, dtype=torch.uint8, device="cuda:0")
    out = torch.empty(KERNEL_BYTES, dtype=torch.uint8, device="cuda:0")
    assert count % 16 == 0 and all(t.data_ptr() % 16 == 0 for t in (planes, base, out))
    torch.cuda.synchronize()
    ms = ctypes.c_double()

    def run(b, dst, reps=REPS):
        rc = lib.orz_element_gather_time(0, ctypes.c_void_p(planes.data_ptr()), ctypes.c_void_p(b.data_ptr()) if b is not None else None,
                                         ctypes.c_void_p(dst.data_ptr()), count, e, reps, ctypes.byref(ms))
        assert rc == 0, _native.last_error()
        return ms.value

    merged = planes.view(e, count).t().contiguous().view(-1)  # the interleaved bytes, in torch
    r = {"bytes": KERNEL_BYTES, "elem": e}
    r["gather_ms"] = round(run(None, out), 4)
    exact = bool(torch.equal(out, merged))
    r["gather_delta_ms"] = round(run(base, out), 4)
    exact = exact and bool(torch.equal(out, merged ^ base))
    # in place, checked and not timed: out := base, gathered over itself.  The hook launches twice (the warming launch and one rep):
    # the first leaves planes XOR base, the second XORs the planes in again and leaves the base
    out.copy_(base)
    torch.cuda.synchronize()
    run(out, out, reps=1)
    r["in_place_twice_is_the_base"] = bool(torch.equal(out, base))
    r.update(exact=exact, delta_over_plain=round(r["gather_delta_ms"] / r["gather_ms"], 3),
             gather_GBps_of_tensor=round(KERNEL_BYTES / r["gather_ms"] / 1e6, 1), gather_delta_GBps_of_tensor=round(KERNEL_BYTES / r["gather_delta_ms"] / 1e6, 1))
    return r


def step():
    import torch

    import orz_amd

    w = torch.randn(ELEMENTS, generator=torch.Generator().manual_seed(1)) * 0.02
    d = torch.randn(ELEMENTS, generator=torch.Generator().manual_seed(5))
    base = w.to(torch.bfloat16).to("cuda:0")
    tuned = (w + d * LR).to(torch.bfloat16).to("cuda:0")
    enc = orz_amd.MemberEncoder(device=0, level=1, jobs=JOBS)
    out = torch.empty(enc.bound_planes_pieces([2 * ELEMENTS], [2], PIECE)[0], dtype=torch.uint8, device="cuda:0")
    r = {"elements": ELEMENTS, "bytes": 2 * ELEMENTS, "piece_elems": PIECE, "jobs": JOBS, "lr": LR}
    for name in ("plain", "delta"):
        encode = (lambda: enc.encode_tensor_pieces([tuned], PIECE, out=out)) if name == "plain" else (lambda: enc.encode_tensor_deltas([tuned], [base], PIECE, out=out))
        encode()
        torch.cuda.synchronize()
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = encode()
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        members, elems, pieces = res[1], res[2], res[3]
        back = torch.empty_like(tuned)
        t0 = time.perf_counter()
        sizes, st = orz_amd.decode_planes_into(out, [back], device=0, members=members, elems=elems, pieces=pieces, stats=True,
                                               bases=None if name == "plain" else [base])
        wall = time.perf_counter() - t0
        r[name] = {"members": len(members), "container_bytes": sum(n for _, n in members), "encode_wall_ms": [round(x * 1e3, 2) for x in sorted(walls)],
                   "encode_median_ms": round(sorted(walls)[1] * 1e3, 2), "decode_kernel_ms": round(st["kernel_ms"], 2),
                   "decode_wall_ms": round(wall * 1e3, 2), "decode_launches": st["launches"], "host_waits": st["host_waits"],
                   "exact": sizes == [2 * ELEMENTS] and bool(torch.equal(back.view(torch.int16), tuned.view(torch.int16)))}
    enc.close()
    for k in ("container_bytes", "encode_median_ms", "decode_kernel_ms"):
        r["delta_over_plain_" + k] = round(r["delta"][k] / r["plain"][k], 3)
    return r


def run_leg(leg):
    import torch

    r = {"leg": leg}
    e = int(leg.rsplit(" ", 1)[1]) if " e = " in leg else 0
    r.update(kernels(e) if leg.startswith("kernels") else gather(e) if leg.startswith("gather") else step())
    r["device"] = torch.cuda.get_device_name(0)
    print("ROW " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "delta_bench.jsonl"))
    ap.add_argument("--leg", default="")
    ap.add_argument("--only", default="", help="run the legs whose names begin with this, and append their lines to --out")
    args = ap.parse_args()
    if args.leg:
        run_leg(args.leg)
        return
    rows = []
    if args.only and os.path.exists(args.out):
        rows = [json.loads(ln) for ln in open(args.out) if ln.strip()]
    for leg in [x for x in LEGS if x.startswith(args.only)]:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], stdout=subprocess.PIPE, text=True, timeout=LIMIT_S)
        if p.returncode != 0:  # (whatever failed on the device: nothing more is started on it)
            sys.exit("leg %r failed with status %d" % (leg, p.returncode))
        rows += [json.loads(ln[4:]) for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
        print(json.dumps(rows[-1]), flush=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
