"""dev: what byte planes cost and buy (orz_planes.h).  Five legs, each once, in a child process of its own under its own time limit,
one JSON line per leg into --out (default profiles/planes_bench.jsonl):

  kernels, e = 2 / 4 / 8   PlaneSplit and PlaneMerge over ONE tensor of 256 MiB at a 16-aligned address (orz_plane_move_time: events
                           around 5 launches after a warming one) beside a device-to-device copy of the same 256 MiB in the same
                           process (Tensor.copy_, events around 5 copies after a warming one).  The kernels move the same bytes
                           each way as the copy; the target is at most 1.5 x the copy's time.  The merge's output is checked.
  fp32 16 MiB, whole       randn * 0.02 through encode_tensors / decode_members_into: container size, encode wall time (median of
                           3 after a warm-up), the decode's kernel_ms (one decode: a 16 MiB member takes seconds)
  fp32 16 MiB, planes      the same tensor through encode_tensor_planes / decode_planes_into"""
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
TENSOR_BYTES, JOBS = 16 << 20, 4
LEGS = ["kernels, e = 2", "kernels, e = 4", "kernels, e = 8", "fp32 16 MiB, whole", "fp32 16 MiB, planes"]
LIMIT_S = 240


def kernels(e):
    import torch

    from orz_amd import _native

    lib = _native.load()
    count = KERNEL_BYTES // e
    g = torch.Generator(device="cuda:0").manual_seed(e)
    inter = torch.randint(0, 256, (KERNEL_BYTES,), generator=g, dtype=torch.uint8, device="cuda:0")
    planes = torch.empty(KERNEL_BYTES, dtype=torch.uint8, device="cuda:0")  # (count is a multiple of 16: the pitch is count)
    back = torch.empty_like(inter)
    assert inter.data_ptr() % 16 == 0 and planes.data_ptr() % 16 == 0 and back.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    ms = ctypes.c_double()

    def move(buf, merge):
        rc = lib.orz_plane_move_time(0, ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(planes.data_ptr()), count, e, merge, REPS, ctypes.byref(ms))
        assert rc == 0, _native.last_error()
        return ms.value

    split_ms = move(inter, 0)
    merge_ms = move(back, 1)
    exact = bool(torch.equal(inter, back)) and bool(torch.equal(planes[:count], inter[0::e]))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    back.copy_(inter)
    a.record()
    for _ in range(REPS):
        back.copy_(inter)
    b.record()
    torch.cuda.synchronize()
    copy_ms = a.elapsed_time(b) / REPS
    return {"bytes": KERNEL_BYTES, "elem": e, "split_ms": round(split_ms, 4), "merge_ms": round(merge_ms, 4), "copy_ms": round(copy_ms, 4),
            "split_over_copy": round(split_ms / copy_ms, 3), "merge_over_copy": round(merge_ms / copy_ms, 3),
            "split_GBps_each_way": round(KERNEL_BYTES / split_ms / 1e6, 1), "merge_GBps_each_way": round(KERNEL_BYTES / merge_ms / 1e6, 1),
            "copy_GBps_each_way": round(KERNEL_BYTES / copy_ms / 1e6, 1), "exact": exact}


def tensor(planes):
    import torch

    import orz_amd

    g = torch.Generator().manual_seed(3)
    t = (torch.randn(TENSOR_BYTES // 4, generator=g) * 0.02).to("cuda:0")
    enc = orz_amd.MemberEncoder(device=0, level=1, jobs=JOBS)
    out = torch.empty(max(enc.bound_planes([TENSOR_BYTES], [4]), enc.bound_segments([TENSOR_BYTES])), dtype=torch.uint8, device="cuda:0")
    encode = (lambda: enc.encode_tensor_planes([t], out=out)) if planes else (lambda: enc.encode_tensors([t], out=out))
    encode()
    torch.cuda.synchronize()
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = encode()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    members = res[1]
    back = torch.empty_like(t)
    decode = orz_amd.decode_planes_into if planes else orz_amd.decode_members_into
    t0 = time.perf_counter()
    sizes, st = decode(out, [back], device=0, members=members, stats=True)
    wall = time.perf_counter() - t0
    enc.close()
    return {"bytes": TENSOR_BYTES, "jobs": JOBS, "members": len(members), "container_bytes": sum(n for _, n in members),
            "encode_wall_ms": [round(w * 1e3, 2) for w in sorted(walls)], "encode_median_ms": round(sorted(walls)[1] * 1e3, 2),
            "decode_kernel_ms": round(st["kernel_ms"], 2), "decode_wall_ms": round(wall * 1e3, 2), "decode_launches": st["launches"],
            "host_waits": st["host_waits"], "exact": sizes == [TENSOR_BYTES] and bool(torch.equal(back, t))}


def run_leg(leg):
    import torch

    r = {"leg": leg}
    r.update(kernels(int(leg.rsplit(" ", 1)[1])) if leg.startswith("kernels") else tensor(leg.endswith("planes")))
    r["device"] = torch.cuda.get_device_name(0)
    print("ROW " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "planes_bench.jsonl"))
    ap.add_argument("--leg", default="")
    args = ap.parse_args()
    if args.leg:
        run_leg(args.leg)
        return
    rows = []
    for leg in LEGS:
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
