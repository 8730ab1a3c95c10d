"""dev: what a chain of delta links costs restored in one call (orz_chain.h: PlaneMergeChain, decode_members_chain) against the
sequential calls and the plain kernels.  ONE process, each case once after one warm-up, every result's bytes checked, one JSON line
per leg into --out (default profiles/chain_bench.jsonl):

  decode            ONE bf16 tensor of 4 Mi elements, w = randn * 0.02, and K = 4 steps of w + randn * 1e-4 each, every step a link
                    of encode_tensor_deltas against the step before at pieces of 2^18: 32 members a link, 128 in all.  The chain call
                    decode_planes_into(bases=, links=4) against the four sequential in-place decode_planes_into(bases=) calls:
                    kernel_ms, wall time and host waits of both.  The pieces table of DESIGN 9 predicts that the chain takes about
                    what the slowest single link takes; the bar is half of the sequential sum.
  merge, e = 1 / 2 / 4 / 8
                    PlaneMergeChain over ONE tensor of 256 MiB, its base and K = 1, 2, 4, 8 plane sets, all at 16-aligned addresses
                    (orz_plane_chain_move_time: events around 5 launches after a warming one); beside it PlaneMergeDelta over the
                    first plane set (orz_plane_delta_move_time) and a device-to-device copy of the 256 MiB (Tensor.copy_).  By bytes
                    moved a chain merge carries K + 2 bytes per byte of tensor where the delta merge carries 3."""
import argparse
import ctypes
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
sys.path.insert(0, os.getcwd())

KERNEL_BYTES, REPS, MERGE_LINKS = 256 << 20, 5, (1, 2, 4, 8)
ELEMENTS, PIECE, JOBS, LR, LINKS = 4 << 20, 1 << 18, 4, 1e-4, 4


def decode():
    import torch

    import orz_amd

    g = torch.Generator().manual_seed(1)
    w = torch.randn(ELEMENTS, generator=g) * 0.02
    steps = [w]
    for _ in range(LINKS):
        steps.append(steps[-1] + torch.randn(ELEMENTS, generator=g) * LR)
    steps = [s.to(torch.bfloat16).to("cuda:0") for s in steps]
    enc = orz_amd.MemberEncoder(device=0, level=1, jobs=JOBS)
    links = []
    for prev, cur in zip(steps, steps[1:]):
        container, members, elems, pieces, crcs = enc.encode_tensor_deltas([cur], [prev], PIECE, digests=True)
        links.append((container, members))
    enc.close()
    chain, table = orz_amd.join_links(links)
    last = steps[-1].view(torch.int16)
    r = {"elements": ELEMENTS, "bytes": 2 * ELEMENTS, "piece_elems": PIECE, "links": LINKS, "lr": LR, "members_a_link": len(links[0][1]),
         "members": len(table), "container_bytes": [sum(n for _, n in m) for _, m in links]}

    def chained():
        out = steps[0].clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, st = orz_amd.decode_planes_into(chain, [out], device=0, members=table, elems=elems, pieces=pieces, bases=[out], digests=crcs, links=LINKS,
                                           stats=True)
        wall = time.perf_counter() - t0
        return {"kernel_ms": round(st["kernel_ms"], 2), "wall_ms": round(wall * 1e3, 2), "host_waits": st["host_waits"], "launches": st["launches"],
                "exact": bool(torch.equal(out.view(torch.int16), last))}

    def sequential():
        out = steps[0].clone()
        torch.cuda.synchronize()
        calls, t0 = [], time.perf_counter()
        for k, (c, m) in enumerate(links):
            t1 = time.perf_counter()
            _, st = orz_amd.decode_planes_into(c, [out], device=0, members=m, elems=elems, pieces=pieces, bases=[out],
                                               digests=crcs if k == LINKS - 1 else None, stats=True)
            calls.append({"kernel_ms": round(st["kernel_ms"], 2), "wall_ms": round((time.perf_counter() - t1) * 1e3, 2), "host_waits": st["host_waits"],
                          "launches": st["launches"]})
        wall = time.perf_counter() - t0
        return {"kernel_ms": round(sum(c["kernel_ms"] for c in calls), 2), "wall_ms": round(wall * 1e3, 2), "host_waits": sum(c["host_waits"] for c in calls),
                "calls": calls, "exact": bool(torch.equal(out.view(torch.int16), last))}

    for name, leg in (("sequential", sequential), ("chain", chained)):
        leg()  # the warm-up
        r[name] = leg()
    r["chain_over_sequential_kernel_ms"] = round(r["chain"]["kernel_ms"] / r["sequential"]["kernel_ms"], 3)
    r["chain_over_slowest_link_kernel_ms"] = round(r["chain"]["kernel_ms"] / max(c["kernel_ms"] for c in r["sequential"]["calls"]), 3)
    r["chain_over_sequential_wall_ms"] = round(r["chain"]["wall_ms"] / r["sequential"]["wall_ms"], 3)
    r["below_half_of_the_sequential_sum"] = r["chain"]["kernel_ms"] < 0.5 * r["sequential"]["kernel_ms"]
    return r


def merge(e):
    import torch

    from orz_amd import _native

    lib = _native.load()
    count, kmax = KERNEL_BYTES // e, max(MERGE_LINKS)
    g = torch.Generator(device="cuda:0").manual_seed(20 + e)
    planes = torch.randint(0, 256, (kmax * KERNEL_BYTES,), generator=g, dtype=torch.uint8, device="cuda:0")  # (count is a multiple of 16: the pitch is count)
    base = torch.randint(0, 256, (KERNEL_BYTES,), generator=g, dtype=torch.uint8, device="cuda:0")
    out = torch.empty(KERNEL_BYTES, dtype=torch.uint8, device="cuda:0")
    assert count % 16 == 0 and all(t.data_ptr() % 16 == 0 for t in (planes, base, out))
    torch.cuda.synchronize()
    ms = ctypes.c_double()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    want = base.clone()
    r = {"bytes": KERNEL_BYTES, "elem": e, "exact": True}
    rc = lib.orz_plane_delta_move_time(0, ptr(out), ptr(base), ptr(planes), count, e, 1, REPS, ctypes.byref(ms))
    assert rc == 0, _native.last_error()
    r["merge_delta_ms"] = round(ms.value, 4)
    done = 0
    for K in MERGE_LINKS:
        rc = lib.orz_plane_chain_move_time(0, ptr(out), ptr(base), ptr(planes), count, e, K, REPS, ctypes.byref(ms))
        assert rc == 0, _native.last_error()
        r["merge_chain_ms_K%d" % K] = round(ms.value, 4)
        for k in range(done, K):  # the interleaved bytes of link k, in torch
            want ^= planes[k * KERNEL_BYTES:(k + 1) * KERNEL_BYTES].view(e, count).t().contiguous().view(-1)
        done = K
        r["exact"] = r["exact"] and bool(torch.equal(out, want))
        r["chain_over_delta_K%d" % K] = round(ms.value / r["merge_delta_ms"], 3)
        r["by_bytes_K%d" % K] = round((K + 2) / 3, 3)
        r["GBps_moved_K%d" % K] = round((K + 2) * KERNEL_BYTES / ms.value / 1e6, 1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out.copy_(base)
    a.record()
    for _ in range(REPS):
        out.copy_(base)
    b.record()
    torch.cuda.synchronize()
    r["copy_ms"] = round(a.elapsed_time(b) / REPS, 4)
    return r


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "chain_bench.jsonl"))
    args = ap.parse_args()
    rows = []
    for leg, run in [("decode", decode)] + [("merge, e = %d" % e, (lambda e=e: merge(e))) for e in (1, 2, 4, 8)]:
        r = {"leg": leg}
        r.update(run())
        r["device"] = torch.cuda.get_device_name(0)
        rows.append(r)
        print(json.dumps(r), flush=True)
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
    if not all(r["exact"] if "exact" in r else r["chain"]["exact"] and r["sequential"]["exact"] for r in rows):
        sys.exit("a result's bytes are wrong")


if __name__ == "__main__":
    main()
