"""dev: what a read of byte ranges costs (orz_amd.MemberReader) beside the whole decode -- 1 GiB of the text workload in 16
members of 64 MiB, encoded on the GPU and left in HBM.  One JSON line per leg into the file named by --out (default
profiles/range_read_bench.jsonl): the whole decode (orz_decode_members_to_device), 16 ranges of 1 MiB at the members' starts,
the same at their ends, one range in the middle of member 7, 4,096 seeded ranges of 4 KiB.  Short legs run three times
after a warm-up read, long ones once; every leg's bytes are compared with the input on the device."""
import argparse
import json
import os
import random
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
sys.path.insert(0, os.getcwd())
sys.path.insert(0, "tools")
import torch  # noqa: E402

import corpus  # noqa: E402
import orz_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "range_read_bench.jsonl"))
ap.add_argument("--members", type=int, default=16)
ap.add_argument("--mib", type=int, default=64)
args = ap.parse_args()
MB, M = args.mib << 20, args.members
base = corpus.enwik_like(100_000_000)
data = (base * (M * MB // len(base) + 1))[: M * MB]
src = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
del data, base
cap = M * orz_amd.stream_bound(MB)
streams = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
enc = orz_amd.MemberEncoder(device=0, level=1, jobs=8)
members = enc.encode_to_device(src.data_ptr(), src.numel(), streams.data_ptr(), cap, member_bytes=MB)
enc.close()
rows = []


def put(row):
    rows.append(row)
    print(json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


put({"leg": "container", "members": len(members), "member_MiB": args.mib, "decoded_bytes": src.numel(),
     "container_bytes": sum(ln for _, ln in members), "device": torch.cuda.get_device_name(0)})
rd = orz_amd.MemberReader(streams, members=members)
rd.read(0, 4096)  # warm-up: buffers, the kernels' code


def leg(name, ranges, times):
    runs = []
    for _ in range(times):
        out, st = rd.read_ranges(ranges, stats=True)
        ok = bool(torch.equal(out, torch.cat([src[o:o + ln] for o, ln in ranges])))
        runs.append((st, ok))
        del out
    k = sorted(s["kernel_ms"] for s, _ in runs)
    st = runs[0][0]
    put({"leg": name, "ranges": len(ranges), "runs": times, "exact": all(ok for _, ok in runs), "kernel_ms": [round(x, 2) for x in k],
         "gather_ms": sorted(round(s["gather_ms"], 3) for s, _ in runs), "total_s": sorted(round(s["total_s"], 4) for s, _ in runs),
         "outside_kernel_ms": sorted(round(s["total_s"] * 1e3 - s["kernel_ms"], 3) for s, _ in runs),
         "members_decoded": st["members_decoded"], "decoded_bytes": st["decoded_bytes"], "out_bytes": st["out_bytes"],
         "launches": st["launches"], "host_waits": st["host_waits"]})
    return k[len(k) // 2]


start = leg("16 x 1 MiB at the members' starts", [(m * MB, 1 << 20) for m in range(M)], 3)
out, n, st = orz_amd.decode_members_to_device(streams, members=members, stats=True)
whole = st["kernel_ms"]
put({"leg": "whole decode (orz_decode_members_to_device)", "exact": bool(torch.equal(out, src)), "kernel_ms": [round(whole, 2)],
     "total_s": [round(st["total_s"], 4)], "launches": st["launches"], "out_bytes": st["out_bytes"]})
del out
mid = leg("1 MiB in the middle of member %d" % min(7, M - 1), [(min(7, M - 1) * MB + MB // 2 - (1 << 19), 1 << 20)], 1)
end = leg("16 x 1 MiB at the members' ends", [((m + 1) * MB - (1 << 20), 1 << 20) for m in range(M)], 1)
rng = random.Random(2026)
many = leg("4096 x 4 KiB, seeded", [(rng.randrange(0, M * MB - 4096), 4096) for _ in range(4096)], 1)
put({"leg": "ratios", "starts_over_whole": round(start / whole, 5), "middle_over_whole": round(mid / whole, 4),
     "ends_over_whole": round(end / whole, 4), "many_over_whole": round(many / whole, 4)})
rd.close()
