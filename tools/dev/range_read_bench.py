"""dev: what a read of byte ranges costs (orz_amd.MemberReader) beside the whole decode -- 1 GiB of the text workload in 16
members of 64 MiB, encoded on the GPU and left in HBM.  One JSON line per leg into the file named by --out (default
profiles/range_read_bench.jsonl): the whole decode (orz_decode_members_to_device), 16 ranges of 1 MiB at the members' starts,
the same at their ends, one range in the middle of member 7, 4,096 seeded ranges of 4 KiB.  Short legs run three times
after a warm-up read, long ones once; every leg's bytes are compared with the input on the device.
Two legs for the cursor cache (MemberReader(cache_bytes=...)), each once with the cache off and once with a budget that holds the
member, per-read kernel_ms and decoded_bytes in the row: "walk" -- the first --walk-mib MiB of member 0 front to back in 1 MiB
windows (default: the whole member; without the cache that decodes n (n + 1) / 2 MiB for n windows) -- and "twice" -- one 1 MiB
range, 2 MiB into member 1, read twice.  --legs picks legs by name (starts, whole, middle, ends, many, walk, twice); the
uncached legs need nothing of the cache, so the same file measures an older library (ORZ_LIB_PATH) for comparison."""
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
ap.add_argument("--legs", default="starts,whole,middle,ends,many,walk,twice")
ap.add_argument("--walk-mib", type=int, default=0)
args = ap.parse_args()
LEGS = set(args.legs.split(","))
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


def series(name, reads, cache_bytes):
    """`reads` one after another on a reader of its own, every read's figures in one row"""
    r = orz_amd.MemberReader(streams, members=members, cache_bytes=cache_bytes) if cache_bytes else orz_amd.MemberReader(streams, members=members)
    r.read((M - 1) * MB, 4096)  # warm-up at the start of the last member, which no series reads
    per, ok = [], True
    for off, ln in reads:
        out, st = r.read(off, ln, stats=True)
        ok = ok and bool(torch.equal(out, src[off:off + ln]))
        per.append(st)
        del out
    row = {"leg": name, "cache_bytes": cache_bytes, "reads": len(reads), "exact": ok, "kernel_ms": [round(s["kernel_ms"], 2) for s in per],
           "decoded_bytes": [s["decoded_bytes"] for s in per], "host_waits": [s["host_waits"] for s in per],
           "kernel_ms_sum": round(sum(s["kernel_ms"] for s in per), 2), "decoded_bytes_sum": sum(s["decoded_bytes"] for s in per),
           "total_s_sum": round(sum(s["total_s"] for s in per), 4)}
    if cache_bytes:
        row["cache"] = r.cache_stats()
    r.close()
    put(row)


ratios = {}
if "starts" in LEGS:
    ratios["starts"] = leg("16 x 1 MiB at the members' starts", [(m * MB, 1 << 20) for m in range(M)], 3)
if "whole" in LEGS:
    out, n, st = orz_amd.decode_members_to_device(streams, members=members, stats=True)
    ratios["whole"] = st["kernel_ms"]
    put({"leg": "whole decode (orz_decode_members_to_device)", "exact": bool(torch.equal(out, src)), "kernel_ms": [round(st["kernel_ms"], 2)],
         "total_s": [round(st["total_s"], 4)], "launches": st["launches"], "out_bytes": st["out_bytes"]})
    del out
if "middle" in LEGS:
    ratios["middle"] = leg("1 MiB in the middle of member %d" % min(7, M - 1), [(min(7, M - 1) * MB + MB // 2 - (1 << 19), 1 << 20)], 1)
if "ends" in LEGS:
    ratios["ends"] = leg("16 x 1 MiB at the members' ends", [((m + 1) * MB - (1 << 20), 1 << 20) for m in range(M)], 1)
if "many" in LEGS:
    rng = random.Random(2026)
    ratios["many"] = leg("4096 x 4 KiB, seeded", [(rng.randrange(0, M * MB - 4096), 4096) for _ in range(4096)], 1)
if "whole" in ratios:
    put(dict({"leg": "ratios"}, **{k + "_over_whole": round(v / ratios["whole"], 5) for k, v in ratios.items() if k != "whole"}))
rd.close()
if "walk" in LEGS or "twice" in LEGS:
    budget = 0  # (a library without the cache: the uncached legs alone)
    if hasattr(orz_amd.MemberReader, "cursor_state_bytes"):
        budget = (MB + 255) // 256 * 256 + orz_amd.MemberReader.cursor_state_bytes()  # one member's cursor
    n_win = (args.walk_mib or args.mib)
    walk = [(k << 20, 1 << 20) for k in range(min(n_win, args.mib))]
    twice = [(min(1, M - 2) * MB + (2 << 20), 1 << 20)] * 2
    for cache_bytes in (0, budget) if budget else (0,):
        if "walk" in LEGS:
            series("member 0 front to back, %d x 1 MiB" % len(walk), walk, cache_bytes)
        if "twice" in LEGS:
            series("1 MiB, 2 MiB into member %d, read twice" % min(1, M - 2), twice, cache_bytes)
