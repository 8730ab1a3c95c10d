"""dev: what cutting the planes of a large tensor into pieces buys and costs (orz_planes.h, orz_read_elements.h).  Two tensors --
bf16 randn * 0.02 of 2^22 elements (seed 1) and int64 sorted ids of 2^20 elements (seed 2) -- each at piece sizes of 0 (planes
whole: the path without pieces), 2^16, 2^18 and 2^20 elements.  One process, each case once after one warm-up of the kernels on
a small tensor.  One JSON line per case into --out (default profiles/plane_pieces.jsonl):

  container_bytes      the members' streams together: each piece restarts the model
  encode_s             wall time of encode_tensor_pieces
  decode_kernel_ms     decode_planes_into of the whole tensor: kernel_ms
  tail_kernel_ms       a cold read_tensor (a fresh reader, no cache) of the last eighth of the tensor: kernel_ms
  tail_members, tail_decoded_bytes   what that read decoded

and each of the four against the same tensor's row without pieces (`*_ratio`).  Every case's bytes are compared with the tensor."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
sys.path.insert(0, os.getcwd())

PIECES = (0, 1 << 16, 1 << 18, 1 << 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "plane_pieces.jsonl"))
    args = ap.parse_args()
    import torch

    import orz_amd

    g = torch.Generator().manual_seed(1)
    weights = (torch.randn(1 << 22, generator=g) * 0.02).to(torch.bfloat16).to("cuda:0")
    g = torch.Generator().manual_seed(2)
    ids = torch.sort(torch.randint(0, 1 << 40, (1 << 20,), generator=g, dtype=torch.int64)).values.to("cuda:0")
    enc = orz_amd.MemberEncoder(device=0, level=1, jobs=4)
    rows = []

    def run(name, t, piece_elems):
        n = t.numel()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        container, members, elems, pieces = enc.encode_tensor_pieces([t], piece_elems)
        encode_s = time.perf_counter() - t0
        back = torch.empty_like(t)
        _, st = orz_amd.decode_planes_into(container, [back], device=0, members=members, pieces=pieces, stats=True)
        exact = bool(torch.equal(back.view(torch.uint8), t.view(torch.uint8)))
        rd = orz_amd.MemberReader(container, device=0, members=members, elems=elems, pieces=pieces)
        first = n - n // 8
        got, rs = rd.read_elements([(0, first, n // 8)], stats=True)
        rd.close()
        exact = exact and bool(torch.equal(got, t[first:].view(torch.uint8).reshape(-1)))
        return {"tensor": name, "elements": n, "elem": t.element_size(), "piece_elems": piece_elems, "pieces": pieces[0], "members": len(members),
                "container_bytes": sum(ln for _, ln in members), "encode_s": round(encode_s, 4), "decode_kernel_ms": round(st["kernel_ms"], 2),
                "decode_launches": st["launches"], "decode_host_waits": st["host_waits"], "tail_kernel_ms": round(rs["kernel_ms"], 2),
                "tail_members": rs["members_decoded"], "tail_decoded_bytes": rs["decoded_bytes"], "tail_host_waits": rs["host_waits"], "exact": exact}

    run("warm-up", weights[:1 << 12].contiguous(), 1 << 10)
    for name, t in (("bf16 randn * 0.02", weights), ("int64 sorted ids", ids)):
        base = None
        for piece_elems in PIECES:
            r = run(name, t, piece_elems)
            base = base or r
            for key in ("container_bytes", "encode_s", "decode_kernel_ms", "tail_kernel_ms"):
                r[key.replace("_bytes", "").replace("_s", "").replace("_ms", "") + "_ratio"] = round(r[key] / base[key], 4) if base[key] else None
            r["device"] = torch.cuda.get_device_name(0)
            rows.append(r)
            print(json.dumps(r), flush=True)
            os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
            with open(args.out, "w") as f:
                for x in rows:
                    f.write(json.dumps(x) + "\n")
    enc.close()
    assert all(r["exact"] for r in rows), "a case's bytes differ from its tensor"


if __name__ == "__main__":
    main()
