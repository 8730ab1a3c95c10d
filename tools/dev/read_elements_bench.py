"""dev: what a read of element ranges of a plane-encoded tensor costs (orz_read_elements.h).  One bf16 tensor of 2^20 elements
(randn * 0.02, seed 1): two planes of 1 MiB.  One JSON line per case into --out (default profiles/read_elements.jsonl):

  whole, decode_planes_into   the whole tensor by the one-shot driver: kernel_ms
  whole, read_tensor          the whole tensor through a MemberReader: kernel_ms, gather_ms
  first eighth, read_tensor   elements [0, 2^17): kernel_ms, decoded_bytes
  walk, 8 windows, cursors    the tensor in eight windows under a budget for both planes: decoded_bytes and kernel_ms, summed
  PlaneMerge alone            orz_plane_move_time for the same tensor: the merge of decode_planes_into, for scale beside gather_ms

Every case's bytes are compared with the tensor.  Nothing is asserted about the times."""
import argparse
import ctypes
import json
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
sys.path.insert(0, os.getcwd())

COUNT = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "read_elements.jsonl"))
    args = ap.parse_args()
    import torch

    import orz_amd
    from orz_amd import _native

    g = torch.Generator().manual_seed(1)
    t = (torch.randn(COUNT, generator=g) * 0.02).to(torch.bfloat16).to("cuda:0")
    enc = orz_amd.MemberEncoder(device=0, level=1, jobs=2)
    container, members, elems = enc.encode_tensor_planes([t])
    enc.close()
    rows = []

    def row(case, **fields):
        r = {"case": case, "elements": COUNT, "elem": 2, "container_bytes": sum(n for _, n in members)}
        r.update(fields)
        r["device"] = torch.cuda.get_device_name(0)
        rows.append(r)
        print(json.dumps(r), flush=True)
        with open(args.out, "w") as f:
            for x in rows:
                f.write(json.dumps(x) + "\n")

    back = torch.empty_like(t)
    _, st = orz_amd.decode_planes_into(container, [back], device=0, members=members, stats=True)
    row("whole, decode_planes_into", kernel_ms=round(st["kernel_ms"], 2), launches=st["launches"], host_waits=st["host_waits"],
        exact=bool(torch.equal(back, t)))

    rd = orz_amd.MemberReader(container, device=0, members=members, elems=elems)
    got, st = rd.read_elements([(0, 0, COUNT)], stats=True)
    row("whole, read_tensor", kernel_ms=round(st["kernel_ms"], 2), gather_ms=round(st["gather_ms"], 4), decoded_bytes=st["decoded_bytes"],
        launches=st["launches"], host_waits=st["host_waits"], exact=bool(torch.equal(got.view(torch.bfloat16), t)))
    got, st = rd.read_elements([(0, 0, COUNT // 8)], stats=True)
    row("first eighth, read_tensor", kernel_ms=round(st["kernel_ms"], 2), gather_ms=round(st["gather_ms"], 4), decoded_bytes=st["decoded_bytes"],
        launches=st["launches"], host_waits=st["host_waits"], exact=bool(torch.equal(got.view(torch.bfloat16), t[:COUNT // 8])))

    rd.set_cache(2 * ((COUNT + 255) // 256 * 256 + orz_amd.MemberReader.cursor_state_bytes()))
    step, kernel, gather, decoded, exact, per = COUNT // 8, 0.0, 0.0, 0, True, []
    for k in range(8):
        got, st = rd.read_elements([(0, k * step, step)], stats=True)
        kernel += st["kernel_ms"]
        gather += st["gather_ms"]
        decoded += st["decoded_bytes"]
        per.append(round(st["kernel_ms"], 2))
        exact = exact and bool(torch.equal(got.view(torch.bfloat16), t[k * step:(k + 1) * step])) and st["host_waits"] == 2
    row("walk, 8 windows, cursors", kernel_ms=round(kernel, 2), kernel_ms_per_window=per, gather_ms=round(gather, 4), decoded_bytes=decoded, exact=exact)
    rd.close()

    planes = torch.empty(2 * COUNT, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ms = ctypes.c_double()
    lib = _native.load()
    rc = lib.orz_plane_move_time(0, ctypes.c_void_p(back.data_ptr()), ctypes.c_void_p(planes.data_ptr()), COUNT, 2, 1, 5, ctypes.byref(ms))
    assert rc == 0, _native.last_error()
    row("PlaneMerge alone", merge_ms=round(ms.value, 4))


if __name__ == "__main__":
    main()
