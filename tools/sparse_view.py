"""The sparse batch on a view: auction_solve_sparse_batch fed what a device pipeline has -- int64 indices that are a
view, float32 or float64 values, offsets on the device -- against what a caller had to do before it.  On one GPU, in
one process, at the sizes of the README's sparse table (the batches of tools/sparse_batch.py).  The indices are seen
through two views:
  wide         storage (nnz, 3) int64 (b, i, j), the view is storage[:, 1:]: strides (3, 1)
  transposed   storage (2, nnz) int64, the view is storage.t(): strides (1, nnz)
Legs, interleaved within every repetition, every call with errors="status" and dims=(N, N), with and without outside:
  v    auction_solve_sparse_batch(view, val, offsets on the device)                    the view call
  y    loc.to(torch.int32).contiguous(), val.double(), offsets.cpu(), then the existing call   the yardstick
  p    the existing call on copies made beforehand                                      the existing call alone
Per leg: host_ms, the time until the call returns; total_ms, the call plus torch.cuda.synchronize().  Median and
p10 - p90 of --reps repetitions; one JSON line per (shape, view, dtype, mode, leg).  Before anything is timed the legs are
compared: the same status, sol and prices, bit for bit.  Nothing gates on speed; --table prints the README table from
the file, losses as losses.  Needs the GPU.

  python tools/sparse_view.py [--reps 30] [--out profiles/sparse_view.jsonl] [--shapes 1024x64x8,...]
  python tools/sparse_view.py --table [--out profiles/sparse_view.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def table(path):
    rows = [json.loads(x) for x in open(path)]
    by = {}
    for r in rows:
        by.setdefault((r["B"], r["N"], r["per_row"], r["view"], r["dtype"], r["mode"]), {})[r["leg"]] = r
    print("| B x N x k | view | val | mode | view call ms (p10 - p90) | host ms | yardstick ms (p10 - p90) | existing call ms | "
          "view / yardstick |")
    print("|---|---|---|---|---|---|---|---|---|")
    for (B, N, k, view, dtype, mode), legs in by.items():
        v, y, p = legs["v"], legs["y"], legs["p"]
        ratio = v["total_ms"] / y["total_ms"]
        print(f"| {B} x {N} x {k} | {view} | {dtype} | {mode} | {v['total_ms']:.3f} ({v['total_ms_p10']:.3f} - "
              f"{v['total_ms_p90']:.3f}) | {v['host_ms']:.3f} | {y['total_ms']:.3f} ({y['total_ms_p10']:.3f} - "
              f"{y['total_ms_p90']:.3f}) | {p['total_ms']:.3f} | {ratio:.2f}{' (loss)' if ratio > 1.0 else ''} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_view.jsonl"))
    ap.add_argument("--shapes", default=None, help="BxNxK,... (K = entries per row)")
    ap.add_argument("--table", action="store_true", help="print the README table from --out and leave")
    args = ap.parse_args()
    if args.table:
        return table(args.out)
    import torch
    from sparse_batch import SHAPES, batch
    from sslap_amd import auction_solve_sparse_batch
    shapes = SHAPES if not args.shapes else [tuple(int(x) for x in p.split("x")) for p in args.shapes.split(",")]
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    rows = []
    for B, N, k in shapes:
        loc, val, off = batch(B, N, k, seed=B * 7919 + N)
        nnz = len(val)
        which = np.repeat(np.arange(B), np.diff(off))
        d_off = torch.from_numpy(off).cuda()
        for view_name in ("wide", "transposed"):
            if view_name == "wide":
                store = torch.from_numpy(np.concatenate([which[:, None], loc], axis=1).astype(np.int64)).cuda()
                view = store[:, 1:]
            else:
                store = torch.from_numpy(np.ascontiguousarray(loc.T).astype(np.int64)).cuda()
                view = store.t()
            assert tuple(view.shape) == (nnz, 2) and not view.is_contiguous()
            for dtype in ("float32", "float64"):
                dv = torch.from_numpy(val.astype(dtype)).cuda()
                copy_l, copy_v = view.to(torch.int32).contiguous(), dv.double()
                for mode, own in (("status", {}), ("outside", dict(outside=50.0))):
                    kw = dict(errors="status", dims=(N, N), **own)

                    def leg(name):
                        if name == "v":
                            return auction_solve_sparse_batch(view, dv, d_off, **kw)
                        if name == "y":
                            return auction_solve_sparse_batch(view.to(torch.int32).contiguous(), dv.double(), d_off.cpu().numpy(),
                                                              **kw)
                        return auction_solve_sparse_batch(copy_l, copy_v, off, **kw)

                    legs = ["v", "y", "p"]
                    ref = leg("p")
                    for name in legs:  # the legs solve the same problems to the same bits
                        got = leg(name)
                        assert torch.equal(got["status"], ref["status"]) and torch.equal(got["sol"], ref["sol"]), name
                        assert torch.equal(got["prices"].view(torch.int64), ref["prices"].view(torch.int64)), name
                    assert not ref["status"].any()
                    times = {}
                    for r in range(-1, args.reps):  # (r = -1: the warm-up)
                        j = r % len(legs)
                        for name in legs[j:] + legs[:j]:  # (no leg always runs behind the same other)
                            sync()
                            t0 = time.perf_counter()
                            leg(name)
                            t1 = time.perf_counter()
                            sync()
                            t2 = time.perf_counter()
                            if r >= 0:
                                times.setdefault(name, []).append(((t1 - t0) * 1e3, (t2 - t0) * 1e3))
                    for name in legs:
                        t = np.array(times[name])
                        row = dict(B=B, N=N, per_row=k, view=view_name, dtype=dtype, mode=mode, leg=name, reps=len(t))
                        for c, what in enumerate(("host_ms", "total_ms")):
                            row[what] = round(float(np.median(t[:, c])), 4)
                            row[what + "_p10"] = round(float(np.percentile(t[:, c], 10)), 4)
                            row[what + "_p90"] = round(float(np.percentile(t[:, c], 90)), 4)
                        rows.append(row)
                        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
