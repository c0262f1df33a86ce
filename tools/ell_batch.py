"""Padded candidate lists (B, N, K) on the device: the packed sparse batch against the ELL batch, on one GPU, in one process.
The batch is that of tools/sparse_batch.py at its four batch sizes (N x N problems, K distinct columns per row, one of
them from a planted perfect matching, uniform [0, 100) doubles), held as cols int64 (B, N, K) / vals (B, N, K) device
tensors, the way torch.topk leaves them.  Three legs, interleaved within every repetition, cardinality check on:
  a  auction_solve_sparse_batch(errors="status", dims=(N, N)) on a packed copy (loc, val, offsets) built beforehand
  b  the same call, the time to build loc / val / offsets from the (B, N, K) tensors included: what a caller does today
     (a mask, a compaction, the casts, and the per-problem counts read back for the host offsets)
  c  auction_solve_ell_batch(cols, vals, n_cols=N, errors="status")
Per leg: host_ms, the time until the call returns; total_ms, the call plus torch.cuda.synchronize(); stream_ms, the time
of everything the leg put on the stream, from events around it (for a and c: the check pass, the guard and the solve).
Median and p10 - p90 of --reps repetitions; one JSON line per (shape, leg).  Before anything is timed the three legs
are compared: identical sol, prices and status.  Needs the GPU.

  python tools/ell_batch.py [--reps 30] [--float32] [--out profiles/ell_batch.jsonl] [--shapes 1024x64x8,...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sparse_batch import SHAPES, batch  # noqa: E402

ELL_SHAPES = tuple(s for s in SHAPES if s[0] > 1)  # 1024 x 64 x 8, 1024 x 256 x 8, 256 x 1024 x 16, 64 x 2048 x 16


def pack_on_device(cols, vals):
    """(B, N, K) device tensors -> loc int32 (nnz, 2), val float64 (nnz,) on the device and offsets on the host."""
    import torch
    valid = cols >= 0
    counts = valid.sum(dim=(1, 2))
    offsets = np.concatenate([[0], np.cumsum(counts.cpu().numpy())]).astype(np.int64)  # (the read-back)
    _, i, _ = valid.nonzero(as_tuple=True)
    loc = torch.stack([i, cols[valid]], dim=1).to(torch.int32)
    return loc, vals[valid].double(), offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--float32", action="store_true", help="vals as float32 (values rounded to it for every leg)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ell_batch.jsonl"))
    ap.add_argument("--shapes", default=None, help="BxNxK,...")
    args = ap.parse_args()
    import torch
    from sslap_amd import auction_solve_ell_batch, auction_solve_sparse_batch
    shapes = ELL_SHAPES if not args.shapes else [tuple(int(x) for x in p.split("x")) for p in args.shapes.split(",")]
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    for B, N, K in shapes:
        loc, val, _ = batch(B, N, K, seed=B * 7919 + N)
        if args.float32:
            val = val.astype(np.float32)
        cols = torch.from_numpy(loc[:, 1].astype(np.int64).reshape(B, N, K)).cuda()
        vals = torch.from_numpy(val.reshape(B, N, K)).cuda()
        st = dict(errors="status", dims=(N, N))
        dl, dv, off = pack_on_device(cols, vals)

        def leg(name):
            if name == "a":
                return auction_solve_sparse_batch(dl, dv, off, **st)
            if name == "b":
                return auction_solve_sparse_batch(*pack_on_device(cols, vals), **st)
            return auction_solve_ell_batch(cols, vals, n_cols=N, errors="status")

        ref = leg("a")
        for name in ("b", "c"):  # the three legs solve the same problems to the same bits
            got = leg(name)
            assert not got["status"].any() and torch.equal(got["sol"], ref["sol"]), name
            assert torch.equal(got["prices"].view(torch.int64), ref["prices"].view(torch.int64)), name
        times = {}
        legs = ["a", "b", "c"]
        for r in range(-1, args.reps):  # (r = -1: the warm-up)
            for name in legs[r % 3:] + legs[:r % 3]:  # (no leg always runs behind the same other)
                sync()
                t0 = time.perf_counter()
                ev[0].record()
                leg(name)
                ev[1].record()
                t1 = time.perf_counter()
                sync()
                t2 = time.perf_counter()
                if r >= 0:
                    times.setdefault(name, []).append(((t1 - t0) * 1e3, (t2 - t0) * 1e3, ev[0].elapsed_time(ev[1])))
        for name in legs:
            t = np.array(times[name])
            row = dict(B=B, N=N, K=K, leg=name, vals="float32" if args.float32 else "float64", reps=len(t))
            for k, what in enumerate(("host_ms", "total_ms", "stream_ms")):
                row[what] = round(float(np.median(t[:, k])), 4)
                row[what + "_p10"] = round(float(np.percentile(t[:, k], 10)), 4)
                row[what + "_p90"] = round(float(np.percentile(t[:, k], 90)), 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
