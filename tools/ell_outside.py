"""Partial assignments from padded candidate lists (B, N, K) on the device: auction_solve_ell_batch(outside=) against the
route a caller had to take before it, the plain call on an explicitly augmented (B, N, K + 1) stack.  On one GPU, in one
process.  The batch is that of tools/ell_batch.py (N x N problems, K distinct columns per row, uniform [0, 100) doubles)
as cols int64 / vals float64 device tensors, with a float64 (B, N) device tensor of outside values drawn like the values.
Three legs, interleaved within every repetition, every solve with the options the outside mode resolves to (fast=True):
  o  auction_solve_ell_batch(cols, vals, n_cols=N, outside=outside, errors="status")
  a  auction_solve_ell_batch(cols_aug, vals_aug, n_cols=2 N, cardinality_check=False, fast=True, errors="status") on a
     stack built beforehand: slot K of row i holds column N + i and the row's outside value
  b  the same call, the time to build the stack (torch.cat of the columns and of the values) included
Legs a and b need N + N <= 2048; a larger shape runs leg o alone.  Per leg: host_ms, the time until the call returns;
total_ms, the call plus torch.cuda.synchronize(); stream_ms, the time of everything the leg put on the stream, from
events around it.  Median and p10 - p90 of --reps repetitions; one JSON line per (shape, leg).  Before anything is timed
the legs are compared: the same assignment after the column mapping, the same prices.  Needs the GPU.

  python tools/ell_outside.py [--reps 30] [--out profiles/ell_outside.jsonl] [--shapes 1024x64x8,...]
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
from ell_batch import ELL_SHAPES  # noqa: E402
from sparse_batch import batch  # noqa: E402

CAP = 2048  # MISSLAP_SPARSE_BATCH_MAX_DIM


def augment(cols, vals, outside):
    """The (B, N, K + 1) stack a caller builds by hand: slot K of row i is (N + i, outside[b, i])."""
    import torch
    B, N, _ = cols.shape
    extra = (N + torch.arange(N, device=cols.device, dtype=cols.dtype)).expand(B, N).unsqueeze(2)
    return torch.cat([cols, extra], dim=2), torch.cat([vals, outside.unsqueeze(2)], dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ell_outside.jsonl"))
    ap.add_argument("--shapes", default=None, help="BxNxK,...")
    args = ap.parse_args()
    import torch
    from sslap_amd import auction_solve_ell_batch
    shapes = ELL_SHAPES if not args.shapes else [tuple(int(x) for x in p.split("x")) for p in args.shapes.split(",")]
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    for B, N, K in shapes:
        loc, val, _ = batch(B, N, K, seed=B * 7919 + N)
        cols = torch.from_numpy(loc[:, 1].astype(np.int64).reshape(B, N, K)).cuda()
        vals = torch.from_numpy(val.reshape(B, N, K)).cuda()
        assert bool((cols.amax(dim=(1, 2)) == N - 1).all())  # m_b = N for every problem: the outside objects are N + i
        outside = torch.from_numpy(np.random.default_rng(B + N).uniform(0, 100, (B, N))).cuda()
        old = 2 * N <= CAP
        ac, av = augment(cols, vals, outside) if old else (None, None)
        plain = dict(n_cols=2 * N, cardinality_check=False, fast=True, errors="status")

        def leg(name):
            if name == "a":
                return auction_solve_ell_batch(ac, av, **plain)
            if name == "b":
                return auction_solve_ell_batch(*augment(cols, vals, outside), **plain)
            return auction_solve_ell_batch(cols, vals, n_cols=N, outside=outside, errors="status")

        ref = leg("o")
        assert not ref["status"].any()
        unmatched = float((ref["sol"] < 0).double().mean())
        legs = ["o", "a", "b"] if old else ["o"]
        for name in legs[1:]:  # the legs solve the same problems to the same bits
            got = leg(name)
            assert not got["status"].any(), name
            assert torch.equal(torch.where(got["sol"] >= N, -1, got["sol"]), ref["sol"]), name
            assert torch.equal(got["prices"][:, :N].view(torch.int64), ref["prices"].view(torch.int64)), name
            assert torch.equal(got["prices"][:, N:].view(torch.int64), ref["outside_prices"].view(torch.int64)), name
        times = {}
        for r in range(-1, args.reps):  # (r = -1: the warm-up)
            k = r % len(legs)
            for name in legs[k:] + legs[:k]:  # (no leg always runs behind the same other)
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
            row = dict(B=B, N=N, K=K, leg=name, reps=len(t), unmatched=round(unmatched, 4))
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
