"""Partial assignments from a dense (B, N, N) stack on the device: auction_solve_batch(outside=) against the route a caller
had to take before it, the plain status call on an explicitly augmented (B, N, N + N) stack.  On one GPU, in one process.
The batch: uniform [0, 100) doubles (the recipe of tools/dense_batch.py), half the entries gated to -1, as a float64 device
tensor, with a float64 (B, N) device tensor of outside values drawn like the values.
Three legs, interleaved within every repetition, every solve with fast=True (what the outside mode resolves to):
  o  auction_solve_batch(mats, outside=outside, fast=True, errors="status")
  a  auction_solve_batch(aug, cardinality_check=False, fast=True, errors="status") on a stack built beforehand: column
     N + i of row i holds the row's outside value, the rest of the N x N block -1
  b  the same call, the time to build the stack (torch.cat of the stack and the block) included
Legs a and b need N + N <= 1024 (MISSLAP_DENSE_BATCH_MAX_DIM); a larger shape runs leg o alone, and the tool says so.
Per leg: host_ms, the time until the call returns; total_ms, the call plus torch.cuda.synchronize(); stream_ms, the time
of everything the leg put on the stream, from events around it.  Median and p10 - p90 of --reps repetitions; one JSON line
per (shape, leg).  Before anything is timed the legs are compared: the same assignment after the column mapping, the same
prices.  Needs the GPU.

  python tools/dense_outside.py [--reps 30] [--out profiles/dense_outside.jsonl] [--shapes 1024x64,...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP = 1024  # MISSLAP_DENSE_BATCH_MAX_DIM
SHAPES = [(1024, 64), (1024, 100), (256, 256), (64, 1000)]  # (B, N): the sizes of the README's dense table


def augment(mats, outside):
    """The (B, N, N + N) stack a caller builds by hand: the outside values on the diagonal of an N x N block of -1."""
    import torch
    B, N, _ = mats.shape
    block = torch.full((B, N, N), -1.0, dtype=mats.dtype, device=mats.device)
    block.diagonal(dim1=1, dim2=2).copy_(outside)
    return torch.cat([mats, block], dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_outside.jsonl"))
    ap.add_argument("--shapes", default=None, help="BxN,...")
    args = ap.parse_args()
    import torch
    from sslap_amd import auction_solve_batch
    shapes = SHAPES if not args.shapes else [tuple(int(x) for x in p.split("x")) for p in args.shapes.split(",")]
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    for B, N in shapes:
        rng = np.random.default_rng(B * 7919 + N)
        host = rng.uniform(0.0, 100.0, (B, N, N))
        host[rng.random((B, N, N)) < 0.5] = -1.0
        mats = torch.from_numpy(host).cuda()
        outside = torch.from_numpy(rng.uniform(0.0, 100.0, (B, N))).cuda()
        old = 2 * N <= CAP
        if not old:
            print(f"# {B} x {N}: the augmented stack would have {2 * N} columns, beyond the cap of {CAP}: legs a and b are "
                  f"impossible, leg o runs alone", flush=True)
        aug = augment(mats, outside) if old else None
        plain = dict(cardinality_check=False, fast=True, errors="status")

        def leg(name):
            if name == "a":
                return auction_solve_batch(aug, **plain)
            if name == "b":
                return auction_solve_batch(augment(mats, outside), **plain)
            return auction_solve_batch(mats, outside=outside, fast=True, errors="status")

        ref = leg("o")
        assert not ref["status"].any()
        unmatched = float((ref["sol"] < 0).double().mean())
        legs = ["o", "a", "b"] if old else ["o"]
        for name in legs[1:]:  # the legs solve the same problems to the same bits
            got = leg(name)
            assert not got["status"].any(), name
            assert torch.equal(torch.where(got["sol"] >= N, -1, got["sol"]), ref["sol"]), name
            assert torch.equal(got["prices"][:, :N].view(torch.int64), ref["prices"].view(torch.int64)), name
            assert torch.equal(got["prices"][:, N:].contiguous().view(torch.int64),
                               ref["outside_prices"].view(torch.int64)), name
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
            row = dict(B=B, N=N, leg=name, reps=len(t), unmatched=round(unmatched, 4))
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
