"""Assignment problems between two point sets on the device: auction_solve_points_batch, which forms the costs
|x_i - y_j|^2 from the coordinates, against what a caller does without it, the float64 (B, N, N) cost stack built on the
device and auction_solve_batch.  On one GPU, in one process.
The batch: float32 coordinates, uniform in [-1, 1)^D with D = 3, N points on either side; the reference's eps-scaling
(fast=False), errors="status".
Three legs, interleaved within every repetition:
  p  auction_solve_points_batch(x, y, errors="status")
  y  the yardstick, at this same commit: the stack built by the definition's formula (points_to_dense in torch: widen,
     subtract, square, add, one coordinate after the other), then auction_solve_batch(cost, cardinality_check=False,
     errors="status") -- every pair is an edge, so a caller who knows that skips the matching guard
  d  the same dense call on a stack built beforehand: separates the build from the solve
Legs y and d need N <= 1024 (MISSLAP_DENSE_BATCH_MAX_DIM); a larger shape runs leg p alone, and the tool says so.
Per leg: host_ms, the time until the call returns; total_ms, the call plus torch.cuda.synchronize(); stream_ms, the time
of everything the leg put on the stream, from events around it.  Median and p10 - p90 of --reps repetitions; one JSON
line per (shape, leg), with peak_bytes, torch.cuda.max_memory_allocated of one run of the leg above what was allocated
before it (leg d: the stack counts as given).  Before anything is timed the legs are compared: the same sol, prices and
records, bit for bit.  Needs the GPU.

  python tools/points_batch.py [--reps 30] [--out profiles/points_batch.jsonl] [--shapes 1024x64,...] [--coords 3]
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
SHAPES = [(1024, 64), (1024, 100), (256, 256), (64, 1000), (64, 2048)]  # (B, N)


def build(x, y):
    """points_to_dense on the device: every operation a separately rounded float64 operation, in the definition's order."""
    xw, yw = x.double(), y.double()
    d = xw[:, :, None, 0] - yw[:, None, :, 0]
    c = d * d
    for k in range(1, x.shape[2]):
        d = xw[:, :, None, k] - yw[:, None, :, k]
        c = c + d * d
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_batch.jsonl"))
    ap.add_argument("--shapes", default=None, help="BxN,...")
    ap.add_argument("--coords", type=int, default=3)
    args = ap.parse_args()
    import torch
    from sslap_amd import auction_solve_batch, auction_solve_points_batch
    shapes = SHAPES if not args.shapes else [tuple(int(v) for v in p.split("x")) for p in args.shapes.split(",")]
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    for B, N in shapes:
        rng = np.random.default_rng(B * 7919 + N)
        x = torch.from_numpy(rng.uniform(-1, 1, (B, N, args.coords)).astype(np.float32)).cuda()
        y = torch.from_numpy(rng.uniform(-1, 1, (B, N, args.coords)).astype(np.float32)).cuda()
        old = N <= CAP
        if not old:
            print(f"# {B} x {N}: beyond the dense batch's cap of {CAP}: legs y and d are impossible, leg p runs alone",
                  flush=True)
        cost = build(x, y) if old else None
        dense = dict(cardinality_check=False, errors="status")

        def leg(name):
            if name == "d":
                return auction_solve_batch(cost, **dense)
            if name == "y":
                return auction_solve_batch(build(x, y), **dense)
            return auction_solve_points_batch(x, y, errors="status")

        legs = ["p", "y", "d"] if old else ["p"]
        ref = leg("p")
        assert not ref["status"].any()
        for name in legs[1:]:  # the legs solve the same problems to the same bits
            got = leg(name)
            assert not got["status"].any(), name
            assert torch.equal(got["sol"], ref["sol"]), name
            assert torch.equal(got["prices"].view(torch.int64), ref["prices"].view(torch.int64)), name
            for key, field in ref["meta"].items():
                assert torch.equal(got["meta"][key], field), (name, key)
        sync()
        its = ref["meta"]["its"].double()
        peak = {}
        for name in legs:
            got = None
            sync()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            got = leg(name)
            sync()
            peak[name] = int(torch.cuda.max_memory_allocated() - base)
            del got
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
            row = dict(B=B, N=N, D=args.coords, leg=name, reps=len(t), its_mean=round(float(its.mean()), 1),
                       its_max=int(its.max()), peak_bytes=peak[name])
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
