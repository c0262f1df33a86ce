"""Gated point-set problems through candidate lists: auction_solve_points_batch(outside=, candidates=K) against the
same call without candidates, and against what a caller did for lists until now.  On one GPU, in one process.
The workload of tools/points_finish.py, cold: float32 coordinates, uniform in [-1, 1)^D with D = 3, N points on either
side, an outside value per row (the squared-distance gate) uniform in [0.5, 1.5) x 4 N^(-2/3), about the squared distance
to a near neighbour; fast=True from zero prices.  Per shape and K the legs
  b  the builder alone: points_candidates(x, y, K, limit=outside)
  n  the new call: auction_solve_points_batch(x, y, outside=, candidates=K)
  p  the yardstick: auction_solve_points_batch(x, y, outside=) -- every bid scans all N columns
  t  what a caller did for lists: the float64 stack built on the device by the definition's chain, torch.topk(-cost, K),
     the gate applied to the K kept, then auction_solve_ell_batch(cols, vals, n_cols=N, outside=) (skipped where the
     stack exceeds --stack-limit bytes)
interleaved within every repetition.  Per leg: host_ms, the time until the call returns; total_ms, the call plus
torch.cuda.synchronize(); stream_ms, everything the leg put on the stream, from events around it; peak_bytes, the peak of
torch's allocator above what was allocated before the leg.  Median and p10 - p90 of --reps repetitions; one JSON line per
(shape, K, leg).  Leg n also records truncated (problems with a truncated row, and the share of rows that took the
truncated path), gap (the mean distance per problem of its objective from leg p's) and builder_share (leg b's stream_ms
over its own).  Needs the GPU.

  python tools/points_candidates.py [--reps 30] [--coords 3] [--k 8,16] [--out profiles/points_candidates.jsonl] [--shapes 1024x64,...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 64), (1, 2048), (16, 16), (1024, 64), (256, 256), (64, 1000), (64, 2048)]  # (B, N): N points on either side


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--coords", type=int, default=3)
    ap.add_argument("--k", default="8,16")
    ap.add_argument("--stack-limit", type=float, default=2e10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_candidates.jsonl"))
    ap.add_argument("--shapes", default=None, help="BxN,...")
    args = ap.parse_args()
    import torch
    from sslap_amd import auction_solve_ell_batch, auction_solve_points_batch, points_candidates
    shapes = SHAPES if not args.shapes else [tuple(int(v) for v in p.split("x")) for p in args.shapes.split(",")]
    ks = [int(v) for v in args.k.split(",")]
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []

    def stack_of(x, y):  # the definition's chain on the device, float64
        xw, yw = x.double(), y.double()
        d = xw[:, :, None, 0] - yw[:, None, :, 0]
        c = d * d
        for k in range(1, x.shape[2]):
            d = xw[:, :, None, k] - yw[:, None, :, k]
            c = c + d * d
        return c

    for B, N in shapes:
        rng = np.random.default_rng(B * 7919 + N * 31)
        x = torch.from_numpy(rng.uniform(-1, 1, (B, N, args.coords)).astype(np.float32)).cuda()
        y = torch.from_numpy(rng.uniform(-1, 1, (B, N, args.coords)).astype(np.float32)).cuda()
        outside = torch.from_numpy(rng.uniform(0.5, 1.5, (B, N)) * 4.0 * N ** (-2.0 / 3.0)).cuda()
        kw = dict(fast=True, errors="status", outside=outside)
        with_topk = B * N * N * 8 * 3 <= args.stack_limit  # (the chain holds the stack and two temporaries)

        def leg(name, K):
            if name == "b":
                return points_candidates(x, y, K, limit=outside)
            if name == "n":
                return auction_solve_points_batch(x, y, candidates=K, **kw)
            if name == "p":
                return auction_solve_points_batch(x, y, **kw)
            cost = stack_of(x, y)
            neg, cols = torch.topk(-cost, min(K, N), dim=2)
            vals = -neg
            cols = torch.where(vals <= outside[:, :, None], cols, -1).int()  # the gate: a column beyond it is a hole
            return auction_solve_ell_batch(cols, vals.contiguous(), n_cols=N, **kw)

        for K in ks:
            legs = ["b", "n", "p"] + (["t"] if with_topk else [])
            times, peaks, gaps, trunc = {}, {}, [], []
            for r in range(-1, args.reps):  # (r = -1: the warm-up)
                k0 = r % len(legs)
                done = {}
                for name in legs[k0:] + legs[:k0]:  # (no leg always runs behind the same other)
                    sync()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    t0 = time.perf_counter()
                    ev[0].record()
                    res = leg(name, K)
                    ev[1].record()
                    t1 = time.perf_counter()
                    sync()
                    t2 = time.perf_counter()
                    done[name] = res
                    if r >= 0:
                        times.setdefault(name, []).append(((t1 - t0) * 1e3, (t2 - t0) * 1e3, ev[0].elapsed_time(ev[1])))
                        peaks.setdefault(name, []).append(torch.cuda.max_memory_allocated() - base)
                for name in legs[1:]:
                    assert not done[name]["status"].any(), name
                if r >= 0:
                    counts = done["n"]["candidates"]["counts"]
                    trunc.append((int((done["n"]["truncated"] > 0).sum()), float((counts > K).double().mean())))
                    gaps.append(float((done["n"]["meta"]["obj_f64"] - done["p"]["meta"]["obj_f64"]).abs().mean()))
                del done, res
            med = {name: float(np.median(np.array(times[name])[:, 2])) for name in legs}
            for name in legs:
                t = np.array(times[name])
                row = dict(B=B, N=N, D=args.coords, K=K, leg=name, reps=len(t), peak_bytes=int(np.max(peaks[name])))
                for k, what in enumerate(("host_ms", "total_ms", "stream_ms")):
                    row[what] = round(float(np.median(t[:, k])), 4)
                    row[what + "_p10"] = round(float(np.percentile(t[:, k], 10)), 4)
                    row[what + "_p90"] = round(float(np.percentile(t[:, k], 90)), 4)
                if name != "p":
                    row["over_p"] = round(med[name] / med["p"], 3)  # stream time over the yardstick's: < 1 is a win
                if name == "n":
                    row["truncated_problems"] = int(np.median([v[0] for v in trunc]))
                    row["truncated_row_share"] = round(float(np.median([v[1] for v in trunc])), 5)
                    row["gap"] = round(float(np.median(gaps)), 6)
                    row["builder_share"] = round(med["b"] / med["n"], 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
