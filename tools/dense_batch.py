"""Many small dense problems: three ways of solving the same stack, on one GPU, in one process.
  loop   a loop of auction_solve(mat=...)
  batch  solve_batch over from_matrix handles (handle creation and the matching guard included)
  dense  auction_solve_batch (one launch, one workgroup per problem)
Matrices follow the reference's benchmarking.py recipes: uniform [0, 100) doubles ("float") and integers 1..99 ("int"),
fully dense.  Each path is timed with the cardinality check on and off: wall time of the whole call with a device
synchronise, and for `dense` the kernel time from HIP events.  One JSON line per (point, recipe, check, path).  The
results of the three paths are compared problem by problem before anything is timed.  Needs the GPU.

  python tools/dense_batch.py [--reps 5] [--out profiles/dense_batch.jsonl] [--points 1x10,1024x64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS = ((1, 10), (1, 100), (1, 300), (1024, 64), (1024, 100), (256, 256), (64, 1000))


def stack(B, N, recipe, seed):
    rng = np.random.default_rng(seed)
    if recipe == "int":
        return rng.integers(1, 100, (B, N, N)).astype(np.float64)
    return rng.uniform(0.0, 100.0, (B, N, N))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_batch.jsonl"))
    ap.add_argument("--points", default=None, help="BxN,BxN,...")
    ap.add_argument("--loop-max", type=int, default=256, help="time the per-problem paths on at most so many problems")
    args = ap.parse_args()
    import torch
    from sslap_amd import AuctionSolver, auction_solve, auction_solve_batch, from_matrix
    points = POINTS if not args.points else [tuple(int(x) for x in p.split("x")) for p in args.points.split(",")]
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    rows = []
    for B, N in points:
        for recipe in ("float", "int"):
            mats = stack(B, N, recipe, seed=B * 7919 + N)
            Bl = min(B, args.loop_max)  # the per-problem paths: on the first Bl problems, scaled per problem
            for check in (True, False):
                kw = dict(problem="min", cardinality_check=check)
                res = auction_solve_batch(mats, **kw)  # warm-up + parity
                for b in range(Bl):
                    ref = auction_solve(mat=mats[b], **kw)
                    assert np.array_equal(ref["sol"], res["sol"][b]) and ref["meta"]["its"] == res["meta"]["its"][b]
                timings = {}
                for path in ("loop", "batch", "dense"):
                    ts, ks = [], []
                    for _ in range(args.reps):
                        sync()
                        t0 = time.perf_counter()
                        if path == "loop":
                            for b in range(Bl):
                                auction_solve(mat=mats[b], **kw)
                        elif path == "batch":
                            AuctionSolver.solve_batch([from_matrix(mats[b], **kw) for b in range(Bl)])
                        else:
                            r = auction_solve_batch(mats, **kw)
                            ks.append(r["meta"]["gpu"]["kernel_ms"])
                        sync()
                        ts.append((time.perf_counter() - t0) * 1e3)
                    nprob = B if path == "dense" else Bl
                    wall = float(np.median(ts))
                    row = dict(B=B, N=N, recipe=recipe, cardinality_check=check, path=path, problems_timed=nprob,
                               wall_ms=round(wall, 4), wall_ms_per_problem=round(wall / nprob, 5),
                               problems_per_s=round(nprob / (wall * 1e-3), 1), reps=args.reps,
                               its_mean=round(float(np.mean(res["meta"]["its"])), 1))
                    if ks:
                        row["kernel_ms"] = round(float(np.median(ks)), 4)
                        row["threads"] = r["meta"]["gpu"]["threads"]
                        row["lds_bytes"] = r["meta"]["gpu"]["lds_bytes"]
                        row["check_ms"] = round(r["meta"]["gpu"]["check_ms"], 4)
                        row["matching_ms"] = round(r["meta"]["gpu"]["matching_ms"], 4)
                    timings[path] = row["problems_per_s"]
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                print(json.dumps(dict(B=B, N=N, recipe=recipe, cardinality_check=check,
                                      dense_vs_batch=round(timings["dense"] / timings["batch"], 2),
                                      dense_vs_loop=round(timings["dense"] / timings["loop"], 2))), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
