"""Many small sparse problems: four ways of solving the same batch, on one GPU, in one process.
  loop    a loop of auction_solve(loc=..., val=...)
  batch   solve_batch over from_sparse handles (handle creation and the matching guard included)
  dense   auction_solve_batch on the densified (B, N, N) stack (-1 = no entry), where N <= 1024
  sparse  auction_solve_sparse_batch (one launch, one workgroup per problem)
Problem b is N x N with `per_row` distinct columns per row, one of them from a planted perfect matching, values uniform
[0, 100) doubles.  Each path is timed with the cardinality check on and off: the median wall time of the whole call
with a device synchronise, and for `dense` / `sparse` the median kernel time from HIP events.  The per-problem paths run
on at most --loop-max problems and are scaled per problem.  Before anything is timed, the sparse path is compared
problem by problem with the loop and with the dense batch.  One JSON line per (shape, check, path).  Needs the GPU.

  python tools/sparse_batch.py [--reps 5] [--out profiles/sparse_batch.jsonl] [--shapes 1x10x3,1024x64x8]

--status times the status mode (auction_solve_sparse_batch(errors="status", dims=(N, N))) against the default mode
instead, on device tensors with the cardinality check on, legs interleaved within every repetition:
  a  default mode, wall time of the call (it synchronises itself)
  b  status mode, host time of the call (it returns once its launches are enqueued)
  c  status mode, the call plus torch.cuda.synchronize(); stream_ms is the time of its kernels from events around it
  d  as c, on a copy of the batch in which every fourth problem holds a +inf (status 3: its workgroup leaves at once)
With --parent-tree DIR (a built checkout of the commit to compare with) leg a is also run there, as `a_parent`, by a
child process of this script per round, the rounds alternating between the two trees.

  python tools/sparse_batch.py --status [--reps 30] [--rounds 3] [--parent-tree DIR] [--out profiles/sparse_batch_status.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (--tree: the package of another checkout, for the child process of --status --parent-tree)
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else ROOT
sys.path.insert(0, TREE)

SHAPES = ((1, 10, 3), (1024, 64, 8), (1024, 256, 8), (256, 1024, 16), (64, 2048, 16))  # (B, N, entries per row)


def batch(B, N, k, seed):
    rng = np.random.default_rng(seed)
    locs, vals = [], []
    for _ in range(B):
        cols = np.argpartition(rng.random((N, N)), k - 1, axis=1)[:, :k]  # k distinct columns per row
        perm = rng.permutation(N)
        has = (cols == perm[:, None]).any(axis=1)
        cols[~has, 0] = perm[~has]
        cols.sort(axis=1)  # stored in column order, the order the dense batch scans a row
        locs.append(np.stack([np.repeat(np.arange(N), k), cols.ravel()], axis=1).astype(np.int32))
        vals.append(rng.uniform(0.0, 100.0, N * k))
    offsets = np.concatenate([[0], np.cumsum([x.shape[0] for x in locs])]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(locs)), np.ascontiguousarray(np.concatenate(vals)), offsets


def densify(loc, val, offsets, N):
    B = offsets.shape[0] - 1
    mats = np.full((B, N, N), -1.0)
    b = np.repeat(np.arange(B), np.diff(offsets))
    mats[b, loc[:, 0], loc[:, 1]] = val
    return mats


def status_times(shapes, reps, legs):
    """{(B, N, leg): [ms per repetition]} (and "stream_ms" lists for c and d), the legs interleaved within a repetition."""
    import torch
    from sslap_amd import auction_solve_sparse_batch
    sync = torch.cuda.synchronize
    out = {}
    for B, N, k in shapes:
        loc, val, off = batch(B, N, k, seed=B * 7919 + N)
        dl, dv = torch.from_numpy(loc).cuda(), torch.from_numpy(val).cuda()
        val[off[:-1][::4]] = np.inf
        quarter = torch.from_numpy(val).cuda()
        st = dict(errors="status", dims=(N, N))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        if "c" in legs:  # the two modes give the same results at the sizes that are timed
            want, got, part = (auction_solve_sparse_batch(dl, dv, off), auction_solve_sparse_batch(dl, dv, off, **st),
                               auction_solve_sparse_batch(dl, quarter, off, **st))
            assert torch.equal(want["sol"], got["sol"]) and not got["status"].any()
            assert torch.equal(want["prices"].view(torch.int64), got["prices"].view(torch.int64))
            keep = part["status"] == 0
            assert int(keep.sum()) == B - len(range(0, B, 4)) and torch.equal(part["sol"][keep], want["sol"][keep])
            assert bool((part["status"][~keep] == 3).all()) and bool((part["sol"][~keep] == -1).all())

        def run(leg):
            sync()
            t0 = time.perf_counter()
            if leg in ("a", "a_parent"):
                auction_solve_sparse_batch(dl, dv, off)
            elif leg == "b":
                auction_solve_sparse_batch(dl, dv, off, **st)
            else:
                ev[0].record()
                auction_solve_sparse_batch(dl, dv if leg == "c" else quarter, off, **st)
                ev[1].record()
                sync()
            t = (time.perf_counter() - t0) * 1e3
            sync()
            return t, ev[0].elapsed_time(ev[1]) if leg in ("c", "d") else None

        for leg in legs:  # warm-up
            run(leg)
        for r in range(reps):
            for leg in legs[r % len(legs):] + legs[:r % len(legs)]:  # (no leg always runs behind the same other)
                t, g = run(leg)
                out.setdefault((B, N, leg), []).append(t)
                if g is not None:
                    out.setdefault((B, N, leg + ":stream_ms"), []).append(g)
    return out


def status_main(args, shapes):
    """The --status legs; as a child (--legs a_parent) the times go to stdout as one JSON line."""
    if args.legs:
        t = status_times(shapes, args.reps, args.legs.split(","))
        print("TIMES " + json.dumps({f"{B}x{N}/{leg}": v for (B, N, leg), v in t.items()}), flush=True)
        return
    import torch
    torch.zeros(1).cuda()
    times = {}
    per_round = -(-args.reps // args.rounds)
    for _ in range(args.rounds):
        if args.parent_tree:
            cmd = [sys.executable, os.path.abspath(__file__), "--status", "--tree", args.parent_tree, "--legs", "a_parent",
                   "--reps", str(per_round), "--shapes", ",".join(f"{B}x{N}x{k}" for B, N, k in shapes)]
            txt = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
            line = [x for x in txt.splitlines() if x.startswith("TIMES ")][-1]
            for key, v in json.loads(line[6:]).items():
                bn, leg = key.split("/")
                B, N = (int(x) for x in bn.split("x"))
                times.setdefault((B, N, leg), []).extend(v)
        for key, v in status_times(shapes, per_round, ["a", "b", "c", "d"]).items():
            times.setdefault(key, []).extend(v)
    per_row = {(B, N): k for B, N, k in shapes}
    rows = []
    for (B, N, leg), v in times.items():
        if ":" in leg:
            continue
        row = dict(B=B, N=N, per_row=per_row[(B, N)], leg=leg, reps=len(v), median_ms=round(float(np.median(v)), 4),
                   p10_ms=round(float(np.percentile(v, 10)), 4), p90_ms=round(float(np.percentile(v, 90)), 4))
        g = times.get((B, N, leg + ":stream_ms"))
        if g:
            row["stream_ms"] = round(float(np.median(g)), 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="BxNxK,... (K = entries per row)")
    ap.add_argument("--loop-max", type=int, default=256, help="time the per-problem paths on at most so many problems")
    ap.add_argument("--status", action="store_true", help="time the status mode against the default mode")
    ap.add_argument("--rounds", type=int, default=3, help="--status: the repetitions are split over so many rounds")
    ap.add_argument("--parent-tree", default=None, help="--status: a built checkout whose default mode is leg a_parent")
    ap.add_argument("--tree", default=None, help="(child of --parent-tree) import sslap_amd from this checkout")
    ap.add_argument("--legs", default=None, help="(child of --parent-tree) time these legs only, print the raw times")
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 30 if args.status else 5
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "sparse_batch_status.jsonl" if args.status else "sparse_batch.jsonl")
    if args.status:
        return status_main(args, SHAPES if not args.shapes else
                           [tuple(int(x) for x in p.split("x")) for p in args.shapes.split(",")])
    import torch
    from sslap_amd import AuctionSolver, auction_solve, auction_solve_batch, auction_solve_sparse_batch, from_sparse
    shapes = SHAPES if not args.shapes else [tuple(int(x) for x in p.split("x")) for p in args.shapes.split(",")]
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    rows = []
    for B, N, k in shapes:
        loc, val, off = batch(B, N, k, seed=B * 7919 + N)
        mats = densify(loc, val, off, N) if N <= 1024 else None
        Bl = min(B, args.loop_max)  # the per-problem paths: on the first Bl problems, scaled per problem
        part = [(loc[off[b]:off[b + 1]], val[off[b]:off[b + 1]]) for b in range(Bl)]
        for check in (True, False):
            kw = dict(problem="min", cardinality_check=check)
            res = auction_solve_sparse_batch(loc, val, off, **kw)  # warm-up + parity
            for b in range(min(Bl, 32)):
                ref = auction_solve(loc=part[b][0], val=part[b][1].copy(), **kw)
                assert np.array_equal(ref["sol"], res["sol"][b]) and ref["meta"]["its"] == res["meta"]["its"][b]
            if mats is not None:
                rd = auction_solve_batch(mats, **kw)
                assert np.array_equal(rd["sol"], res["sol"]) and np.array_equal(rd["meta"]["its"], res["meta"]["its"])
            timings = {}
            for path in ("loop", "batch", "dense", "sparse"):
                if path == "dense" and mats is None:
                    continue
                ts, ks = [], []
                for _ in range(args.reps):
                    sync()
                    t0 = time.perf_counter()
                    if path == "loop":
                        for lb, vb in part:
                            auction_solve(loc=lb, val=vb.copy(), **kw)
                    elif path == "batch":
                        AuctionSolver.solve_batch([from_sparse(lb, vb.copy(), **kw) for lb, vb in part])
                    elif path == "dense":
                        r = auction_solve_batch(mats, **kw)
                        ks.append(r["meta"]["gpu"]["kernel_ms"])
                    else:
                        r = auction_solve_sparse_batch(loc, val, off, **kw)
                        ks.append(r["meta"]["gpu"]["kernel_ms"])
                    sync()
                    ts.append((time.perf_counter() - t0) * 1e3)
                nprob = B if path in ("dense", "sparse") else Bl
                wall = float(np.median(ts))
                row = dict(B=B, N=N, per_row=k, cardinality_check=check, path=path, problems_timed=nprob,
                           wall_ms=round(wall, 4), wall_ms_per_problem=round(wall / nprob, 5),
                           problems_per_s=round(nprob / (wall * 1e-3), 1), reps=args.reps,
                           its_mean=round(float(np.mean(res["meta"]["its"])), 1))
                if ks:
                    row["kernel_ms"] = round(float(np.median(ks)), 4)
                    row["threads"] = r["meta"]["gpu"]["threads"]
                    row["lds_bytes"] = r["meta"]["gpu"]["lds_bytes"]
                    row["check_ms"] = round(r["meta"]["gpu"]["check_ms"], 4)
                    row["matching_ms"] = round(r["meta"]["gpu"]["matching_ms"], 4)
                    row["lib_wall_ms"] = round(r["meta"]["gpu"]["wall_ms"], 4)  # the C call alone (last rep)
                timings[path] = row["problems_per_s"]
                rows.append(row)
                print(json.dumps(row), flush=True)
            summary = dict(B=B, N=N, per_row=k, cardinality_check=check,
                           sparse_vs_batch=round(timings["sparse"] / timings["batch"], 2),
                           sparse_vs_loop=round(timings["sparse"] / timings["loop"], 2))
            if "dense" in timings:
                summary["sparse_vs_dense"] = round(timings["sparse"] / timings["dense"], 2)
            print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
