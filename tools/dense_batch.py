"""Many small dense problems: three ways of solving the same stack, on one GPU, in one process.
  loop   a loop of auction_solve(mat=...)
  batch  solve_batch over from_matrix handles (handle creation and the matching guard included)
  dense  auction_solve_batch (one launch, one workgroup per problem)
Matrices follow the reference's benchmarking.py recipes: uniform [0, 100) doubles ("float") and integers 1..99 ("int"),
fully dense.  Each path is timed with the cardinality check on and off: wall time of the whole call with a device
synchronise, and for `dense` the kernel time from HIP events.  One JSON line per (point, recipe, check, path).  The
results of the three paths are compared problem by problem before anything is timed.  Needs the GPU.

  python tools/dense_batch.py [--reps 5] [--out profiles/dense_batch.jsonl] [--points 1x10,1024x64]

--status times the status mode (auction_solve_batch(errors="status")) against the default mode instead, on a device
stack with the cardinality check on, legs interleaved within every repetition:
  a  default mode, wall time of the call (it synchronises itself)
  b  status mode, host time of the call (it returns once its launches are enqueued)
  c  status mode, the call plus torch.cuda.synchronize(); stream_ms is the time of its kernels from events around it
  d  as c, on a copy of the stack in which every fourth problem holds a +inf (status 3: its workgroup leaves at once)
With --parent-tree DIR (a built checkout of the commit to compare with) leg a is also run there, as `a_parent`, by a
child process of this script per round, the rounds alternating between the two trees.

  python tools/dense_batch.py --status [--reps 30] [--rounds 3] [--parent-tree DIR] [--out profiles/dense_batch_status.jsonl]

--dtype times typed stacks (auction_solve_batch(mat_dtype=)) on a device stack, default mode, the cardinality check on.
Every leg solves the same values: uniform [0, 100) rounded to what float16 and bfloat16 both hold, so the four stacks
are one problem and their results are compared bit for bit before anything is timed.  Legs, interleaved within every
repetition:
  float64                        the float64 stack
  float32, float16, bfloat16     the typed stack, read in place
  float32+widen, ...             what a caller does without the keyword: mats.double(), then the float64 call, together
Per leg: wall time of the call plus torch.cuda.synchronize() (median, p10, p90) and the solve kernel's time from HIP
events (median).  With --parent-lib PATH (libmisslap.so of the commit to compare with) the float64 leg also runs on
that library, as `float64_parent`, in a child process per round, the rounds alternating between the two libraries.

  python tools/dense_batch.py --dtype [--reps 30] [--rounds 3] [--parent-lib PATH] [--out profiles/dense_batch_dtype.jsonl]
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

POINTS = ((1, 10), (1, 100), (1, 300), (1024, 64), (1024, 100), (256, 256), (64, 1000))
STATUS_POINTS = ((1, 10), (1, 100), (1024, 64), (1024, 100), (256, 256), (64, 1000))


def stack(B, N, recipe, seed):
    rng = np.random.default_rng(seed)
    if recipe == "int":
        return rng.integers(1, 100, (B, N, N)).astype(np.float64)
    return rng.uniform(0.0, 100.0, (B, N, N))


def status_times(points, reps, legs):
    """{(B, N, leg): [ms per repetition]} (and "stream_ms" lists for c), the legs interleaved within a repetition."""
    import torch
    from sslap_amd import auction_solve_batch
    sync = torch.cuda.synchronize
    out = {}
    for B, N in points:
        host = stack(B, N, "float", seed=B * 7919 + N)
        mats = torch.from_numpy(host).cuda()
        host[::4, 0, 0] = np.inf
        quarter = torch.from_numpy(host).cuda()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        if "c" in legs:  # the two modes give the same results at the sizes that are timed
            want, got, part = (auction_solve_batch(mats), auction_solve_batch(mats, errors="status"),
                               auction_solve_batch(quarter, errors="status"))
            assert torch.equal(want["sol"], got["sol"]) and not got["status"].any()
            assert torch.equal(want["prices"].view(torch.int64), got["prices"].view(torch.int64))
            keep = part["status"] == 0
            assert int(keep.sum()) == B - len(range(0, B, 4)) and torch.equal(part["sol"][keep], want["sol"][keep])

        def run(leg):
            sync()
            t0 = time.perf_counter()
            if leg in ("a", "a_parent"):
                auction_solve_batch(mats)
            elif leg == "b":
                auction_solve_batch(mats, errors="status")
            else:
                ev[0].record()
                auction_solve_batch(mats if leg == "c" else quarter, errors="status")
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


DTYPES = ("float32", "float16", "bfloat16")


def dtype_times(points, reps, legs):
    """{(B, N, leg): [ms per repetition]} and (B, N, leg + ":kernel_ms") lists, the legs interleaved within a repetition."""
    import torch
    from sslap_amd import auction_solve_batch
    sync = torch.cuda.synchronize
    out = {}
    for B, N in points:
        draw = torch.from_numpy(stack(B, N, "float", seed=B * 7919 + N))
        wide = draw.to(torch.bfloat16).double()
        wide[wide.to(torch.float16).double() != wide] = 1.0  # (below float16's normal range: not the same value there)
        stacks = {"float64": wide.cuda()}
        for name in DTYPES:
            stacks[name] = wide.to(getattr(torch, name)).cuda()
            assert torch.equal(stacks[name].double(), stacks["float64"])
        want = auction_solve_batch(stacks["float64"])
        for name in DTYPES if len(legs) > 1 else ():  # one problem, one result
            got = auction_solve_batch(stacks[name], mat_dtype=name)
            assert torch.equal(want["sol"], got["sol"])
            assert torch.equal(want["prices"].view(torch.int64), got["prices"].view(torch.int64))
            assert np.array_equal(want["meta"]["its"], got["meta"]["its"])

        def run(leg):
            sync()
            t0 = time.perf_counter()
            if leg in ("float64", "float64_parent"):
                r = auction_solve_batch(stacks["float64"])
            elif leg.endswith("+widen"):
                r = auction_solve_batch(stacks[leg[:-6]].double())
            else:
                r = auction_solve_batch(stacks[leg], mat_dtype=leg)
            sync()
            return (time.perf_counter() - t0) * 1e3, r["meta"]["gpu"]

        for leg in legs:  # warm-up
            run(leg)
        for r in range(reps):
            for leg in legs[r % len(legs):] + legs[:r % len(legs)]:
                t, g = run(leg)
                out.setdefault((B, N, leg), []).append(t)
                for k in ("kernel_ms", "check_ms", "matching_ms"):
                    out.setdefault((B, N, leg + ":" + k), []).append(g[k])
    return out


def dtype_main(args, points):
    """The --dtype legs; as a child (--legs float64_parent, MISSLAP_LIB set) the times go to stdout as one JSON line."""
    if args.legs:
        t = dtype_times(points, args.reps, args.legs.split(","))
        print("TIMES " + json.dumps({f"{B}x{N}/{leg}": v for (B, N, leg), v in t.items()}), flush=True)
        return
    import torch
    torch.zeros(1).cuda()
    legs = ["float64"] + [x for name in DTYPES for x in (name, name + "+widen")]
    times = {}
    per_round = -(-args.reps // args.rounds)
    for _ in range(args.rounds):
        if args.parent_lib:
            cmd = [sys.executable, os.path.abspath(__file__), "--dtype", "--legs", "float64_parent", "--reps", str(per_round),
                   "--points", ",".join(f"{B}x{N}" for B, N in points)]
            txt = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900,
                                 env=dict(os.environ, MISSLAP_LIB=os.path.abspath(args.parent_lib))).stdout
            line = [x for x in txt.splitlines() if x.startswith("TIMES ")][-1]
            for k, v in json.loads(line[6:]).items():
                bn, leg = k.split("/")
                B, N = (int(x) for x in bn.split("x"))
                times.setdefault((B, N, leg), []).extend(v)
        for k, v in dtype_times(points, per_round, legs).items():
            times.setdefault(k, []).extend(v)
    rows = []
    for (B, N, leg), v in times.items():
        if ":" in leg:
            continue
        row = dict(B=B, N=N, leg=leg, reps=len(v), median_ms=round(float(np.median(v)), 4),
                   p10_ms=round(float(np.percentile(v, 10)), 4), p90_ms=round(float(np.percentile(v, 90)), 4))
        for k in ("kernel_ms", "check_ms", "matching_ms"):
            row[k] = round(float(np.median(times[(B, N, leg + ":" + k)])), 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


def status_main(args, points):
    """The --status legs; as a child (--legs a_parent) the times go to stdout as one JSON line."""
    if args.legs:
        t = status_times(points, args.reps, args.legs.split(","))
        print("TIMES " + json.dumps({f"{B}x{N}/{leg}": v for (B, N, leg), v in t.items()}), flush=True)
        return
    import torch
    torch.zeros(1).cuda()
    times = {}
    per_round = -(-args.reps // args.rounds)
    for _ in range(args.rounds):
        if args.parent_tree:
            cmd = [sys.executable, os.path.abspath(__file__), "--status", "--tree", args.parent_tree, "--legs", "a_parent",
                   "--reps", str(per_round), "--points", ",".join(f"{B}x{N}" for B, N in points)]
            txt = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
            line = [x for x in txt.splitlines() if x.startswith("TIMES ")][-1]
            for k, v in json.loads(line[6:]).items():
                bn, leg = k.split("/")
                B, N = (int(x) for x in bn.split("x"))
                times.setdefault((B, N, leg), []).extend(v)
        for k, v in status_times(points, per_round, ["a", "b", "c", "d"]).items():
            times.setdefault(k, []).extend(v)
    rows = []
    for (B, N, leg), v in times.items():
        if ":" in leg:
            continue
        row = dict(B=B, N=N, leg=leg, reps=len(v), median_ms=round(float(np.median(v)), 4),
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
    ap.add_argument("--points", default=None, help="BxN,BxN,...")
    ap.add_argument("--loop-max", type=int, default=256, help="time the per-problem paths on at most so many problems")
    ap.add_argument("--status", action="store_true", help="time the status mode against the default mode")
    ap.add_argument("--dtype", action="store_true", help="time float32 / float16 / bfloat16 stacks against float64")
    ap.add_argument("--parent-lib", default=None, help="--dtype: another build's libmisslap.so, leg float64_parent")
    ap.add_argument("--rounds", type=int, default=3, help="--status / --dtype: the repetitions are split over so many rounds")
    ap.add_argument("--parent-tree", default=None, help="--status: a built checkout whose default mode is leg a_parent")
    ap.add_argument("--tree", default=None, help="(child of --parent-tree) import sslap_amd from this checkout")
    ap.add_argument("--legs", default=None, help="(child of --parent-tree) time these legs only, print the raw times")
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 30 if args.status or args.dtype else 5
    if args.out is None:
        name = "dense_batch_status.jsonl" if args.status else "dense_batch_dtype.jsonl" if args.dtype else "dense_batch.jsonl"
        args.out = os.path.join(ROOT, "profiles", name)
    if args.dtype:
        pts = STATUS_POINTS if not args.points else [tuple(int(x) for x in p.split("x")) for p in args.points.split(",")]
        return dtype_main(args, pts)
    if args.status:
        pts = STATUS_POINTS if not args.points else [tuple(int(x) for x in p.split("x")) for p in args.points.split(",")]
        return status_main(args, pts)
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
