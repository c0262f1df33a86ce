"""Warm-started tracker frames from two point sets on the device: auction_solve_points_batch(prices=, outside=,
finish="reverse") against the cold solve it replaces, and against the dense route at the same commit.  On one GPU, in
one process.
A sequence of frames: frame 0 is float32 coordinates, uniform in [-1, 1)^D with D = 3, N points on either side; every
later frame adds N(0, 0.02) to every coordinate of the frame before.  Every row has an outside value (the squared-distance
gate), uniform in [0.5, 1.5) x 4 N^(-2/3), about the squared distance to a nearest neighbour.  Frame f is solved
  c  cold: fast=True from zero prices (optimal within n * eps on its own: what the README advises for a cold solve)
  w  warm: fast=True from prices= of the finished solve of frame f - 1, no finish
  f  warm with finish="reverse": the same call and one more launch
  d  (N <= 1024) the yardstick: the float64 stack of the frame built on the device by the definition's chain, then
     auction_solve_batch(stack, prices=, outside=, finish="reverse"); the stack's bytes are peak_stack_bytes
interleaved within every repetition, the frame changing from repetition to repetition.  Per leg: host_ms, the time until
the call returns; total_ms, the call plus torch.cuda.synchronize(); stream_ms, the time of everything the leg put on the
stream, from events around it; rounds, the forward rounds; gap, the mean distance per problem of the leg's objective from
the cold leg's.  Median and p10 - p90 of --reps repetitions; one JSON line per (shape, leg).
Leg r is the finish launch alone, on copies of leg w's outputs (misslap_points_batch_reverse_finish through the front
end's own launch helper), with its iteration count (mean and largest over the batch) and the microseconds per iteration of
the problem with the most.  Needs the GPU.

  python tools/points_finish.py [--reps 30] [--frames 6] [--coords 3] [--out profiles/points_finish.jsonl] [--shapes 1024x64,...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1024, 64), (256, 256), (64, 1000), (64, 2048)]  # (B, N): N points on either side
DENSE_MAX = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--coords", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_finish.jsonl"))
    ap.add_argument("--shapes", default=None, help="BxN,...")
    args = ap.parse_args()
    import torch
    from sslap_amd import auction_solve_batch, auction_solve_points_batch
    from sslap_amd.points_batch import _reverse_finish_launch
    shapes = SHAPES if not args.shapes else [tuple(int(v) for v in p.split("x")) for p in args.shapes.split(",")]
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
        hx = rng.uniform(-1, 1, (B, N, args.coords))
        hy = rng.uniform(-1, 1, (B, N, args.coords))
        frames = []
        for f in range(args.frames):
            if f:
                hx, hy = hx + rng.normal(0.0, 0.02, hx.shape), hy + rng.normal(0.0, 0.02, hy.shape)
            frames.append((torch.from_numpy(hx.astype(np.float32)).cuda(), torch.from_numpy(hy.astype(np.float32)).cuda()))
        kw = dict(fast=True, errors="status", outside=torch.from_numpy(rng.uniform(0.5, 1.5, (B, N)) * 4.0 * N ** (-2.0 / 3.0)).cuda())
        # the chain: frame f starts from the finished prices of frame f - 1
        warm = [None]
        for f in range(args.frames - 1):
            r = auction_solve_points_batch(*frames[f], prices=warm[f], finish="reverse", **kw)
            assert not r["status"].any() and not r["reverse"]["left"].any()
            warm.append(r["prices"].clone())
        dense = N <= DENSE_MAX

        def leg(name, f):
            if name == "c":
                return auction_solve_points_batch(*frames[f], **kw)
            if name == "d":
                return auction_solve_batch(stack_of(*frames[f]), prices=warm[f], finish="reverse", **kw)
            return auction_solve_points_batch(*frames[f], prices=warm[f], **(dict(kw, finish="reverse") if name == "f" else kw))

        legs = ["c", "w", "f"] + (["d"] if dense else [])
        times, rounds, gaps, its_all, agree = {}, {}, {}, [], []
        for r in range(-1, args.reps):  # (r = -1: the warm-up)
            f = 1 + r % (args.frames - 1)
            k = r % len(legs)
            done = {}
            for name in legs[k:] + legs[:k]:  # (no leg always runs behind the same other)
                sync()
                t0 = time.perf_counter()
                ev[0].record()
                res = leg(name, f)
                ev[1].record()
                t1 = time.perf_counter()
                sync()
                t2 = time.perf_counter()
                done[name] = res
                if r >= 0:
                    times.setdefault(name, []).append(((t1 - t0) * 1e3, (t2 - t0) * 1e3, ev[0].elapsed_time(ev[1])))
                    rounds.setdefault(name, []).append(float(res["meta"]["its"].double().mean()))
            cold_obj = done["c"]["meta"]["obj_f64"]
            for name in legs:
                assert not done[name]["status"].any(), name
                if r >= 0:
                    gaps.setdefault(name, []).append(float((done[name]["meta"]["obj_f64"] - cold_obj).abs().mean()))
            if dense and r >= 0:  # whether the two routes gave one result, bit for bit
                agree.append(bool(torch.equal(done["d"]["sol"], done["f"]["sol"]) and torch.equal(done["d"]["prices"], done["f"]["prices"])))
            # the finish launch alone, on copies of the warm leg's outputs
            w = done["w"]
            copy = dict(w, sol=w["sol"].clone(), prices=w["prices"].clone(), records=w["records"].clone(),
                        outside_prices=w["outside_prices"].clone())
            sync()
            ev[0].record()
            its, left = _reverse_finish_launch(*frames[f], copy, "min", 1000000)
            ev[1].record()
            sync()
            assert not left.any()
            if r >= 0:
                its_all.append((ev[0].elapsed_time(ev[1]), float(its.double().mean()), int(its.max())))
        for name in legs:
            t = np.array(times[name])
            row = dict(B=B, N=N, D=args.coords, leg=name, reps=len(t), rounds=round(float(np.median(rounds[name])), 1),
                       gap=round(float(np.median(gaps[name])), 6))
            if name == "d":
                row["peak_stack_bytes"] = B * N * N * 8
                row["same_as_f"] = all(agree)
            for k, what in enumerate(("host_ms", "total_ms", "stream_ms")):
                row[what] = round(float(np.median(t[:, k])), 4)
                row[what + "_p10"] = round(float(np.percentile(t[:, k], 10)), 4)
                row[what + "_p90"] = round(float(np.percentile(t[:, k], 90)), 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
        a = np.array(its_all)
        row = dict(B=B, N=N, D=args.coords, leg="r", reps=len(a), stream_ms=round(float(np.median(a[:, 0])), 4),
                   stream_ms_p10=round(float(np.percentile(a[:, 0], 10)), 4),
                   stream_ms_p90=round(float(np.percentile(a[:, 0], 90)), 4), its_mean=round(float(np.median(a[:, 1])), 1),
                   its_max=int(np.median(a[:, 2])), us_per_it=round(float(np.median(a[:, 0] * 1e3 / np.maximum(a[:, 2], 1))), 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
