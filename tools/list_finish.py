"""Warm-started gated frames on the device through the list front ends: auction_solve_ell_batch /
auction_solve_sparse_batch(prices=, outside=, finish="reverse") against the cold solve they replace.  On one GPU, in one
process; it follows tools/dense_finish.py.
A sequence of frames: K distinct candidates per row among M = N columns, values uniform [0, 100); every later frame adds
N(0, 1) to the values of the frame before (clipped at 0, the candidates stay).  Every row has an outside value.  Frame f
is solved, through each front end,
  c  cold: fast=True from zero prices (optimal within n * eps on its own: what the README advises for a cold solve)
  w  warm: fast=True from prices= of the finished solve of frame f - 1, no finish
  f  warm with finish="reverse": the same call and one more launch
interleaved within every repetition, the frame changing from repetition to repetition.  Per leg: host_ms, total_ms and
stream_ms as in tools/dense_finish.py, the forward rounds, and gap, the mean distance per problem of the leg's objective
from the cold leg's.  Leg r is the finish launch alone on copies of leg w's outputs, with its iteration count (mean and
largest over the batch) and the microseconds per iteration of the problem with the most.  Where the densified stack fits
the dense batch (N, M <= 1024) leg rd is the dense finish alone on the outputs of the dense warm call on it
(entries="finite"), in the same repetitions.  Median and p10 - p90 of --reps repetitions; one JSON line per
(shape, front, leg).  Needs the GPU.

  python tools/list_finish.py [--reps 30] [--frames 6] [--out profiles/list_finish.jsonl] [--shapes 1024x64x8,...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1024, 64, 8), (1024, 256, 8), (256, 1024, 16), (64, 2048, 16)]  # (B, N, K), M = N, outside on


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_finish.jsonl"))
    ap.add_argument("--shapes", default=None, help="BxNxK,...")
    args = ap.parse_args()
    import torch
    from sslap_amd import _lib, auction_solve_batch, auction_solve_ell_batch, auction_solve_sparse_batch
    from sslap_amd import dense_batch, ell_batch, sparse_batch
    shapes = SHAPES if not args.shapes else [tuple(int(x) for x in p.split("x")) for p in args.shapes.split(",")]
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []

    def summary(t, names):
        out = {}
        for k, what in enumerate(names):
            out[what] = round(float(np.median(t[:, k])), 4)
            out[what + "_p10"] = round(float(np.percentile(t[:, k], 10)), 4)
            out[what + "_p90"] = round(float(np.percentile(t[:, k], 90)), 4)
        return out

    for B, N, K in shapes:
        M = N
        rng = np.random.default_rng(B * 7919 + N * 31 + K)
        start, step = rng.integers(0, M, (B, N, 1)), 2 * rng.integers(0, M // 2, (B, N, 1)) + 1
        cols = np.sort((start + step * np.arange(K)) % M, axis=2).astype(np.int32)  # (M a power of two: K distinct columns)
        host = rng.uniform(0.0, 100.0, (B, N, K))
        d_cols = torch.from_numpy(cols).cuda()
        loc = np.stack([np.tile(np.repeat(np.arange(N), K), B), cols.reshape(-1)], axis=1).astype(np.int32)
        d_loc, off = torch.from_numpy(loc).cuda(), np.arange(B + 1, dtype=np.int64) * (N * K)
        dense_fits = N <= dense_batch.MAX_DIM and M <= dense_batch.MAX_DIM
        frames, stacks = [], []
        bi, ri = np.arange(B)[:, None, None], np.arange(N)[None, :, None]
        for f in range(args.frames):
            if f:
                host = np.maximum(host + rng.normal(0.0, 1.0, host.shape), 0.0)
            frames.append(torch.from_numpy(host.copy()).cuda())
            if dense_fits:
                mat = np.full((B, N, M), np.nan)
                mat[bi, ri, cols] = host
                stacks.append(torch.from_numpy(mat).cuda())
        outside = torch.from_numpy(rng.uniform(0.0, 100.0, (B, N))).cuda()
        kw = dict(fast=True, errors="status", outside=outside)

        def call(front, f, **more):
            if front == "ell":
                return auction_solve_ell_batch(d_cols, frames[f], n_cols=M, **kw, **more)
            return auction_solve_sparse_batch(d_loc, frames[f].reshape(-1), off, dims=(N, M), **kw, **more)

        warm = [None]  # the chain: frame f starts from the finished prices of frame f - 1
        for f in range(args.frames - 1):
            r = call("ell", f, prices=warm[f], finish="reverse")
            assert not r["status"].any() and not r["reverse"]["left"].any()
            warm.append(r["prices"].clone())

        def leg(front, name, f):
            if name == "c":
                return call(front, f)
            return call(front, f, prices=warm[f], finish="reverse" if name == "f" else None)

        legs = [(front, name) for front in ("ell", "sparse") for name in ("c", "w", "f")]
        times, rounds, gaps, alone = {}, {}, {}, {}
        for r in range(-1, args.reps):  # (r = -1: the warm-up)
            f = 1 + r % (args.frames - 1)
            k = r % len(legs)
            done = {}
            for key in legs[k:] + legs[:k]:  # (no leg always runs behind the same other)
                sync()
                t0 = time.perf_counter()
                ev[0].record()
                res = leg(*key, f)
                ev[1].record()
                t1 = time.perf_counter()
                sync()
                t2 = time.perf_counter()
                done[key] = res
                if r >= 0:
                    times.setdefault(key, []).append(((t1 - t0) * 1e3, (t2 - t0) * 1e3, ev[0].elapsed_time(ev[1])))
                    rounds.setdefault(key, []).append(float(res["meta"]["its"].double().mean()))
            for key in legs:
                assert not done[key]["status"].any(), key
                if r >= 0:
                    cold = done[(key[0], "c")]["meta"]["obj_f64"]
                    gaps.setdefault(key, []).append(float((done[key]["meta"]["obj_f64"] - cold).abs().mean()))
            # the finish launches alone, on copies of the warm legs' outputs
            todo = [("ell", ell_batch._reverse_finish_launch, done[("ell", "w")]),
                    ("sparse", sparse_batch._reverse_finish_launch, done[("sparse", "w")])]
            if dense_fits:
                w = auction_solve_batch(stacks[f], entries="finite", prices=warm[f], **kw)
                todo.append(("dense", lambda c, p, n, s=stacks[f]: dense_batch._reverse_finish_launch(
                    s, c, p, n, _lib.DTYPE_F64 | _lib.DENSE_ENTRIES_FINITE), w))
            for front, launch, w in todo:
                copy = dict(w, sol=w["sol"].clone(), prices=w["prices"].clone(), records=w["records"].clone(),
                            outside_prices=w["outside_prices"].clone())
                sync()
                ev[0].record()
                its, left = launch(copy, "min", 1000000)
                ev[1].record()
                sync()
                assert not left.any()
                if r >= 0:
                    alone.setdefault(front, []).append((ev[0].elapsed_time(ev[1]), float(its.double().mean()), int(its.max())))
        for key in legs:
            row = dict(B=B, N=N, K=K, M=M, outside=True, front=key[0], leg=key[1], reps=len(times[key]),
                       rounds=round(float(np.median(rounds[key])), 1), gap=round(float(np.median(gaps[key])), 4),
                       **summary(np.array(times[key]), ("host_ms", "total_ms", "stream_ms")))
            rows.append(row)
            print(json.dumps(row), flush=True)
        for front, a in alone.items():
            a = np.array(a)
            row = dict(B=B, N=N, K=K, M=M, outside=True, front=front, leg="rd" if front == "dense" else "r", reps=len(a),
                       **summary(a, ("stream_ms",)), its_mean=round(float(np.median(a[:, 1])), 1), its_max=int(np.median(a[:, 2])),
                       us_per_it=round(float(np.median(a[:, 0] * 1e3 / np.maximum(a[:, 2], 1))), 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
