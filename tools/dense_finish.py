"""Warm-started rectangular frames on the device: auction_solve_batch(prices=, finish="reverse") against the cold solve
it replaces.  On one GPU, in one process.
A sequence of frames: frame 0 is uniform [0, 100) doubles with half the entries gated to -1; every later frame adds
N(0, 1) to the entries of the frame before (clipped at 0, the gates stay).  Frame f is solved
  c  cold: fast=True from zero prices (optimal within n * eps on its own: what the README advises for a cold solve)
  w  warm: fast=True from prices= of the finished solve of frame f - 1, no finish
  f  warm with finish="reverse": the same call and one more launch
interleaved within every repetition, the frame changing from repetition to repetition.  Per leg: host_ms, the time until
the call returns; total_ms, the call plus torch.cuda.synchronize(); stream_ms, the time of everything the leg put on the
stream, from events around it; rounds, the forward rounds; gap, the mean distance per problem of the leg's objective from
the cold leg's.  Median and p10 - p90 of --reps repetitions; one JSON line per (shape, leg).
Leg r is the finish launch alone, on copies of leg w's outputs (misslap_dense_batch_reverse_finish through the front
end's own launch helper), with its iteration count (mean and largest over the batch) and the microseconds per iteration of
the problem with the most.  Needs the GPU.

  python tools/dense_finish.py [--reps 30] [--frames 6] [--out profiles/dense_finish.jsonl] [--shapes 1024x64x96,256x256o,...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (B, N, M, outside): the plain rectangular sizes, and the README's outside sizes
SHAPES = [(1024, 64, 96, False), (256, 256, 320, False), (64, 1000, 1024, False), (1024, 64, 64, True), (256, 256, 256, True)]


def parse(text):
    out = []
    for p in text.split(","):
        o = p.endswith("o")
        d = [int(x) for x in p.rstrip("o").split("x")]
        out.append((d[0], d[1], d[2] if len(d) > 2 else d[1], o))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_finish.jsonl"))
    ap.add_argument("--shapes", default=None, help="BxNxM or BxNo (with an outside value per row),...")
    args = ap.parse_args()
    import torch
    from sslap_amd import _lib, auction_solve_batch
    from sslap_amd.dense_batch import _reverse_finish_launch
    shapes = SHAPES if not args.shapes else parse(args.shapes)
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    for B, N, M, out in shapes:
        rng = np.random.default_rng(B * 7919 + N * 31 + M)
        host = rng.uniform(0.0, 100.0, (B, N, M))
        gate = rng.random((B, N, M)) < 0.5
        frames = []
        for f in range(args.frames):
            if f:
                host = np.maximum(host + rng.normal(0.0, 1.0, host.shape), 0.0)
            frames.append(torch.from_numpy(np.where(gate, -1.0, host)).cuda())
        kw = dict(fast=True, errors="status")
        if out:
            kw["outside"] = torch.from_numpy(rng.uniform(0.0, 100.0, (B, N))).cuda()
        # the chain: frame f starts from the finished prices of frame f - 1
        warm = [None]
        for f in range(args.frames - 1):
            r = auction_solve_batch(frames[f], prices=warm[f], finish="reverse", **kw)
            assert not r["status"].any() and not r["reverse"]["left"].any()
            warm.append(r["prices"].clone())

        def leg(name, f):
            if name == "c":
                return auction_solve_batch(frames[f], **kw)
            return auction_solve_batch(frames[f], prices=warm[f], finish="reverse" if name == "f" else None, **kw)

        legs = ["c", "w", "f"]
        times, rounds, gaps, its_all = {}, {}, {}, []
        for r in range(-1, args.reps):  # (r = -1: the warm-up)
            f = 1 + r % (args.frames - 1)
            k = r % len(legs)
            cold_obj = None
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
            # the finish launch alone, on copies of the warm leg's outputs
            w = done["w"]
            copy = dict(w, sol=w["sol"].clone(), prices=w["prices"].clone(), records=w["records"].clone())
            if out:
                copy["outside_prices"] = w["outside_prices"].clone()
            sync()
            ev[0].record()
            its, left = _reverse_finish_launch(frames[f], copy, "min", 1000000, _lib.DTYPE_F64)
            ev[1].record()
            sync()
            assert not left.any()
            if r >= 0:
                its_all.append((ev[0].elapsed_time(ev[1]), float(its.double().mean()), int(its.max())))
        for name in legs:
            t = np.array(times[name])
            row = dict(B=B, N=N, M=M, outside=out, leg=name, reps=len(t), rounds=round(float(np.median(rounds[name])), 1),
                       gap=round(float(np.median(gaps[name])), 4))
            for k, what in enumerate(("host_ms", "total_ms", "stream_ms")):
                row[what] = round(float(np.median(t[:, k])), 4)
                row[what + "_p10"] = round(float(np.percentile(t[:, k], 10)), 4)
                row[what + "_p90"] = round(float(np.percentile(t[:, k], 90)), 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
        a = np.array(its_all)
        row = dict(B=B, N=N, M=M, outside=out, leg="r", reps=len(a), stream_ms=round(float(np.median(a[:, 0])), 4),
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
