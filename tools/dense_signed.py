"""Signed dense stacks: auction_solve_batch(entries="finite") on a contiguous device stack of signed costs, against what
a caller had to do before it (subtract every problem's minimum, then today's call), and the price of routing a
contiguous stack through the strided kernel family.  On one GPU, in one process, at the B x N sizes of the README's
dense table; float64 and float32 device stacks.
Legs, interleaved within every repetition, every call with errors="status":
  f    auction_solve_batch(signed, entries="finite")            the finite-mode call, uniform values in [-50, 50)
  m    auction_solve_batch(signed - signed.amin((1, 2), True))  the shift, then today's call (the yardstick)
  n    auction_solve_batch(shifted)                             today's call alone, on a stack shifted beforehand
  g    auction_solve_batch(shifted, entries="finite")           the finite-mode call on that same non-negative stack:
                                                                g against n is the price of the strided family
Per leg: host_ms, the time until the call returns; total_ms, the call plus torch.cuda.synchronize(); stream_ms, the time
of everything the leg put on the stream, from events around it.  Median and p10 - p90 of --reps repetitions; one JSON line
per (shape, dtype, leg).  Before anything is timed legs n and g are compared: the same sol and the same prices, bit for
bit (legs f and m solve differently rounded values and need not tie-break alike: only their statuses are compared).
Needs the GPU.

  python tools/dense_signed.py [--reps 30] [--out profiles/dense_signed.jsonl] [--shapes 1024x64,...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 10), (1, 100), (1, 300), (1024, 64), (1024, 100), (256, 256), (64, 1000)]  # (B, N): the README's dense table
LEGS = ["f", "m", "n", "g"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_signed.jsonl"))
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
        host = np.random.default_rng(B * 7919 + N).uniform(-50.0, 50.0, (B, N, N))
        for dtype in ("float64", "float32"):
            signed = torch.from_numpy(host).to(getattr(torch, dtype)).cuda()
            shifted = signed - signed.amin(dim=(1, 2), keepdim=True)
            kw = dict(errors="status", mat_dtype=dtype)

            def leg(name):
                if name == "f":
                    return auction_solve_batch(signed, entries="finite", **kw)
                if name == "m":
                    return auction_solve_batch(signed - signed.amin(dim=(1, 2), keepdim=True), **kw)
                if name == "n":
                    return auction_solve_batch(shifted, **kw)
                return auction_solve_batch(shifted, entries="finite", **kw)

            ref = leg("n")
            assert not ref["status"].any()
            for name in LEGS:
                got = leg(name)
                assert torch.equal(got["status"], ref["status"]), name
                if name == "g":  # the same entries under either rule: the same bits
                    assert torch.equal(got["sol"], ref["sol"]), name
                    assert torch.equal(got["prices"].view(torch.int64), ref["prices"].view(torch.int64)), name
            times = {}
            for r in range(-1, args.reps):  # (r = -1: the warm-up)
                k = r % len(LEGS)
                for name in LEGS[k:] + LEGS[:k]:  # (no leg always runs behind the same other)
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
            for name in LEGS:
                t = np.array(times[name])
                row = dict(B=B, N=N, dtype=dtype, leg=name, reps=len(t))
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
