"""Strided device stacks: auction_solve_batch on a view, read where it lies, against what a caller had to do before it,
view.contiguous() followed by the call.  On one GPU, in one process, at the B x N sizes of the README's dense table.
The stacks: uniform [0, 100) values (the recipe of tools/dense_batch.py) as float64 and float32 device tensors, seen
through two views:
  transposed   storage (B, N, N), the view is storage.transpose(1, 2): persons run along the unit stride
  cols         storage (B, N, 2 N), the view is storage[:, :, N // 2 : N // 2 + N]: a column slice of a buffer twice as wide
Legs, interleaved within every repetition, every call with errors="status":
  s    auction_solve_batch(view)                            the strided call
  c    auction_solve_batch(view.contiguous())               the copy, then today's call (the yardstick)
  p    auction_solve_batch(copy) on a copy made beforehand  today's call alone
  w    (transposed only) leg s with the lane-per-person bid switched off: every round on the wavefront scan
  kT   (transposed only, --thresholds T,...) leg s with the lane-per-person bid in rounds of at least T bidders
       (MISSLAP_STRIDED_LANE_MIN_K, read by the library at every call): where the library's threshold came from
Per leg: host_ms, the time until the call returns; total_ms, the call plus torch.cuda.synchronize(); stream_ms, the time
of everything the leg put on the stream, from events around it.  Median and p10 - p90 of --reps repetitions; one JSON line
per (shape, dtype, view, leg).  Before anything is timed the legs are compared: the same sol and the same prices, bit for
bit.  Needs the GPU.

  python tools/dense_strided.py [--reps 30] [--out profiles/dense_strided.jsonl] [--shapes 1024x64,...] [--thresholds 16,64]
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
ENV = "MISSLAP_STRIDED_LANE_MIN_K"
OFF = 1 << 20  # above every row count: no round bids one lane per person


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_strided.jsonl"))
    ap.add_argument("--shapes", default=None, help="BxN,...")
    ap.add_argument("--thresholds", default="", help="T,...: extra legs kT on the transposed view")
    args = ap.parse_args()
    import torch
    from sslap_amd import auction_solve_batch
    shapes = SHAPES if not args.shapes else [tuple(int(x) for x in p.split("x")) for p in args.shapes.split(",")]
    thresholds = [int(t) for t in args.thresholds.split(",") if t]
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    os.environ.pop(ENV, None)
    rows = []
    for B, N in shapes:
        host = np.random.default_rng(B * 7919 + N).uniform(0.0, 100.0, (B, N, N))
        for dtype in ("float64", "float32"):
            vals = torch.from_numpy(host).to(getattr(torch, dtype)).cuda()
            for layout in ("transposed", "cols"):
                if layout == "transposed":
                    view = vals.transpose(1, 2).contiguous().transpose(1, 2)
                else:
                    wide = torch.zeros((B, N, 2 * N), dtype=vals.dtype, device="cuda")
                    view = wide[:, :, N // 2:N // 2 + N]
                    view.copy_(vals)
                copy = view.contiguous()
                assert torch.equal(copy, vals) and (N == 1 or not view.is_contiguous())
                kw = dict(errors="status", mat_dtype=dtype)

                def leg(name):
                    if name == "c":
                        return auction_solve_batch(view.contiguous(), **kw)
                    if name == "p":
                        return auction_solve_batch(copy, **kw)
                    if name == "s":
                        return auction_solve_batch(view, **kw)
                    os.environ[ENV] = str(OFF if name == "w" else int(name[1:]))
                    try:
                        return auction_solve_batch(view, **kw)
                    finally:
                        del os.environ[ENV]

                legs = ["s", "c", "p"] + (["w"] + [f"k{t}" for t in thresholds] if layout == "transposed" else [])
                ref = leg("p")
                assert not ref["status"].any()
                for name in legs:  # the legs solve the same problems to the same bits
                    got = leg(name)
                    assert torch.equal(got["status"], ref["status"]) and torch.equal(got["sol"], ref["sol"]), name
                    assert torch.equal(got["prices"].view(torch.int64), ref["prices"].view(torch.int64)), name
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
                    row = dict(B=B, N=N, dtype=dtype, view=layout, leg=name, reps=len(t))
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
