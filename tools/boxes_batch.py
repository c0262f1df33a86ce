"""IoU / GIoU costs from two box sets: auction_solve_boxes_batch(a, b, metric, outside=1 - 0.3) against what a tracker
did until now, against the plain points call on the same coordinates, and at two eps.  On one GPU.
The workload: float32 boxes on the device, a tracker-like frame pair -- N tracks with centres uniform over a field in
which a box overlaps a handful of others, sides 0.6 .. 1.4, and the detections are the tracks in another order, each
moved by up to 0.15 and resized by up to 10 %.  outside = 1 - 0.3 (the IoU gate of SORT and its kin), errors="status".
Per shape and metric the legs, interleaved within every repetition:
  n  the new call: auction_solve_boxes_batch(a, b, metric, outside=0.7)                      (fast=True: eps = 1 / N)
  c  the list route: ... candidates=16
  b  the builder alone: boxes_candidates(a, b, 16, limit=0.7, metric=metric)
  t  the yardstick (N <= 1024, the dense batch's cap): the float64 stack built on the device with torch by the
     definition's formula, then auction_solve_batch(stack, outside=0.7).  torch may round differently, so `gap` is the
     mean |objective difference| per problem against leg n, not a comparison of bits.
  p  the plain points call at D = 4 on the same coordinates, its gate at the quantile of ITS costs that lets as many
     columns per row pass: n - p is the price of the divisions and selects
  e  the new call at eps_start = 1e-3 / N (one phase, optimal within 1e-3 in total): `rounds` and `obj_gap`, the mean
     objective of leg n minus this leg's, are the price and the gain of the smaller eps (--eps-reps repetitions)
  q  (--parent-tree DIR, a built checkout of the parent commit; metric "iou" only, the leg does not depend on it) leg p
     run there by a child process per round, the rounds alternating between the two trees: the plain call must not have
     moved.
Per leg: host_ms, the time until the call returns; total_ms, the call plus torch.cuda.synchronize(); peak_bytes,
torch.cuda.max_memory_allocated above what was allocated before the leg.  Median and p10 - p90 of --reps repetitions;
one JSON line per (shape, metric, leg).  Needs the GPU.

  python tools/boxes_batch.py [--reps 30] [--rounds 3] [--metrics iou,giou] [--parent-tree DIR] [--out profiles/boxes_batch.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (--tree: the package of another checkout, for the child process of --parent-tree)
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else ROOT
sys.path.insert(0, TREE)

SHAPES = [(1024, 64), (256, 256), (64, 1000), (64, 2048)]  # (B, N): N boxes on either side
K = 16
IOU_MIN = 0.3


def torch_stack(a, b, giou):
    """The float64 (B, N, M) cost stack by the definition's formula, in torch."""
    import torch
    ax1, ay1, ax2, ay2 = (a[:, :, None, k].double() for k in range(4))
    bx1, by1, bx2, by2 = (b[:, None, :, k].double() for k in range(4))
    area_a, area_b = (ax2 - ax1) * (ay2 - ay1), (bx2 - bx1) * (by2 - by1)
    iw = (torch.minimum(ax2, bx2) - torch.maximum(ax1, bx1)).clamp_min(0.0)
    ih = (torch.minimum(ay2, by2) - torch.maximum(ay1, by1)).clamp_min(0.0)
    inter = iw * ih
    u = (area_a + area_b) - inter
    zero = torch.zeros((), dtype=torch.float64, device=a.device)
    iou = torch.where(u > 0, inter / u, zero)
    if not giou:
        return 1.0 - iou
    hull = (torch.maximum(ax2, bx2) - torch.minimum(ax1, bx1)) * (torch.maximum(ay2, by2) - torch.minimum(ay1, by1))
    e = (hull - u).clamp_min(0.0)
    return 1.0 - (iou - torch.where(hull > 0, e / hull, zero))


def workload(B, N, giou):
    """Tracks a and detections b on the device, and the gate of the plain points call."""
    import torch
    rng = np.random.default_rng(B * 7919 + N * 31)
    side = max(np.sqrt(N) * 0.8, 2.0)
    c = rng.uniform(0, side, (B, N, 2))
    s = rng.uniform(0.6, 1.4, (B, N, 2))
    tracks = np.concatenate([c - s / 2, c + s / 2], axis=2)
    order = np.argsort(rng.random((B, N)), axis=1)
    c2 = np.take_along_axis(c, order[:, :, None], axis=1) + rng.uniform(-0.15, 0.15, (B, N, 2))
    s2 = np.take_along_axis(s, order[:, :, None], axis=1) * rng.uniform(0.9, 1.1, (B, N, 2))
    dets = np.concatenate([c2 - s2 / 2, c2 + s2 / 2], axis=2)
    a, b = (torch.from_numpy(t.astype(np.float32)).cuda() for t in (tracks, dets))
    cost = torch_stack(a[:1], b[:1], giou)[0]
    inside = float((cost <= 1.0 - IOU_MIN).double().mean())
    d0 = (a[0, :, None, :] - b[0, None, :, :]).double()
    plain_gate = float(torch.quantile((d0 ** 2).sum(-1).flatten()[:1 << 22], min(max(inside, 1.0 / (N * N)), 1.0)))
    return a, b, plain_gate


def stats(rows, name, t, peak, **more):
    t = np.array(t)
    row = dict(leg=name, reps=len(t), peak_bytes=int(peak), **more)
    for k, what in enumerate(("host_ms", "total_ms")):
        row[what] = round(float(np.median(t[:, k])), 4)
        row[what + "_p10"] = round(float(np.percentile(t[:, k], 10)), 4)
        row[what + "_p90"] = round(float(np.percentile(t[:, k], 90)), 4)
    rows.append(row)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--eps-reps", type=int, default=5, help="repetitions of leg e")
    ap.add_argument("--rounds", type=int, default=3, help="the repetitions are split over so many rounds")
    ap.add_argument("--metrics", default="iou,giou")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxes_batch.jsonl"))
    ap.add_argument("--shapes", default=None, help="BxN,...")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: leg q")
    ap.add_argument("--tree", default=None, help="(child of --parent-tree) import sslap_amd from this checkout")
    ap.add_argument("--legs", default=None, help="(child of --parent-tree) time leg p only, print the raw times")
    args = ap.parse_args()
    import torch
    import sslap_amd
    from sslap_amd import auction_solve_batch, auction_solve_points_batch
    assert os.path.dirname(os.path.dirname(os.path.abspath(sslap_amd.__file__))) == os.path.abspath(TREE)
    child = args.legs is not None
    if not child:
        from sslap_amd import auction_solve_boxes_batch, boxes_candidates
    shapes = SHAPES if not args.shapes else [tuple(int(v) for v in p.split("x")) for p in args.shapes.split(",")]
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    per_round = -(-args.reps // args.rounds)
    outside = 1.0 - IOU_MIN
    rows, raw = [], {}

    for B, N in shapes:
        for metric in args.metrics.split(","):
            giou = metric == "giou"
            a, b, plain_gate = workload(B, N, giou)
            kw = dict(fast=True, errors="status")
            with_stack = N <= 1024 and not child

            def leg(name):
                if name == "n":
                    return auction_solve_boxes_batch(a, b, metric, outside=outside, **kw)
                if name == "c":
                    return auction_solve_boxes_batch(a, b, metric, outside=outside, candidates=K, **kw)
                if name == "b":
                    return boxes_candidates(a, b, K, limit=outside, metric=metric)
                if name == "p":
                    return auction_solve_points_batch(a, b, outside=plain_gate, **kw)
                if name == "e":
                    return auction_solve_boxes_batch(a, b, metric, outside=outside, eps_start=1e-3 / N, errors="status")
                return auction_solve_batch(torch_stack(a, b, giou), outside=outside, **kw)

            legs = ["p"] if child else ["n", "c", "b", "p"] + (["t"] if with_stack else [])
            times, peaks, gaps, inside = {}, {}, [], None
            for rnd in range(args.rounds):
                if args.parent_tree and not child and metric == "iou":
                    cmd = [sys.executable, os.path.abspath(__file__), "--tree", args.parent_tree, "--legs", "p", "--reps",
                           str(per_round), "--rounds", "1", "--metrics", metric, "--shapes", f"{B}x{N}"]
                    txt = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
                    line = [ln for ln in txt.splitlines() if ln.startswith("TIMES ")][-1]
                    times.setdefault("q", []).extend(json.loads(line[6:])["p"])
                    peaks.setdefault("q", []).append(0)
                for r in range(-1 if rnd == 0 else 0, per_round):  # (r = -1: the warm-up)
                    k0 = r % len(legs)
                    done = {}
                    for name in legs[k0:] + legs[:k0]:  # (no leg always runs behind the same other)
                        sync()
                        base = torch.cuda.memory_allocated()
                        torch.cuda.reset_peak_memory_stats()
                        t0 = time.perf_counter()
                        res = leg(name)
                        t1 = time.perf_counter()
                        sync()
                        t2 = time.perf_counter()
                        done[name] = res
                        if r >= 0:
                            times.setdefault(name, []).append(((t1 - t0) * 1e3, (t2 - t0) * 1e3))
                            peaks.setdefault(name, []).append(torch.cuda.max_memory_allocated() - base)
                    for name in legs:
                        if name != "b":
                            assert not done[name]["status"].any(), name
                    if r >= 0 and not child:
                        inside = float((done["b"]["counts"].double()).mean())
                        if with_stack:
                            gaps.append(float((done["t"]["meta"]["obj_f64"] - done["n"]["meta"]["obj_f64"]).abs().mean()))
                    last = done
                    del done, res
            if child:
                raw["p"] = times["p"]
                continue
            # the eps trade-off, behind the interleaved legs: it can be orders of magnitude slower
            eps_more = {}
            for r in range(-1, max(args.eps_reps, 1)):
                sync()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                res = leg("e")
                t1 = time.perf_counter()
                sync()
                t2 = time.perf_counter()
                if r >= 0:
                    times.setdefault("e", []).append(((t1 - t0) * 1e3, (t2 - t0) * 1e3))
                    peaks.setdefault("e", []).append(torch.cuda.max_memory_allocated() - base)
                if r == -1:
                    assert not res["status"].any()
                    fine, coarse = res["meta"], last["n"]["meta"]
                    eps_more = dict(rounds=round(float(fine["its"].double().mean()), 1),
                                    rounds_fast=round(float(coarse["its"].double().mean()), 1),
                                    obj_gap=round(float((coarse["obj_f64"] - fine["obj_f64"]).mean()), 6),
                                    obj=round(float(fine["obj_f64"].mean()), 6),
                                    unmatched_fast=round(float((last["n"]["sol"] < 0).double().sum(1).mean()), 2),
                                    unmatched=round(float((res["sol"] < 0).double().sum(1).mean()), 2))
                    if (t2 - t0) > 5.0:  # (seconds per call: one repetition is the measurement)
                        times.setdefault("e", []).append(((t1 - t0) * 1e3, (t2 - t0) * 1e3))
                        peaks.setdefault("e", []).append(torch.cuda.max_memory_allocated() - base)
                        break
            del last
            med = {name: float(np.median(np.array(t)[:, 1])) for name, t in times.items()}
            for name in legs + ["e"] + (["q"] if "q" in times else []):
                more = dict(B=B, N=N, metric=metric, outside=outside, in_gate_per_row=round(inside, 2))
                if name != "n":
                    more["over_n"] = round(med[name] / med["n"], 3)  # total time over the new call's
                if name == "t":
                    more["gap"] = round(float(np.median(gaps)), 9)
                if name == "e":
                    more.update(eps_more)
                if name == "q":
                    lo, hi = np.percentile(np.array(times["p"])[:, 1], (10, 90))
                    lo2, hi2 = np.percentile(np.array(times["q"])[:, 1], (10, 90))
                    more["medians_within_each_others_p10_p90"] = bool(lo <= med["q"] <= hi and lo2 <= med["p"] <= hi2)
                stats(rows, name, times[name], np.max(peaks[name]), **more)
    if child:
        print("TIMES " + json.dumps(raw), flush=True)
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
