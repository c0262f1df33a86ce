"""Mahalanobis costs in the points batch: auction_solve_points_batch(whiten=W, outside=gate) against what a caller with
per-track covariances did until now, and against the plain call.  On one GPU.
The workload: float32 coordinates uniform in [-1, 1)^D, N points on either side, a random SPD covariance S per row
(A A^T / D + 0.05 I with A standard normal), W = L^-1 of its Cholesky factor, and ONE chi-square gate per shape, the
quantile of the first problem's whitened costs at which about --pass columns per row pass.  fast=True, errors="status".
Per shape and D the legs, interleaved within every repetition:
  w  the whitened call: auction_solve_points_batch(x, y, whiten=W, outside=gate)
  c  the whitened list route: ... candidates=16
  b  the whitened builder alone: points_candidates(x, y, 16, limit=gate, whiten=W)
  t  the yardstick (N <= 1024, the dense batch's cap): the float64 whitened stack built on the device with torch
     (einsum of W with the (B, N, M, D) differences), then auction_solve_batch(stack, outside=gate).  torch rounds in
     another order, so `gap` is the mean |objective difference| per problem against leg w, not a comparison of bits.
  p  the plain call on the same coordinates, with the gate at the same quantile of ITS costs: w - p is the price of the
     matrix
  q  (--parent-tree DIR, a built checkout of the parent commit) leg p run there by a child process per round, the rounds
     alternating between the two trees: the plain call must not have moved.
Per leg: host_ms, the time until the call returns; total_ms, the call plus torch.cuda.synchronize(); peak_bytes,
torch.cuda.max_memory_allocated above what was allocated before the leg.  Median and p10 - p90 of --reps repetitions;
one JSON line per (shape, D, leg).  Needs the GPU.

  python tools/points_whiten.py [--reps 30] [--rounds 3] [--coords 2,4] [--parent-tree DIR] [--out profiles/points_whiten.jsonl]
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

SHAPES = [(1024, 64), (256, 256), (64, 1000), (64, 2048)]  # (B, N): N points on either side
K = 16


def workload(B, N, D, passing):
    """x, y, W on the device, and the two gates (whitened, plain)."""
    import torch
    rng = np.random.default_rng(B * 7919 + N * 31 + D)
    x = torch.from_numpy(rng.uniform(-1, 1, (B, N, D)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.uniform(-1, 1, (B, N, D)).astype(np.float32)).cuda()
    a = torch.from_numpy(rng.standard_normal((B, N, D, D))).cuda()
    s = a @ a.transpose(2, 3) / D + 0.05 * torch.eye(D, dtype=torch.float64, device="cuda")
    w = torch.linalg.solve_triangular(torch.linalg.cholesky(s), torch.eye(D, dtype=torch.float64, device="cuda").expand(B, N, D, D),
                                      upper=False).float().contiguous()
    d0 = (x[0, :, None, :] - y[0, None, :, :]).double()
    q = min(passing / N, 1.0)
    gate = float(torch.quantile(((w[0].double()[:, None] @ d0[..., None])[..., 0] ** 2).sum(-1).flatten()[:1 << 22], q))
    plain_gate = float(torch.quantile((d0 ** 2).sum(-1).flatten()[:1 << 22], q))
    return x, y, w, gate, plain_gate


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
    ap.add_argument("--rounds", type=int, default=3, help="the repetitions are split over so many rounds")
    ap.add_argument("--coords", default="2,4")
    ap.add_argument("--pass", dest="passing", type=float, default=4.0, help="columns per row inside the gate, about")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_whiten.jsonl"))
    ap.add_argument("--shapes", default=None, help="BxN,...")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: leg q")
    ap.add_argument("--tree", default=None, help="(child of --parent-tree) import sslap_amd from this checkout")
    ap.add_argument("--legs", default=None, help="(child of --parent-tree) time leg p only, print the raw times")
    args = ap.parse_args()
    import torch
    import sslap_amd
    from sslap_amd import auction_solve_batch, auction_solve_points_batch, points_candidates
    assert os.path.dirname(os.path.dirname(os.path.abspath(sslap_amd.__file__))) == os.path.abspath(TREE)
    shapes = SHAPES if not args.shapes else [tuple(int(v) for v in p.split("x")) for p in args.shapes.split(",")]
    coords = [int(v) for v in args.coords.split(",")]
    child = args.legs is not None
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    per_round = -(-args.reps // args.rounds)
    rows, raw = [], {}

    for B, N in shapes:
        for D in coords:
            x, y, w, gate, plain_gate = workload(B, N, D, args.passing)
            kw = dict(fast=True, errors="status")
            with_stack = N <= 1024 and not child

            def leg(name):
                if name == "w":
                    return auction_solve_points_batch(x, y, whiten=w, outside=gate, **kw)
                if name == "c":
                    return auction_solve_points_batch(x, y, whiten=w, outside=gate, candidates=K, **kw)
                if name == "b":
                    return points_candidates(x, y, K, limit=gate, whiten=w)
                if name == "p":
                    return auction_solve_points_batch(x, y, outside=plain_gate, **kw)
                d = (x[:, :, None, :] - y[:, None, :, :]).double()  # (B, N, M, D)
                stack = (torch.einsum("bnkl,bnml->bnmk", torch.tril(w.double()), d) ** 2).sum(-1)
                del d
                return auction_solve_batch(stack, outside=gate, **kw)

            legs = ["p"] if child else ["w", "c", "b", "p"] + (["t"] if with_stack else [])
            times, peaks, gaps, inside = {}, {}, [], None
            for rnd in range(args.rounds):
                if args.parent_tree and not child:
                    cmd = [sys.executable, os.path.abspath(__file__), "--tree", args.parent_tree, "--legs", "p", "--reps",
                           str(per_round), "--rounds", "1", "--coords", str(D), "--shapes", f"{B}x{N}", "--pass",
                           str(args.passing)]
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
                            gaps.append(float((done["t"]["meta"]["obj_f64"] - done["w"]["meta"]["obj_f64"]).abs().mean()))
                    del done, res
            if child:
                raw["p"] = times["p"]
                continue
            med = {name: float(np.median(np.array(t)[:, 1])) for name, t in times.items()}
            for name in legs + (["q"] if "q" in times else []):
                more = dict(B=B, N=N, D=D, gate=round(gate, 5), in_gate_per_row=round(inside, 2))
                if name != "w":
                    more["over_w"] = round(med[name] / med["w"], 3)  # total time over the whitened call's
                if name == "t":
                    more["gap"] = round(float(np.median(gaps)), 9)
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
