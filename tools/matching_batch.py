"""hopcroft_solve_batch against a loop of hopcroft_solve (the host matcher), on the same graphs, on one GPU box.
Graphs: the dense stacks of tools/dense_batch.py (every entry >= 0, so complete graphs), the sparse batches of
tools/sparse_batch.py, and chain graphs (row i stores (i, i + 1) then (i, i); row n - 1 only (n - 1, n - 1): one
augmenting path through every row, the deepest DFS there is).  Both paths are timed as the median wall time of the
whole call (the batch with a device synchronise); the loop runs on at most --loop-max graphs and is scaled per graph.
Every graph the loop matches is compared with the batch first.  One JSON line per shape.  Needs the GPU.

  python tools/matching_batch.py [--reps 5] [--out profiles/matching_batch.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CHAINS = ((1, 2048), (64, 2048), (1024, 256))  # (B, n)


def chain(n):
    rows = np.concatenate([np.repeat(np.arange(n - 1), 2), [n - 1]])
    cols = np.concatenate([np.stack([np.arange(1, n), np.arange(n - 1)], axis=1).ravel(), [n - 1]])
    return np.ascontiguousarray(np.stack([rows, cols], axis=1), dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-max", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matching_batch.jsonl"))
    args = ap.parse_args()
    import torch
    import dense_batch as dtool
    import sparse_batch as stool
    from sslap_amd import hopcroft_solve, hopcroft_solve_batch
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    rows = []

    def run(kind, point, B, batch_call, one_call):
        res = batch_call()  # warm-up + parity
        Bl = min(B, args.loop_max)
        for b in range(Bl):
            r = one_call(b)
            n, m = r["left_pairings"].shape[0], r["right_pairings"].shape[0]
            assert res["size"][b] == r["size"], (kind, point, b)
            assert np.array_equal(res["left_pairings"][b, :n], r["left_pairings"]), (kind, point, b)
            assert np.array_equal(res["right_pairings"][b, :m], r["right_pairings"]), (kind, point, b)
        tb, tk, tl = [], [], []
        for _ in range(args.reps):
            sync()
            t0 = time.perf_counter()
            r = batch_call()
            sync()
            tb.append((time.perf_counter() - t0) * 1e3)
            tk.append(r["gpu"]["kernel_ms"])
            t0 = time.perf_counter()
            for b in range(Bl):
                one_call(b)
            tl.append((time.perf_counter() - t0) * 1e3)
        wb, wl = float(np.median(tb)), float(np.median(tl))
        row = dict(kind=kind, **point, B=B, batch_wall_ms=round(wb, 4), batch_kernel_ms=round(float(np.median(tk)), 4),
                   lds_bytes=r["gpu"]["lds_bytes"], loop_graphs_timed=Bl, loop_wall_ms_per_graph=round(wl / Bl, 5),
                   batch_graphs_per_s=round(B / (wb * 1e-3), 1), loop_graphs_per_s=round(Bl / (wl * 1e-3), 1),
                   reps=args.reps, size_mean=round(float(np.mean(res["size"])), 1))
        row["batch_vs_loop"] = round(row["batch_graphs_per_s"] / row["loop_graphs_per_s"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)

    for B, N in dtool.POINTS:
        mats = dtool.stack(B, N, "float", seed=B * 7919 + N)
        run("dense", dict(N=N), B, lambda: hopcroft_solve_batch(mats=mats), lambda b: hopcroft_solve(mat=mats[b]))
    for B, N, k in stool.SHAPES:
        loc, _, off = stool.batch(B, N, k, seed=B * 7919 + N)
        run("sparse", dict(N=N, per_row=k), B, lambda: hopcroft_solve_batch(loc, off),
            lambda b: hopcroft_solve(loc=loc[off[b]:off[b + 1]]))
    for B, n in CHAINS:
        c = chain(n)
        loc = np.ascontiguousarray(np.tile(c, (B, 1)))
        off = np.arange(B + 1, dtype=np.int64) * c.shape[0]
        run("chain", dict(N=n), B, lambda: hopcroft_solve_batch(loc, off), lambda b: hopcroft_solve(loc=c))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
