"""Partial assignments from ragged packed candidate lists on the device: auction_solve_sparse_batch(outside=) against the
two routes a caller had before it.  On one GPU, in one process.  The batches have the sizes of tools/sparse_batch.py's
table (B problems of N rows and N columns, K entries per row there): here row i holds len_i distinct columns, len_i drawn
uniformly from 0 .. 2K (so the mean is K and about 1 row in 2K + 1 has no entry), uniform [0, 100) doubles, the last row
holding column N - 1 (so m_b = N for every problem); loc int32 / val float64 device tensors, offsets on the host, and a
float64 (B, N) device tensor of outside values drawn like the values.  Legs, interleaved within every repetition, every
solve with the options the outside mode resolves to (fast=True):
  o   auction_solve_sparse_batch(loc, val, offsets, sizes=, dims=(N, N), outside=outside, errors="status")
  a   auction_solve_sparse_batch(errors="status", fast=True) on the explicitly augmented packed problem built beforehand:
      one more entry (i, N + i) behind every row, new loc / val / offsets, sizes = (2 N, N); needs N + N <= 2048
  ab  the same call, the time to build those arrays (a stable sort of the entries and the outside entries by row) included
  e   auction_solve_ell_batch(cols, vals, n_cols=N, outside=outside, errors="status") on the same problems padded with
      holes to the longest row of the batch, the stack built beforehand
  eb  the same call, the padding (the slot of every entry from the row starts, one scatter) included
Per leg: host_ms, the time until the call returns; total_ms, the call plus torch.cuda.synchronize(); stream_ms, the time
of everything the leg put on the stream, from events around it.  Median and p10 - p90 of --reps repetitions; one JSON
line per (shape, leg).  Before anything is timed the legs are compared: the same assignment and the same prices.  Needs
the GPU.

  python tools/sparse_outside.py [--reps 30] [--out profiles/sparse_outside.jsonl] [--shapes 1024x64x8,...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sparse_batch import SHAPES  # noqa: E402

CAP = 2048  # MISSLAP_SPARSE_BATCH_MAX_DIM


def ragged_batch(B, N, K, seed):
    """(loc, val, offsets): B problems of N rows, row lengths uniform in 0 .. min(2 K, N), distinct columns per row."""
    rng = np.random.default_rng(seed)
    W = min(2 * K, N)
    locs = []
    for _ in range(B):
        cols = np.argpartition(rng.random((N, N)), W - 1, axis=1)[:, :W] if W < N else np.argsort(rng.random((N, N)), axis=1)
        lens = rng.integers(0, W + 1, N)
        lens[N - 1] = max(lens[N - 1], 1)
        cols[N - 1, 0] = N - 1
        keep = np.arange(W)[None, :] < lens[:, None]
        locs.append(np.stack([np.nonzero(keep)[0], cols[keep]], axis=1).astype(np.int32))
    loc = np.ascontiguousarray(np.concatenate(locs))
    offsets = np.concatenate([[0], np.cumsum([x.shape[0] for x in locs])]).astype(np.int64)
    return loc, rng.uniform(0.0, 100.0, loc.shape[0]), offsets


def row_keys(loc, counts, N):
    """b * N + row of every packed entry (counts: the entries per problem, a device tensor)."""
    import torch
    prob = torch.repeat_interleave(torch.arange(counts.shape[0], device=loc.device), counts)
    return prob * N + loc[:, 0].long()


def augment(loc, val, counts, outside, N):
    """The packed arrays a caller builds by hand: (i, N + i) with the row's outside value behind every row."""
    import torch
    B = counts.shape[0]
    rows = torch.arange(B * N, device=loc.device)
    order = torch.sort(torch.cat([row_keys(loc, counts, N), rows]), stable=True).indices
    extra = torch.stack([rows % N, N + rows % N], dim=1).to(loc.dtype)
    return torch.cat([loc, extra])[order].contiguous(), torch.cat([val, outside.reshape(-1)])[order].contiguous()


def pad(loc, val, counts, N):
    """The (B, N, K) stack of the ELL batch: K the longest row, holes at column -1."""
    import torch
    B = counts.shape[0]
    keys = row_keys(loc, counts, N)
    lens = torch.bincount(keys, minlength=B * N)
    K = max(int(lens.max()), 1)
    slot = torch.arange(keys.shape[0], device=loc.device) - (torch.cumsum(lens, 0) - lens)[keys]
    cols = torch.full((B * N * K,), -1, dtype=torch.int32, device=loc.device)
    vals = torch.zeros(B * N * K, dtype=torch.float64, device=loc.device)
    at = keys * K + slot
    cols[at] = loc[:, 1]
    vals[at] = val
    return cols.view(B, N, K), vals.view(B, N, K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_outside.jsonl"))
    ap.add_argument("--shapes", default=None, help="BxNxK,...")
    args = ap.parse_args()
    import torch
    from sslap_amd import auction_solve_ell_batch, auction_solve_sparse_batch
    shapes = SHAPES if not args.shapes else [tuple(int(x) for x in p.split("x")) for p in args.shapes.split(",")]
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out_rows = []
    for B, N, K in shapes:
        loc_h, val_h, off = ragged_batch(B, N, K, seed=B * 7919 + N)
        loc, val = torch.from_numpy(loc_h).cuda(), torch.from_numpy(val_h).cuda()
        counts = torch.from_numpy(np.diff(off)).cuda()
        outside = torch.from_numpy(np.random.default_rng(B + N).uniform(0, 100, (B, N))).cuda()
        sizes = np.tile(np.array([[N, N]], dtype=np.int64), (B, 1))
        old = 2 * N <= CAP
        aug_sizes = np.tile(np.array([[2 * N, N]], dtype=np.int64), (B, 1))
        aug_off = off + N * np.arange(B + 1, dtype=np.int64)
        al, av = augment(loc, val, counts, outside, N) if old else (None, None)
        ec, evv = pad(loc, val, counts, N)
        plain = dict(sizes=aug_sizes, dims=(N, 2 * N), fast=True, errors="status")

        def leg(name):
            if name == "a":
                return auction_solve_sparse_batch(al, av, aug_off, **plain)
            if name == "ab":
                return auction_solve_sparse_batch(*augment(loc, val, counts, outside, N), aug_off, **plain)
            if name == "e":
                return auction_solve_ell_batch(ec, evv, n_cols=N, outside=outside, errors="status")
            if name == "eb":
                return auction_solve_ell_batch(*pad(loc, val, counts, N), n_cols=N, outside=outside, errors="status")
            return auction_solve_sparse_batch(loc, val, off, sizes=sizes, dims=(N, N), outside=outside, errors="status")

        ref = leg("o")
        assert not ref["status"].any()
        unmatched = float((ref["sol"] < 0).double().mean())
        legs = ["o", "a", "ab", "e", "eb"] if old else ["o", "e", "eb"]
        for name in legs[1:]:  # the legs solve the same problems to the same bits
            got = leg(name)
            assert not got["status"].any(), name
            assert torch.equal(torch.where(got["sol"] >= N, -1, got["sol"]), ref["sol"]), name
            assert torch.equal(got["prices"][:, :N].view(torch.int64), ref["prices"].view(torch.int64)), name
            op = got["prices"][:, N:] if name in ("a", "ab") else got["outside_prices"]
            assert torch.equal(op.contiguous().view(torch.int64), ref["outside_prices"].view(torch.int64)), name
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
            row = dict(B=B, N=N, K=K, leg=name, reps=len(t), nnz=int(off[-1]), ell_K=int(ec.shape[2]),
                       unmatched=round(unmatched, 4))
            for k, what in enumerate(("host_ms", "total_ms", "stream_ms")):
                row[what] = round(float(np.median(t[:, k])), 4)
                row[what + "_p10"] = round(float(np.percentile(t[:, k], 10)), 4)
                row[what + "_p90"] = round(float(np.percentile(t[:, k], 90)), 4)
            out_rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in out_rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
