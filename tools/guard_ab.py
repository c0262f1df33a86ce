"""The batch solves with cardinality_check=True, timed on the library MISSLAP_LIB selects: the A/B of the device-side
matching guard against an earlier library.  Same points, recipes and seeds as tools/dense_batch.py and
tools/sparse_batch.py; only the one-launch path (auction_solve_batch / auction_solve_sparse_batch) is timed: the median
wall time of the whole call with a device synchronise, and the call's check_ms / matching_ms.  A digest of every
assignment goes with each line, so that two libraries can be compared for equal results.  Run it once per library and
alternate the runs in one session (tools/guard_ab.sh).  One JSON line per point.  Needs the GPU.

  MISSLAP_LIB=<lib> python tools/guard_ab.py --label new [--reps 7] [--out file.jsonl] [--input host|device]
                                            [--pkg <dir holding the sslap_amd package that goes with the library>]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

# beyond the points of tools/sparse_batch.py: a batch just below the device guard's threshold (B >= 256), which keeps the
# host guard, and one at it
EXTRA_SPARSE = ((200, 64, 8), (256, 64, 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the lines to this file")
    ap.add_argument("--input", default="host", choices=("host", "device"))
    ap.add_argument("--which", default="dense,sparse")
    ap.add_argument("--pkg", default=None, help="import sslap_amd from this directory (an earlier library's own package)")
    args = ap.parse_args()
    import torch
    import dense_batch as dtool
    import sparse_batch as stool
    if args.pkg:  # (after the tools, which put this tree first on the path)
        sys.path.insert(0, os.path.abspath(args.pkg))
    import sslap_amd
    from sslap_amd import auction_solve_batch, auction_solve_sparse_batch
    print("sslap_amd from", os.path.dirname(sslap_amd.__file__), file=sys.stderr)
    sync = torch.cuda.synchronize
    torch.zeros(1).cuda()
    dev = args.input == "device"
    rows = []

    def timed(kind, point, call):
        res = call()  # warm-up
        digest = hashlib.sha1(np.ascontiguousarray(res["sol"].cpu().numpy() if dev else res["sol"]).tobytes()).hexdigest()
        ts, mm, cm = [], [], []
        for _ in range(args.reps):
            sync()
            t0 = time.perf_counter()
            r = call()
            sync()
            ts.append((time.perf_counter() - t0) * 1e3)
            mm.append(r["meta"]["gpu"]["matching_ms"])
            cm.append(r["meta"]["gpu"]["check_ms"])
        row = dict(lib=args.label, kind=kind, input=args.input, cardinality_check=True, **point,
                   wall_ms=round(float(np.median(ts)), 4), matching_ms=round(float(np.median(mm)), 4),
                   check_ms=round(float(np.median(cm)), 4), reps=args.reps, sol_sha1=digest[:16])
        rows.append(row)
        print(json.dumps(row), flush=True)

    if "dense" in args.which:
        for B, N in dtool.POINTS:
            for recipe in ("float", "int"):
                mats = dtool.stack(B, N, recipe, seed=B * 7919 + N)
                src = torch.from_numpy(mats).cuda() if dev else mats
                timed("dense", dict(B=B, N=N, recipe=recipe), lambda: auction_solve_batch(src, cardinality_check=True))
    if "sparse" in args.which:
        for B, N, k in tuple(stool.SHAPES) + EXTRA_SPARSE:
            loc, val, off = stool.batch(B, N, k, seed=B * 7919 + N)
            if dev:
                loc, val = torch.from_numpy(loc).cuda(), torch.from_numpy(val).cuda()
            timed("sparse", dict(B=B, N=N, per_row=k),
                  lambda: auction_solve_sparse_batch(loc, val, off, cardinality_check=True))
    if args.out:
        with open(args.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
