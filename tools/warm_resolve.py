"""Warm-started re-solve at the BASELINE sizes: cold solve, perturb a fraction of the values, then time
  (a) update_values + resolve(eps_start=delta) on the solved handle (its current prices),
  (b) a fresh handle on the new values with a cold solve,
  (c) a fresh handle on the new values with resolve(prices=old prices, eps_start=delta),
and the value-update pass alone (device-resident values, update_values_device) with its bandwidth.  One JSON line per
(config, perturbation).  Needs the GPU.

  python tools/warm_resolve.py [--configs C2,C3] [--reps 5] [--out file.jsonl]

Bytes of the update pass, as the algorithm needs them: 8 B new + 8 B old value per edge (phase 1), the new value again and
the edge layout's value (phase 2: 4 B of an 8 B/edge fp32 edge, 8 B of a 12 B/edge one) and the tile-major record's value
(4 or 8 B) -- `bytes_min` -- over the measured wall time of the call (host read-back of the check included); fraction of the
8 TB/s data-sheet peak like bench.py's roofline.  A warm solve can take MORE rounds than a cold one (a price war of a large
perturbation against a small eps): the numbers are what was measured, nothing more.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PERTURBATIONS = (("1pct_pm1", 0.01, 1.0), ("10pct_pm5", 0.10, 5.0))
PEAK = 8e12


def perturb(val, frac, step, seed):
    rng = np.random.default_rng(seed)
    out = val.copy()
    idx = rng.choice(val.size, int(frac * val.size), replace=False)
    out[idx] += rng.choice([-step, step], idx.size)
    return out.astype(np.float32).astype(np.float64)  # (kept fp32-exact: the 8 B/edge layout stays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sslap_amd import from_sparse, synth
    out = open(a.out, "w") if a.out else None
    for cfg in a.configs.split(","):
        loc, A = synth.gen_config(cfg, seed=1)
        for name, frac, step in PERTURBATIONS:
            B = perturb(A, frac, step, seed=1 + PERTURBATIONS.index((name, frac, step)))
            s = from_sparse(loc, A.copy(), problem="max", cardinality_check=False)
            s.solve()
            cold_A = dict(rounds=s.meta["its"], ms=round(s.gpu["solve_ms"], 3))
            pA = s.prices
            # the update pass alone, values in HBM: alternately B and A, the last call leaves B in place
            tA, tB = torch.tensor(A, device="cuda"), torch.tensor(B, device="cuda")
            torch.cuda.synchronize()
            times = []
            for k in range(2 * a.reps + 1):
                t = tB if k % 2 == 0 else tA
                t0 = time.perf_counter()
                delta = s.update_values_device(t.data_ptr())
                times.append((time.perf_counter() - t0) * 1e3)
            upd_ms = float(np.median(times))
            nnz = int(A.size)
            tiled_val = 4 if s.gpu["tiled_format"] in (0, 2) else 8
            edge_val = 4 if s.gpu["bytes_per_edge"] == 8 else 8
            bytes_min = nnz * (8 + 8 + 8 + edge_val + (tiled_val if s.gpu["tiled_active"] else 0))
            # (a) warm on the solved handle (host values: the upload is part of what a caller pays)
            s.update_values(A)
            t0 = time.perf_counter()
            d = s.update_values(B)
            upd_host_ms = (time.perf_counter() - t0) * 1e3
            assert d == delta
            sol_a = s.resolve(eps_start=delta)
            warm = dict(rounds=s.meta["its"], nreductions=s.meta["nreductions"], ms=round(s.gpu["solve_ms"], 3),
                        start_eps=s.gpu["start_eps_f32"])
            # (b) fresh handle, cold
            t0 = time.perf_counter()
            f = from_sparse(loc, B.copy(), problem="max", cardinality_check=False)
            create_ms = (time.perf_counter() - t0) * 1e3
            f.solve()
            cold_B = dict(rounds=f.meta["its"], nreductions=f.meta["nreductions"], ms=round(f.gpu["solve_ms"], 3),
                          create_ms=round(create_ms, 3), obj_f64=f.gpu["obj_f64"])
            # (c) fresh handle, warm from the old prices
            c = from_sparse(loc, B.copy(), problem="max", cardinality_check=False)
            sol_c = c.resolve(prices=pA, eps_start=delta)
            fresh_warm = dict(rounds=c.meta["its"], ms=round(c.gpu["solve_ms"], 3))
            line = dict(config=cfg, perturbation=name, changed_fraction=frac, step=step, nnz=nnz, delta=delta,
                        cold_A=cold_A, a_update_resolve=warm, b_fresh_cold=cold_B, c_fresh_resolve_old_prices=fresh_warm,
                        a_equals_c=bool(np.array_equal(sol_a, sol_c)), warm_obj_f64=s.gpu["obj_f64"],
                        warm_soln_found=s.meta["soln_found"], cold_soln_found=f.meta["soln_found"],
                        update_pass=dict(ms_median=round(upd_ms, 4), ms_all=[round(x, 4) for x in times],
                                         host_values_ms=round(upd_host_ms, 3), bytes_min=bytes_min,
                                         GBs=round(bytes_min / (upd_ms * 1e-3) / 1e9, 1),
                                         frac_of_8TBs=round(bytes_min / (upd_ms * 1e-3) / PEAK, 4),
                                         tiled_format=s.gpu["tiled_format"] if s.gpu["tiled_active"] else None,
                                         bytes_per_edge=s.gpu["bytes_per_edge"]))
            print(json.dumps(line), flush=True)
            if out:
                out.write(json.dumps(line) + "\n")
                out.flush()
            del s, f, c, tA, tB
    if out:
        out.close()


if __name__ == "__main__":
    main()
