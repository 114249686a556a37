#!/usr/bin/env python
"""Lockstep batches on the jagged layout (kernels_batch.hip kbj_*) against one LP at a time: one JSON line per (workload, what).  GPU only.

  python scripts/jag_batch_time.py [--workloads banded,staircase] [--rows 1000000] [--ks 2,4,8,16] [--wall-lps 16]

Per workload (1e6 x 1e6: `banded` = 10 nonzeros per row within +-2000 columns of the diagonal, `staircase` = synthetic.generate_structured):
  single      the default solver and solvers created with batch_lanes = K: iterations/s of ONE LP
  batch       K LPs (the others with a tenth of the upper bounds tightened, seeded) in lockstep on a parent created with batch_lanes = K:
              AGGREGATE iterations/s, its ratio to the default single solve, and pdlpdev_batch_time_kernels' four kernels (us) with the
              two products' fractions of 8 TB/s under the byte model below
  wall        cuoptamd_batch_solve of `wall-lps` such LPs to 1e-4, CUOPT_AMD_TUNE=shared_batch=1 (lockstep where it wins) vs 0 (independent)
Timing as bench.py's batch_line: Stable2 preset, tolerances 0, whole major-iteration periods after a warm-up of >= 2 periods, the best
of the timed windows.  Byte model of a batched product over a matrix of R rows, C columns, N nonzeros: the jagged arrays once (value +
16-bit slot per entry: 10 N) + K x (the gathered vector once, 8 C, + the epilogue's streams: 6 x 8 R on the rows of A -- y, y', lo, hi,
the interleaved copy, the running sum --, 4 x 8 R on the rows of A^T -- x, x', AtY, AtY')."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cuopt_amd import capi, synthetic  # noqa: E402

HBM = 8e12


def problem(kind, rows):
    if kind == "banded":
        return synthetic.generate(rows, rows, 10, seed=2, band=2000)
    return synthetic.generate_structured(kind, m=rows, n=rows, k=10, seed=7)


def bound_sets(p, k, seed=8):
    rng = np.random.default_rng(seed)
    out = [(np.array(p["lb"], float), np.array(p["ub"], float))]
    for _ in range(1, k):
        lb, ub = np.array(p["lb"], float), np.array(p["ub"], float)
        cols = rng.choice(p["n"], size=p["n"] // 10, replace=False)
        ub[cols] = p["x_star"][cols] + 0.3 * rng.random(len(cols))
        out.append((lb, ub))
    return out


def rate(advance, sync, period, windows=4, per=10):
    best = 0.0
    for _ in range(windows):
        sync()
        t0 = time.perf_counter()
        advance(per * period)
        sync()
        best = max(best, per * period / (time.perf_counter() - t0))
    return best


def single_rate(p, lanes):
    s = capi.Solver(p, mode=1, tol=0.0, batch_lanes=lanes)
    dev = s.device
    dev.call("prepare_graphs")
    period = max(int(s.hyper.major_iteration), 1)
    s.advance(max(2 * period, int(s.hyper.min_iteration_restart) + period))
    r = rate(s.advance, lambda: dev.call("synchronize"), period)
    lay = dev.layout()
    s.close()
    return r, lay


def batch_rate(p, k, sets):
    parent = capi.Solver(dict(p, lb=sets[0][0], ub=sets[0][1]), mode=1, tol=0.0, batch_lanes=k)
    dev = parent.device
    period = max(int(parent.hyper.major_iteration), 1)
    clones = [parent.clone(lb, ub) for lb, ub in sets[1:k]]
    b = capi.SharedMatrixBatch([parent] + clones)
    b.advance(max(2 * period, int(parent.hyper.min_iteration_restart) + period))
    r = k * rate(b.advance, lambda: dev.call("synchronize"), period, per=5)
    t = {q: v * 1e3 for q, v in b.time_kernels(20).items()}  # (ms -> us)
    b.close()
    for c in clones:
        c.close()
    parent.close()
    return r, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="banded,staircase")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--ks", default="2,4,8,16")
    ap.add_argument("--wall-lps", type=int, default=16)
    ap.add_argument("--wall-limit", type=int, default=20000)
    args = ap.parse_args()
    ks = [int(v) for v in args.ks.split(",") if v]
    for kind in [w for w in args.workloads.split(",") if w]:
        p = problem(kind, args.rows)
        m, n, nnz = p["m"], p["n"], int(len(p["values"]))
        base, lay = single_rate(p, 0)
        print(json.dumps(dict(workload=kind, what="single", batch_lanes=0, it_s=round(base, 1), layout=lay)), flush=True)
        sets = bound_sets(p, max(ks + [args.wall_lps]))
        for k in ks:
            one, lay_k = single_rate(p, k)
            try:
                agg, t = batch_rate(p, k, sets)
            except capi.CuOptError as e:  # (-7: a side the jagged lockstep products do not serve)
                print(json.dumps(dict(workload=kind, what="batch", k=k, refused=str(e), single_it_s_same_lanes=round(one, 1), layout=lay_k)), flush=True)
                continue
            ka, kt = t.get("a_dual", 0.0), t.get("at_step", 0.0)
            bytes_a = 10 * nnz + k * (8 * n + 6 * 8 * m)
            bytes_t = 10 * nnz + k * (8 * m + 4 * 8 * n)
            print(json.dumps(dict(workload=kind, what="batch", k=k, single_it_s_same_lanes=round(one, 1), aggregate_it_s=round(agg, 1),
                                  ratio_to_default_single=round(agg / base, 3), kernels_us={q: round(v, 1) for q, v in t.items()},
                                  a_dual_hbm_fraction=round(bytes_a / (ka * 1e-6) / HBM, 3) if ka else None,
                                  at_step_hbm_fraction=round(bytes_t / (kt * 1e-6) / HBM, 3) if kt else None,
                                  workgroups_a=lay_k["A"]["workgroups"], workgroups_at=lay_k["At"]["workgroups"])), flush=True)
        lps = [dict(p, lb=lb, ub=ub) for lb, ub in sets[:args.wall_lps]]
        for shared in (1, 0):
            os.environ["CUOPT_AMD_TUNE"] = "shared_batch=%d" % shared
            t0 = time.perf_counter()
            rs = capi.batch_solve(lps, tol=1e-4, iteration_limit=args.wall_limit)
            wall = time.perf_counter() - t0
            print(json.dumps(dict(workload=kind, what="wall", lps=len(lps), shared_batch=shared, seconds=round(wall, 2),
                                  statuses=sorted({r["status_name"] for r in rs}), steps=[int(r["steps_taken"]) for r in rs])), flush=True)
        os.environ.pop("CUOPT_AMD_TUNE", None)


if __name__ == "__main__":
    main()
