#!/usr/bin/env python
"""Lockstep shared-matrix batches in reflected Halpern mode (kernels_batch_halpern.hip; cuoptamd_settings::halpern_lockstep) against the
same K solvers advanced one after the other -- what cuoptamd_batch_solve does for mode-4 LPs without the option.  One JSON line per
(workload, what), printed and written to --out, which a run replaces (default profiles/halpern_lockstep.jsonl).  GPU only.

  python scripts/halpern_lockstep_time.py [--workloads c2,c3] [--ks 4,8,16] [--steps 400] [--runs 5] [--wall-lps 16] [--out FILE]
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/halpern_lockstep_time.py --trace --ks 8,16      (per-kernel times)

Per workload (synthetic.CONFIGS: c2 = 1e5 x 1e5, the CSR stream layout; c3 = 1e6 x 1e6, the row-sum panels), K bound variants (a tenth
of the upper bounds tightened, seeded), solver mode 4, tolerance 0:
  rate    per K: AGGREGATE steps/s over a fixed budget of --steps steps per LP (whole periods, behind a warm-up of two periods) through
          SharedMatrixBatch with the option, and through the same K solvers advanced one after the other; --runs alternating runs
          each (every run starts from freshly reset solvers); median, spread (max - min) and every sample.  `routes`: the lockstep
          median beats the sequential median by more than the two spreads combined -- at K = 4 the test that keeps the routing of
          cuoptamd_batch_solve for that layout (docs/design/07_measurement.md, "Halpern mode").
  wall    --wall-lps variants to 1e-8: wall seconds of capi.batch_solve with the option, without it, and under Stable2 (its lockstep batch)
  --trace only K lockstep batches of --steps steps, no baseline: the run to put under a kernel trace."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cuopt_amd import capi, synthetic  # noqa: E402


def bound_sets(p, k, seed=8):
    rng = np.random.default_rng(seed)
    out = [(np.array(p["lb"], float), np.array(p["ub"], float))]
    for _ in range(1, k):
        lb, ub = np.array(p["lb"], float), np.array(p["ub"], float)
        cols = rng.choice(p["n"], size=p["n"] // 10, replace=False)
        ub[cols] = p["x_star"][cols] + 0.3 * rng.random(len(cols))
        out.append((lb, ub))
    return out


def summary(samples):
    return dict(median=round(statistics.median(samples), 1), spread=round(max(samples) - min(samples), 1), samples=[round(v, 1) for v in samples])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c3")
    ap.add_argument("--ks", default="4,8,16")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--wall-lps", type=int, default=16)
    ap.add_argument("--wall-limit", type=int, default=200000)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "halpern_lockstep.jsonl"))
    args = ap.parse_args()
    ks = [int(v) for v in args.ks.split(",") if v]
    sink = None if args.trace else open(args.out, "w")  # (a run replaces the file: its lines are one run's)

    def emit(**line):
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    kw = dict(tol=0.0, halpern_lockstep=1)
    if args.trace:  # (plain launches: the profiler names the kernels of every step, and no graph is instantiated under it)
        kw["use_graph"] = 0
    for name in [w for w in args.workloads.split(",") if w]:
        p = synthetic.generate(**synthetic.CONFIGS[name])
        sets = bound_sets(p, max(ks + [args.wall_lps]))
        if ks:
            parent = capi.Solver(dict(p, lb=sets[0][0], ub=sets[0][1]), mode=4, **kw)
            dev = parent.device
            lay = dev.layout()
            layout = dict(A=lay["A"]["layout"], At=lay["At"]["layout"])
            period = max(int(parent.hyper.major_iteration), 1)
            steps = max(args.steps // period, 1) * period
            solvers = [parent] + [parent.clone(lb, ub) for lb, ub in sets[1:max(ks)]]
            sync = lambda: dev.call("synchronize")

            def fresh(k):
                for s in solvers[:k]:
                    s.reset(**kw)

            def lockstep(k):
                fresh(k)
                b = capi.SharedMatrixBatch(solvers[:k])
                b.advance(2 * period)
                sync()
                t0 = time.perf_counter()
                b.advance(steps)
                sync()
                dt = time.perf_counter() - t0
                b.close()
                return k * steps / dt

            def sequential(k):
                fresh(k)
                for s in solvers[:k]:
                    s.advance(2 * period)
                sync()
                t0 = time.perf_counter()
                for s in solvers[:k]:
                    s.advance(steps)
                sync()
                return k * steps / (time.perf_counter() - t0)

            for k in ks:
                if args.trace:
                    print(json.dumps(dict(workload=name, what="trace", k=k, layout=layout, aggregate_steps_s=round(lockstep(k), 1))), flush=True)
                    continue
                lockstep(k), sequential(k)  # (graphs captured, clocks up)
                a, b = [], []
                for _ in range(args.runs):
                    a.append(lockstep(k))
                    b.append(sequential(k))
                la, sb = summary(a), summary(b)
                emit(workload=name, what="rate", k=k, layout=layout, steps_per_lp=steps, lockstep=la, sequential=sb,
                     ratio=round(la["median"] / sb["median"], 3), routes=bool(la["median"] - sb["median"] > la["spread"] + sb["spread"]))
            for s in solvers[1:]:
                s.close()
            parent.close()
        if args.trace or args.wall_lps < 4:
            continue
        lps = [dict(p, lb=lb, ub=ub) for lb, ub in sets[:args.wall_lps]]
        for what, over in (("halpern_lockstep", dict(mode=4, halpern_lockstep=1)), ("halpern_sequential", dict(mode=4)), ("stable2_lockstep", dict(mode=1))):
            t0 = time.perf_counter()
            rs = capi.batch_solve(lps, tol=1e-8, iteration_limit=args.wall_limit, **over)
            wall = time.perf_counter() - t0
            emit(workload=name, what="wall", way=what, lps=len(lps), tol=1e-8, seconds=round(wall, 2), path=capi.batch_solve_last_path(),
                 statuses=sorted({r["status_name"] for r in rs}), steps=[int(r["steps_taken"]) for r in rs])


if __name__ == "__main__":
    main()
