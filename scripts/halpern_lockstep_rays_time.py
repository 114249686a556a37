#!/usr/bin/env python
"""Infeasibility detection inside the Halpern lockstep batch (kernels_batch_halpern_ray.hip; cuoptamd_settings::halpern_lockstep_rays)
against the route such LPs took before it: the clones one after the other.  One JSON line per (workload, what), printed and written to
--out, which a run replaces (default profiles/halpern_lockstep_rays.jsonl).  GPU only.

  python scripts/halpern_lockstep_rays_time.py [--workloads c2,c3] [--ks 4,8,16] [--runs 5] [--steps 400] [--what routing,price] [--out FILE]
  CUOPT_AMD_LIB=<the parent commit's libcuopt.so> python scripts/halpern_lockstep_rays_time.py --what sequential ...

Per workload (synthetic.CONFIGS: c2 = 1e5 x 1e5, the CSR stream layout; c3 = 1e6 x 1e6, the row-sum panels), K bound variants
(scripts/halpern_lockstep_time.py's: a tenth of the upper bounds tightened, seeded), solver mode 4:
  routing     per K: wall seconds of capi.batch_solve of the K LPs to 1e-8 with halpern_lockstep and halpern_infeasibility set -- with
              halpern_lockstep_rays (the lockstep batch, "shared_matrix_halpern") and without it (the clones one after the other,
              "shared_matrix": the parent commit's route for such LPs); --runs alternating runs each behind one warm-up of both; median,
              spread (max - min) and every sample.  `routes`: the lockstep median beats the sequential median by more than the two spreads
              combined -- at K = 4 the test that keeps the routing of cuoptamd_batch_solve for that layout (docs/design/07_measurement.md,
              "Halpern mode").
  sequential  the second half of `routing` alone (no field is passed that an older library does not know): the run to repeat under
              CUOPT_AMD_LIB with the parent commit's library, whose medians the routing rule is stated against.
  price       per K: AGGREGATE steps/s of the lockstep batch over --steps steps per LP (whole periods, behind a warm-up of two periods;
              tolerance 0, feasible variants) with halpern_infeasibility + halpern_lockstep_rays and without the two: what the K-wide pass
              costs a batch that never meets an infeasible member."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cuopt_amd import capi, synthetic  # noqa: E402
from halpern_lockstep_time import bound_sets  # noqa: E402


def summary(samples, digits):
    return dict(median=round(statistics.median(samples), digits), spread=round(max(samples) - min(samples), digits), samples=[round(v, digits) for v in samples])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c3")
    ap.add_argument("--ks", default="16,8,4")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--limit", type=int, default=200000)
    ap.add_argument("--what", default="routing,price")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "halpern_lockstep_rays.jsonl"))
    args = ap.parse_args()
    ks = [int(v) for v in args.ks.split(",") if v]
    what = set(args.what.split(","))
    sink = open(args.out, "w")  # (a run replaces the file: its lines are one run's)

    def emit(**line):
        text = json.dumps(line)
        print(text, flush=True)
        sink.write(text + "\n")
        sink.flush()

    for name in [w for w in args.workloads.split(",") if w]:
        p = synthetic.generate(**synthetic.CONFIGS[name])
        sets = bound_sets(p, max(ks))
        base = dict(mode=4, tol=1e-8, iteration_limit=args.limit, halpern_lockstep=1, halpern_infeasibility=1)

        def wall(lps, **over):
            t0 = time.perf_counter()
            rs = capi.batch_solve(lps, **dict(base, **over))
            dt = time.perf_counter() - t0
            return dt, capi.batch_solve_last_path(), rs

        for k in ks if what & {"routing", "sequential"} else []:
            lps = [dict(p, lb=lb, ub=ub) for lb, ub in sets[:k]]
            both = "routing" in what
            paths, checked = {}, False
            a, b = [], []
            for run in range(-1, args.runs):  # (run -1: the warm-up of both)
                if both:
                    dt, paths["lockstep"], ra = wall(lps, halpern_lockstep_rays=1)
                    if run >= 0:
                        a.append(dt)
                dt, paths["sequential"], rb = wall(lps)
                if run >= 0:
                    b.append(dt)
                if both and not checked:  # (the two routes answer alike: bit for bit, tests/test_halpern_lockstep_rays_gpu.py)
                    assert [(r["status"], r["steps_taken"]) for r in ra] == [(r["status"], r["steps_taken"]) for r in rb]
                    checked = True
            sb = summary(b, 3)
            line = dict(workload=name, what="routing" if both else "sequential", k=k, tol=1e-8, library=os.environ.get("CUOPT_AMD_LIB", "this commit"),
                        paths=paths, sequential=sb, statuses=sorted({r["status_name"] for r in rb}), steps=[int(r["steps_taken"]) for r in rb])
            if both:
                la = summary(a, 3)
                line.update(lockstep=la, ratio=round(sb["median"] / la["median"], 3), routes=bool(sb["median"] - la["median"] > la["spread"] + sb["spread"]))
            emit(**line)
        if "price" not in what:
            continue
        kw = dict(tol=0.0, halpern_lockstep=1, halpern_lockstep_rays=1)
        parent = capi.Solver(dict(p, lb=sets[0][0], ub=sets[0][1]), mode=4, **kw)
        dev = parent.device
        period = max(int(parent.hyper.major_iteration), 1)
        steps = max(args.steps // period, 1) * period
        solvers = [parent] + [parent.clone(lb, ub) for lb, ub in sets[1:max(ks)]]

        def rate(k, rays):
            for s in solvers[:k]:
                s.reset(halpern_infeasibility=rays, **kw)
            b = capi.SharedMatrixBatch(solvers[:k])
            b.advance(2 * period)
            dev.call("synchronize")
            t0 = time.perf_counter()
            b.advance(steps)
            dev.call("synchronize")
            dt = time.perf_counter() - t0
            st = b.ray_stats()
            b.close()
            return k * steps / dt, st

        for k in ks:
            rate(k, 1), rate(k, 0)  # (graphs captured, clocks up)
            a, b = [], []
            for _ in range(args.runs):
                r, st = rate(k, 1)
                a.append(r)
                b.append(rate(k, 0)[0])
            la, lb_ = summary(a, 1), summary(b, 1)
            emit(workload=name, what="price", k=k, steps_per_lp=steps, with_rays=la, without=lb_, ratio=round(la["median"] / lb_["median"], 4), ray_stats=st)
        for s in solvers[1:]:
            s.close()
        parent.close()


if __name__ == "__main__":
    main()
