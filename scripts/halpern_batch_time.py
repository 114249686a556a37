#!/usr/bin/env python3
"""What K reflected-Halpern LPs in K workgroups are worth on bench.py's c5 pattern (docs/design/07_measurement.md, "Halpern mode").

    scripts/halpern_batch_time.py [--k 64 256 1024] [--tol 1e-4 1e-8] [--runs 5] [--sample 32] [--budget-seconds S] [--out FILE]

The pattern is bench.py --workload c5_batch<K>'s: K copies of the 50v-10 LP relaxation are K open nodes of a branch-and-bound tree; a
round tightens, in every node, the bound of one integer variable that the relaxation left fractional and re-solves from the node's own
last primal / dual.  Round 0 (the cold root relaxations) is not timed; six rounds are.  Three ways through the same nodes, on the same
build, in alternating order, `--runs` times each:
  halpern_batch     mode 4, halpern_resident = 1, halpern_batch = 1: one cuoptamd_batch_branch + one cuoptamd_batch_advance + one
                    cuoptamd_batch_solution_views per round (K workgroups per launch)
  halpern_serial    mode 4, halpern_resident = 1: the nodes through their own resident loops one after the other (Solver.reset from the
                    solution read back, Solver.advance, Solver.solution) -- what a caller of mode 4 had before the option.  A serial rate
                    does not depend on K: measured on the first `--sample` nodes
  averaging_batch   mode 1 (Stable2): the K-workgroup batch of the averaging iteration, bench.py's own line
One JSON line per (K, tolerance, way): re-solves/s over reset + advance + read-back (median, min, max of the runs), aggregate steps/s
inside advance, steps per re-solve, verdicts.  The branching variables are chosen from each way's own solutions with the same seeds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cuopt_amd import capi  # noqa: E402

ROUNDS = 6


def base_lp():
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "problems.json")))["mip-50v-10-free-bound-relaxation"]
    dec = lambda v: np.array([np.inf if x == "inf" else -np.inf if x == "-inf" else x for x in v], dtype=np.float64)
    base = dict(m=gold["m"], n=gold["n"], offsets=np.array(gold["offsets"], np.int32), indices=np.array(gold["indices"], np.int32),
                values=dec(gold["values"]), c=dec(gold["c"]), lo=dec(gold["lo"]), hi=dec(gold["hi"]), lb=dec(gold["lb"]), ub=dec(gold["ub"]),
                maximize=bool(gold["maximize"]), objective_offset=float(gold["objective_offset"]))
    return base, np.array([t == "I" for t in gold["var_types"]])


def branch(l, lb, ub, x, rng, integer):
    """bench.py's: an integer variable with a fractional relaxation value (a random integer one when all are integral); -1: none"""
    frac = np.abs(x - np.round(x))
    cand = np.flatnonzero(integer & (frac > 1e-3) & (ub - lb >= 1.0))
    if len(cand) == 0:
        cand = np.flatnonzero(integer & (ub - lb >= 1.0))
    if len(cand) == 0:
        return -1
    j = int(rng.choice(cand))
    if l % 2 == 0:
        ub[j] = max(np.floor(x[j]), lb[j])
    else:
        lb[j] = min(np.ceil(x[j]), ub[j])
    return j


class Way:
    def __init__(self, name, base, integer, count, batched, **kw):
        self.name, self.base, self.integer, self.k, self.runs = name, base, integer, count, []
        self.solvers = [capi.Solver(base, **kw) for _ in range(count)]
        self.batch = capi.SmallBatch(self.solvers) if batched else None

    def run(self):
        k, base = self.k, self.base
        rng = np.random.default_rng(17)
        lbs, ubs = [base["lb"].copy() for _ in range(k)], [base["ub"].copy() for _ in range(k)]
        if self.batch is not None:
            self.batch.reset(lb=lbs, ub=ubs)
        else:
            for s in self.solvers:
                s.reset(lb=base["lb"], ub=base["ub"])
        pipeline = advance = 0.0
        steps, verdicts, prev = 0, {}, None
        for r in range(ROUNDS + 1):
            var = np.full(k, -1, np.int32)
            if r:
                for l in range(k):
                    var[l] = branch(l, lbs[l], ubs[l], prev[l][0], rng, self.integer)
            t0 = time.perf_counter()
            if self.batch is not None:
                if r:
                    jv = np.maximum(var, 0)
                    self.batch.branch(var, np.array([lbs[l][jv[l]] for l in range(k)]), np.array([ubs[l][jv[l]] for l in range(k)]))
                t1 = time.perf_counter()
                rs = self.batch.advance()
                t2 = time.perf_counter()
                prev = self.batch.solution_views()
            else:
                rs, sols, t_adv = [], [], 0.0
                for l, s in enumerate(self.solvers):
                    if r:
                        s.reset(lb=lbs[l], ub=ubs[l], init_x=prev[l][0], init_y=prev[l][1])
                    ta = time.perf_counter()
                    rs.append(s.advance())
                    t_adv += time.perf_counter() - ta
                    sols.append(s.solution())
                prev = sols
                t1, t2 = t0, t0 + t_adv
            t3 = time.perf_counter()
            if r:
                pipeline += t3 - t0
                advance += t2 - t1
                steps += sum(q["steps_taken"] for q in rs)
                for q in rs:
                    verdicts[q["status_name"]] = verdicts.get(q["status_name"], 0) + 1
        self.runs.append(dict(lps_per_sec=k * ROUNDS / pipeline, steps_per_sec=steps / advance, steps_per_lp=steps / (k * ROUNDS), verdicts=verdicts))

    def line(self, K, tol):
        rate = sorted(q["lps_per_sec"] for q in self.runs)
        agg = sorted(q["steps_per_sec"] for q in self.runs)
        mid = lambda v: round(float(np.median(v)), 1)
        return dict(K=K, tol=tol, way=self.name, nodes_measured=self.k, rounds=ROUNDS, runs=len(self.runs), re_solves_per_sec=mid(rate),
                    re_solves_per_sec_min=round(rate[0], 1), re_solves_per_sec_max=round(rate[-1], 1), steps_per_sec_aggregate=mid(agg),
                    steps_per_sec_min=round(agg[0], 1), steps_per_sec_max=round(agg[-1], 1), steps_per_re_solve=round(self.runs[-1]["steps_per_lp"], 1),
                    verdicts=self.runs[-1]["verdicts"])

    def close(self):
        if self.batch is not None:
            self.batch.close()
        for s in reversed(self.solvers):
            s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--k", type=int, nargs="*", default=[64, 256, 1024])
    ap.add_argument("--tol", type=float, nargs="*", default=[1e-4, 1e-8])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sample", type=int, default=32, help="nodes of the serial way")
    ap.add_argument("--limit", type=int, default=20000, help="iteration limit of a re-solve")
    ap.add_argument("--budget-seconds", type=float, default=0.0, help="> 0: no further (K, tolerance) is started after this many seconds")
    ap.add_argument("--out", help="append the JSON lines to this file")
    args = ap.parse_args()
    base, integer = base_lp()
    start = time.perf_counter()
    for K in args.k:
        for tol in args.tol:
            if args.budget_seconds > 0 and time.perf_counter() - start > args.budget_seconds:
                print(json.dumps(dict(K=K, tol=tol, skipped="time budget used up")), flush=True)
                continue
            kw = dict(tol=tol, iteration_limit=args.limit)
            ways = [Way("halpern_batch", base, integer, K, True, mode=4, halpern_resident=1, halpern_batch=1, **kw),
                    Way("halpern_serial", base, integer, min(K, args.sample), False, mode=4, halpern_resident=1, **kw),
                    Way("averaging_batch", base, integer, K, True, mode=1, **kw)]
            for w in ways:
                w.run()  # warm-up: clocks, code objects, the allocator's pools
                w.runs.clear()
            for i in range(args.runs):
                for w in ways[i % 3:] + ways[:i % 3]:
                    w.run()
            for w in ways:
                text = json.dumps(w.line(K, tol))
                print(text, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(text + "\n")
                w.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
