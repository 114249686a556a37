#!/usr/bin/env python
"""The K-workgroup Halpern batch with its major iterations decided on the device (cuoptamd_batch_set_halpern_device_major; kernels:
kernels_halpern_major.hip) against the host-decided round.  One JSON line per P, printed and written to --out, which a run replaces
unless --append is given (default profiles/halpern_batch_major.jsonl).  GPU only.

  CUOPT_AMD_LIB=<the parent commit's libcuopt.so> python scripts/halpern_batch_major_time.py --ps 0
  python scripts/halpern_batch_major_time.py --ps 0,1,4,8,16 --append --baseline profiles/halpern_batch_major.jsonl

Workload: the 256 nodes of the 50v-10 relaxation as bench.py's c5_batch256 builds them (K copies of the relaxation, the root solved in
every node, then one bound of a fractional integer variable tightened per node: down-branch in even nodes, up-branch in odd ones, seed
17), under mode=4, halpern_resident=1, halpern_batch=1.  A cycle: batch.reset to the nodes' bounds (a cold start), then batch.advance
to the default 1e-4.  Per P: --runs cycles, the P taking turns inside every run, behind one warm-up cycle of each; the profiler off.
  resolves_per_sec      K / (reset + advance) seconds: median, spread (max - min) and every sample
  syncs_per_period, launches_per_period   from the batch's counters over one cycle's advance (launches: loop, evaluation, decision,
                        restart and arming kernels; a period: one major iteration of the whole batch, host-decided or inside a burst)
The P = 0 line of the PARENT commit is taken by the first command (an older library has no setter: only --ps 0 runs there).  With
--baseline the lines of this run carry, against that line: the ratio of the medians, whether the slowest run here is above the fastest
run there, and the gain as a multiple of the parent's spread.  The script checks once that every P gives the same bits (status, step,
restart and major-iteration counts, x, y, reduced costs of every node)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cuopt_amd import capi  # noqa: E402


def summary(samples, digits):
    return dict(median=round(statistics.median(samples), digits), spread=round(max(samples) - min(samples), digits), samples=[round(v, digits) for v in samples])


def relaxation():
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "problems.json")))["mip-50v-10-free-bound-relaxation"]
    dec = lambda v: np.array([np.inf if x == "inf" else -np.inf if x == "-inf" else x for x in v], dtype=np.float64)
    base = dict(m=gold["m"], n=gold["n"], offsets=np.array(gold["offsets"], np.int32), indices=np.array(gold["indices"], np.int32),
                values=dec(gold["values"]), c=dec(gold["c"]), lo=dec(gold["lo"]), hi=dec(gold["hi"]), lb=dec(gold["lb"]), ub=dec(gold["ub"]),
                maximize=bool(gold["maximize"]), objective_offset=float(gold["objective_offset"]))
    return base, np.array([t == "I" for t in gold["var_types"]])


def nodes(base, integer, roots, K):
    """bench.py's branch per node on the root relaxation's solution: (lbs, ubs)"""
    rng = np.random.default_rng(17)
    lbs, ubs = [base["lb"].copy() for _ in range(K)], [base["ub"].copy() for _ in range(K)]
    for l in range(K):
        x, lb, ub = roots[l][0], lbs[l], ubs[l]
        frac = np.abs(x - np.round(x))
        cand = np.flatnonzero(integer & (frac > 1e-3) & (ub - lb >= 1.0))
        if len(cand) == 0:
            cand = np.flatnonzero(integer & (ub - lb >= 1.0))
        if len(cand) == 0:
            continue
        j = int(rng.choice(cand))
        if l % 2 == 0:
            ub[j] = max(np.floor(x[j]), lb[j])
        else:
            lb[j] = min(np.ceil(x[j]), ub[j])
    return lbs, ubs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ps", default="0,1,4,8,16")
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--limit", type=int, default=4000)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--baseline", default=None, help="a file of this script's lines: the parent commit's P = 0 line is compared against")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "halpern_batch_major.jsonl"))
    args = ap.parse_args()
    ps = [int(v) for v in args.ps.split(",") if v]
    library = os.environ.get("CUOPT_AMD_LIB", "this commit")
    has_setter = hasattr(capi.lib, "cuoptamd_batch_set_halpern_device_major")
    if not has_setter and ps != [0]:
        sys.exit("this library has no cuoptamd_batch_set_halpern_device_major: --ps 0 only")
    parent = None
    if args.baseline:
        for text in open(args.baseline):
            line = json.loads(text)
            if line.get("p") == 0 and line.get("library") != "this commit":
                parent = line
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    sink = open(args.out, "a" if args.append else "w")

    def emit(**line):
        text = json.dumps(line)
        print(text, flush=True)
        sink.write(text + "\n")
        sink.flush()

    K = args.k
    base, integer = relaxation()
    solvers = [capi.Solver(base, mode=4, halpern_resident=1, halpern_batch=1, iteration_limit=args.limit) for _ in range(K)]
    batch = capi.SmallBatch(solvers)
    batch.advance()  # the root relaxation in every node
    lbs, ubs = nodes(base, integer, batch.solutions(), K)

    def counters():
        st = batch.stats()
        bs = batch.burst_stats() if has_setter else dict(bursts=0, periods=0, records=0, empty_periods=0)
        return st, bs

    def cycle(P):
        if has_setter:
            batch.set_halpern_device_major(P)
        t0 = time.perf_counter()
        batch.reset(lb=lbs, ub=ubs)
        s0, b0 = counters()
        rs = batch.advance()
        dt = time.perf_counter() - t0
        s1, b1 = counters()
        d = {k: s1[k] - s0[k] for k in ("loop_launches", "eval_launches", "periods", "restart_rounds", "syncs")}
        db = {k: b1[k] - b0[k] for k in b1}
        periods = d["periods"] + db["periods"]
        launches = d["loop_launches"] + d["eval_launches"] + 2 * d["restart_rounds"] + 3 * db["periods"] + db["bursts"]
        return K / dt, rs, dict(periods=periods, syncs_per_period=round(d["syncs"] / periods, 3), launches_per_period=round(launches / periods, 3), bursts=db["bursts"],
                                empty_member_periods=db["empty_periods"], restart_rounds=d["restart_rounds"])

    def snapshot(rs):
        return [(r["status"], r["steps_taken"], r["num_restarts"], r["num_major_iterations"]) for r in rs], [tuple(a.copy() for a in s) for s in batch.solutions()]

    first = None
    for P in ps:  # the warm-up cycle of each P, and the bit check
        _, rs, _ = cycle(P)
        snap = snapshot(rs)
        if first is None:
            first = snap
        assert snap[0] == first[0], ("counts differ", P)
        for u, v in zip(snap[1], first[1]):
            assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(u, v)), ("solutions differ", P)
    samples, shape = {P: [] for P in ps}, {}
    for _ in range(args.runs):
        for P in ps:
            rate, rs, shape[P] = cycle(P)
            samples[P].append(rate)
    statuses = sorted({r["status_name"] for r in rs})
    for P in ps:
        line = dict(workload="c5_batch%d nodes, mode 4 resident batch" % K, p=P, k=K, library=library, tol=1e-4, runs=args.runs, resolves_per_sec=summary(samples[P], 1),
                    steps_total=int(sum(c[1] for c in first[0])), statuses=statuses, same_bits_for_every_p=len(ps) > 1, **shape[P])
        if parent is not None:
            mine, theirs = line["resolves_per_sec"], parent["resolves_per_sec"]
            line.update(ratio_to_parent=round(mine["median"] / theirs["median"], 4), slowest_above_parents_fastest=bool(min(mine["samples"]) > max(theirs["samples"])),
                        gain_in_parent_spreads=round((mine["median"] - theirs["median"]) / theirs["spread"], 2) if theirs["spread"] > 0 else None)
        emit(**line)
    batch.close()
    for s in solvers:
        s.close()


if __name__ == "__main__":
    main()
