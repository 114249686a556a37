"""Times of the persistent re-solve with a new objective (docs/design/07_measurement.md, "A new objective through the persistent solver")
on the 50v-10 relaxation (tests/golden/problems.json): (a) eight feasibility-pump rounds through one solver
(cuoptamd_solver_reset_objective) against a solver per round; (b) one round of K = 256 members through cuoptamd_batch_reset_objectives +
cuoptamd_batch_advance against 256 single reset_objective + advance calls.  Five alternating runs each behind one untimed pair; the
sorted times in ms go to --out as one JSON object, the medians and spreads are printed.

    python scripts/objective_resolve_time.py --out profiles/objective_resolve_times.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cuopt_amd import capi  # noqa: E402
from conftest import decode_problem  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
raw = json.load(open(os.path.join(ROOT, "tests", "golden", "problems.json")))
full = decode_problem(raw["mip-50v-10-free-bound-relaxation"])
p = {k: v for k, v in full.items() if k != "var_types"}
KW = dict(tol=1e-6, iteration_limit=50000)


def pump_objective(x, alpha):
    ints = np.asarray(full["var_types"]) == ord("I")
    lb, ub, c = p["lb"], p["ub"], np.asarray(p["c"], float)
    r = np.clip(np.round(x), lb, ub)
    at_ub = ints & (r == ub)
    at_lb = ints & ~at_ub & (r == lb)
    d = np.zeros(p["n"])
    d[at_ub], d[at_lb] = -1.0, 1.0
    return d * ((1.0 - alpha) / np.linalg.norm(d)) + (alpha / np.linalg.norm(c)) * c, float(ub[at_ub].sum() - lb[at_lb].sum())


s = capi.Solver(p, **KW)
s.advance()
plan = []
for k in range(1, 9):
    x, y, _ = s.solution()
    c, off = pump_objective(x, 0.9 ** k)
    s.reset_objective(c, objective_offset=off, init_x=x, init_y=y, **KW)
    r = s.advance()
    assert r["status_name"] == "Optimal"
    plan.append((c, off, x.copy(), y.copy(), r["steps_taken"]))


def persistent():
    t0 = time.perf_counter()
    for c, off, ix, iy, _ in plan:
        s.reset_objective(c, objective_offset=off, init_x=ix, init_y=iy, **KW)
        s.advance()
    return time.perf_counter() - t0


def per_round():
    t0 = time.perf_counter()
    for c, off, ix, iy, _ in plan:
        f = capi.Solver(dict(p, c=c, objective_offset=off), init_x=ix, init_y=iy, **KW)
        f.advance()
        f.close()
    return time.perf_counter() - t0


persistent(), per_round()  # warm
a, b = [], []
for _ in range(5):
    a.append(persistent())
    b.append(per_round())
out = dict(pump_steps=[e[4] for e in plan], pump_persistent_ms=sorted(1e3 * np.array(a)), pump_per_round_ms=sorted(1e3 * np.array(b)))
print("pump persistent ms: median %.2f (%.2f .. %.2f); solver per round ms: median %.2f (%.2f .. %.2f)" % (
    np.median(a) * 1e3, min(a) * 1e3, max(a) * 1e3, np.median(b) * 1e3, min(b) * 1e3, max(b) * 1e3), flush=True)

# (b) K = 256: the eight objectives cycled over 256 members
K = 256
solvers = [capi.Solver(p, **KW) for _ in range(K)]
batch = capi.SmallBatch(solvers)
batch.advance()
cs = [plan[l % 8][0] for l in range(K)]
offs = [plan[l % 8][1] for l in range(K)]
xs = [plan[l % 8][2] for l in range(K)]
ys = [plan[l % 8][3] for l in range(K)]
singles = [capi.Solver(p, **KW) for _ in range(K)]
for q in singles:
    q.advance()


def batched():
    t0 = time.perf_counter()
    batch.reset_objectives(cs, objective_offset=offs, init_x=xs, init_y=ys)
    t1 = time.perf_counter()
    batch.advance()
    return time.perf_counter() - t0, t1 - t0


def one_by_one():
    t0 = time.perf_counter()
    tr = 0.0
    for l, q in enumerate(singles):
        t = time.perf_counter()
        q.reset_objective(cs[l], objective_offset=offs[l], init_x=xs[l], init_y=ys[l])
        tr += time.perf_counter() - t
        q.advance()
    return time.perf_counter() - t0, tr


batched(), one_by_one()
a, b = [], []
for _ in range(5):
    a.append(batched())
    b.append(one_by_one())
a, b = np.array(a) * 1e3, np.array(b) * 1e3
got = batch.solutions()
for l in (0, 7, 255):
    np.testing.assert_array_equal(got[l][0], singles[l].solution()[0])
out.update(k256_batch_round_ms=sorted(a[:, 0]), k256_batch_reset_ms=sorted(a[:, 1]), k256_single_round_ms=sorted(b[:, 0]), k256_single_reset_ms=sorted(b[:, 1]))
out = {k: [float(v) for v in vs] for k, vs in out.items()}
print("K=256 batch round ms: median %.2f (%.2f .. %.2f), of which reset_objectives %.2f; 256 singles ms: median %.2f (%.2f .. %.2f), of which reset_objective %.2f" % (
    np.median(a[:, 0]), a[:, 0].min(), a[:, 0].max(), np.median(a[:, 1]), np.median(b[:, 0]), b[:, 0].min(), b[:, 0].max(), np.median(b[:, 1])), flush=True)
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
batch.close()
for q in solvers + singles:
    q.close()
s.close()
