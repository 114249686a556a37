"""What tests/test_halpern_lockstep_rays_gpu.py shares: the family of bound variants that gives all three verdicts over ONE matrix through
bounds only, the single solves the batches are compared with (computed once per layout, never changed) and the comparisons.

The family: p0 = synthetic.generate(m, n, k, seed) with lb = 0, ub = inf; the base LP is halpern_ray_reference.with_ray_column(p0) (an
appended column of cost -1 in an appended row >= 0); member l takes halpern_lockstep_case.variants(p0, 16, seed=7)[l], its bounds extended
by the ray column's [0, 1]; l % 4 == 1: the ray column's ub becomes inf; l % 4 == 2: additionally ub = 0 on the columns of row rows[l],
rows = the rows of p0 with lo > 0.  The verdict names are those of the numpy restatement (halpern_ray_reference.detect, eps = 1e-4, both
ray tolerances 1e-8, restarts on), in both bases (generate(600, 500, 6, seed=1): at most 1960 steps; generate(6000, 5000, 8, seed=33): at
most 3000).  Several verdict ratios end within 2-3 % of the tolerance: only the NAMES are compared with this table; step counts and
figures are compared with the member's own GPU solve."""
import functools
import os

import numpy as np

import halpern_ray_reference as R
from cuopt_amd import capi, synthetic
from halpern_lockstep_case import KEYS_F64, KEYS_INT, layout_is, same, state, variants  # noqa: F401

LIMIT = 20000  # (a condition, not a measurement: the restatement needs at most 3000 steps)
BASES = {"large": (6000, 5000, 8, 33), "small": (600, 500, 6, 1)}
SINGLE = dict(mode=4, tol=1e-4, iteration_limit=LIMIT, halpern_infeasibility=1)
KW = dict(SINGLE, halpern_lockstep=1, halpern_lockstep_rays=1)
FIGURES = R.KEYS
VERDICT = {l: "Optimal" for l in (0, 3, 4, 7, 12, 15)}
VERDICT.update({l: "DualInfeasible" for l in (1, 9, 13)})
VERDICT.update({l: "PrimalInfeasible" for l in (2, 5, 6, 8, 10, 11, 14)})
RAY_VERDICTS = ("PrimalInfeasible", "DualInfeasible")


@functools.lru_cache(maxsize=None)
def family(base):
    """(the base LP, the sixteen (lb, ub))"""
    p0 = dict(synthetic.generate(*BASES[base][:3], seed=BASES[base][3]))
    p0.setdefault("lb", np.zeros(p0["n"]))
    p0.setdefault("ub", np.full(p0["n"], np.inf))
    assert np.all(np.asarray(p0["lb"]) == 0.0) and np.all(np.isinf(np.asarray(p0["ub"])))
    lp = R.with_ray_column(p0)
    rows = np.flatnonzero(np.asarray(p0["lo"], float) > 0.0)
    bounds = []
    for l, (lb, ub) in enumerate(variants(p0, 16, seed=7)):
        lb, ub = np.concatenate([lb, [0.0]]), np.concatenate([ub, [1.0]])
        if l % 4 == 1:
            ub[-1] = np.inf
        if l % 4 == 2:
            ub[R.row_columns(p0, int(rows[l]))] = 0.0
        bounds.append((lb, ub))
    return lp, bounds


def member_lp(base, l):
    lp, bounds = family(base)
    return dict(lp, lb=bounds[l][0], ub=bounds[l][1])


def figures(result):
    return tuple(result[k] for k in FIGURES)


def snapshot(solver, result, with_ray):
    """everything the contract covers at a checkpoint: halpern_lockstep_case.state, the four figures of the result, the device layer's
    figures under both reduced-cost rules (the first is what the period left where a major iteration has just run) and, for a member
    that ended with a ray verdict, the certificate"""
    probes = tuple(tuple(solver.device.halpern_eval_infeasibility(rule_finite=rule)[k] for k in FIGURES) for rule in (True, False))
    ray = solver.ray() if with_ray and result["status_name"] in RAY_VERDICTS else None
    return state(solver, dict(result)), figures(result), probes, ray


def same_snapshot(a, b, what):
    same(a[0], b[0], what)
    assert a[1] == b[1], (what, "figures", a[1], b[1])
    assert a[2] == b[2], (what, "device figures, both rules", a[2], b[2])
    assert (a[3] is None) == (b[3] is None), (what, "a certificate on one side only")
    if a[3] is not None:
        for u, v, name in zip(a[3], b[3], ("dx", "dy")):
            np.testing.assert_array_equal(u, v, err_msg="%s: %s" % (what, name))


@functools.lru_cache(maxsize=None)
def singles(base, layout, checkpoints=True):
    """the sixteen members solved by freshly created solvers with halpern_infeasibility=1 and no batch, under CUOPT_AMD_SPMV_LAYOUT =
    layout (set by the caller): per member the snapshots after advance(40), after advance(130) and at the end (checkpoints=False:
    at the end only)"""
    assert os.environ.get("CUOPT_AMD_SPMV_LAYOUT") == layout
    out = []
    for l in range(16):
        s = capi.Solver(member_lp(base, l), **SINGLE)
        layout_is(s, layout)
        steps = []
        if checkpoints:
            steps.append(snapshot(s, s.advance(40), False))
            steps.append(snapshot(s, s.advance(130), False))
        steps.append(snapshot(s, s.advance(), True))
        out.append(steps)
        s.close()
    return out


def make_batch(base, members, per_member=None, **kw):
    """a parent on the first member and clones for the others (per_member[l]: that clone's own settings), and their batch"""
    lp, bounds = family(base)
    per_member = per_member or {}
    first = members[0]
    parent = capi.Solver(dict(lp, lb=bounds[first][0], ub=bounds[first][1]), **dict(kw, **per_member.get(0, {})))
    solvers = [parent]
    for q, l in enumerate(members[1:], start=1):
        # (a clone keeps its parent's settings unless it is given settings of its own -- all of them; the mode is the parent's)
        over = {k: v for k, v in dict(kw, **per_member[q]).items() if k != "mode"} if q in per_member else {}
        solvers.append(parent.clone(lb=bounds[l][0], ub=bounds[l][1], **over))
    try:
        return solvers, capi.SharedMatrixBatch(solvers)
    except capi.CuOptError:
        for s in solvers[:0:-1] + solvers[:1]:  # (the clones before their parent)
            s.close()
        raise


def verdicts_are_the_tables(results, members):
    got = {l: r["status_name"] for l, r in zip(members, results)}
    assert got == {l: VERDICT[l] for l in members}, got
