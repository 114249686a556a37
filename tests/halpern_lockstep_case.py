"""The main case of tests/test_halpern_lockstep_gpu.py, importable and runnable on its own (the side-by-side test starts it in child
processes): K bound variants of one LP in reflected Halpern mode (solver mode 4), each solved by a freshly created Solver and all of
them together by a shared-matrix lockstep batch (cuoptamd_settings::halpern_lockstep), compared bit for bit.

    python tests/halpern_lockstep_case.py K LAYOUT      -> prints "identical K LAYOUT", exit status 0; an assertion otherwise
"""
import functools
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from cuopt_amd import capi, synthetic  # noqa: E402

LIMIT = 4000
KW = dict(mode=4, tol=1e-4, iteration_limit=LIMIT, halpern_lockstep=1)

KEYS_INT = ("status", "steps_taken", "attempted_steps", "num_restarts", "num_major_iterations")
KEYS_F64 = ("primal_objective", "dual_objective", "gap", "l2_primal_residual", "l2_dual_residual", "step_size", "primal_weight",
            "initial_step_size", "initial_primal_weight")
KEYS_HALPERN = ("r", "r_first", "r2", "r2_min", "k")


def variants(p, k, seed=3):
    """tests/test_shared_batch_gpu.py's: k LPs over p's matrix, the first p itself, the others with some bounds tightened around the
    known optimum or a few variables fixed (the first l sets do not depend on k)"""
    rng = np.random.default_rng(seed)
    x = p["x_star"]
    out = [(np.array(p["lb"], float), np.array(p["ub"], float))]
    for l in range(1, k):
        lb, ub = np.array(p["lb"], float), np.array(p["ub"], float)
        cols = rng.choice(p["n"], size=p["n"] // (4 + l), replace=False)
        for j in cols:
            if l % 3 == 2:
                ub[j] = lb[j] if np.isfinite(lb[j]) else ub[j]
            elif rng.random() < 0.5:
                ub[j] = x[j] + 0.3 * rng.random()
            else:
                lb[j] = max(lb[j], x[j] - 0.3 * rng.random())
        out.append((lb, ub))
    return out


def state(solver, result):
    """everything the contract covers: the result's integers and doubles, x / y / reduced costs, the Halpern scalars"""
    return result, solver.solution(), solver.device.halpern()


def same(a, b, what):
    (ra, sa, ha), (rb, sb, hb) = a, b
    for k in KEYS_INT + KEYS_F64:
        assert ra[k] == rb[k], (what, k, ra[k], rb[k])
    for u, v, name in zip(sa, sb, ("x", "y", "reduced cost")):
        np.testing.assert_array_equal(u, v, err_msg="%s: %s" % (what, name))
    for k in KEYS_HALPERN:
        assert ha[k] == hb[k], (what, k, ha[k], hb[k])


def layout_is(solver, layout):
    lay = solver.device.layout()
    assert lay["A"]["layout"] == layout and lay["At"]["layout"] == layout, lay


@functools.lru_cache(maxsize=None)
def main_lp():
    p = synthetic.generate(6000, 5000, 8, seed=33)
    return p, variants(p, 16, seed=7)


@functools.lru_cache(maxsize=None)
def main_singles(layout):
    """the sixteen single solves under CUOPT_AMD_SPMV_LAYOUT = layout (set by the caller): per LP the state after 130 iterations and
    at the end.  Computed once per layout and shared, never changed."""
    assert os.environ.get("CUOPT_AMD_SPMV_LAYOUT") == layout
    p, bounds = main_lp()
    out = []
    for lb, ub in bounds:
        s = capi.Solver(dict(p, lb=lb, ub=ub), **KW)
        layout_is(s, layout)
        a = state(s, s.advance(130))
        out.append((a, state(s, s.advance())))
        s.close()
    return out


def make_batch(p, bounds, **kw):
    parent = capi.Solver(dict(p, lb=bounds[0][0], ub=bounds[0][1]), **kw)
    solvers = [parent] + [parent.clone(lb=lb, ub=ub) for lb, ub in bounds[1:]]
    return solvers, capi.SharedMatrixBatch(solvers)


def close_all(batch, solvers):
    batch.close()
    for s in solvers[1:]:
        s.close()
    solvers[0].close()


def trajectories(k, layout, singles=None):
    """case 1: the batch against the single solves after advance(130) and at the end; members rest and restart at different steps"""
    p, bounds = main_lp()
    single = (singles or main_singles(layout))[:k]
    solvers, batch = make_batch(p, bounds[:k], **KW)
    layout_is(solvers[0], layout)
    got = batch.advance(130)
    for l in range(k):
        same(state(solvers[l], got[l]), single[l][0], "LP %d after 130 iterations" % l)
    got = batch.advance()
    for l in range(k):
        same(state(solvers[l], got[l]), single[l][1], "LP %d at the end" % l)
    assert len({g["steps_taken"] for g in got}) > 1, [g["steps_taken"] for g in got]
    if k >= 4:
        assert len({g["num_restarts"] for g in got}) > 1, [g["num_restarts"] for g in got]
    return solvers, batch, single


if __name__ == "__main__":
    k, layout = int(sys.argv[1]), sys.argv[2]
    os.environ["CUOPT_AMD_SPMV_LAYOUT"] = layout
    p, bounds = main_lp()
    singles = []
    for lb, ub in bounds[:k]:  # (only the k this process needs)
        s = capi.Solver(dict(p, lb=lb, ub=ub), **KW)
        a = state(s, s.advance(130))
        singles.append((a, state(s, s.advance())))
        s.close()
    solvers, batch, _ = trajectories(k, layout, singles)
    close_all(batch, solvers)
    print("identical %d %s" % (k, layout))
