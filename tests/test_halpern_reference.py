"""CPU: the numpy restatement of the restarted reflected-Halpern mode (tests/halpern_reference.py) solves what the GPU tests hold the
device against -- so that a disagreement there is the device's -- and obeys Halpern's rate for a nonexpansive map."""
import json
import os

import numpy as np
import pytest

import halpern_reference as H
from conftest import GOLDEN, decode_problem
from cuopt_amd import synthetic

SYNTHETIC = {"synthetic-2000x3000-seed1": dict(m=2000, n=3000, k=6, seed=1),
             "synthetic-3000x2000-seed2": dict(m=3000, n=2000, k=5, seed=2),
             "synthetic-2000x3000-seed3-hard": dict(m=2000, n=3000, k=6, seed=3, hard=True)}
RAW = json.load(open(os.path.join(GOLDEN, "problems.json")))


def synthetic_lp(name):
    p = synthetic.generate(**SYNTHETIC[name])
    p.setdefault("lb", np.zeros(p["n"]))
    p.setdefault("ub", np.full(p["n"], np.inf))
    return p


def known_objective(name):
    """pinned_objective, else the reference's dual simplex objective (goldens); objective_star (synthetic)"""
    meta = RAW[name]
    if meta.get("pinned_objective") is not None:
        return float(meta["pinned_objective"])
    return float(meta["reference_dual_simplex"]["objective"])


@pytest.mark.parametrize("name", sorted(RAW))
def test_goldens_reach_optimal_at_1e_4(name):
    r = H.solve(decode_problem(RAW[name]), eps=1e-4, max_iterations=60000)
    ref = known_objective(name)
    assert r["status"] == "Optimal", r
    assert abs(r["objective"] - ref) <= 2e-4 * (1.0 + abs(ref))


@pytest.mark.parametrize("name", sorted(SYNTHETIC))
def test_synthetic_reach_optimal_at_1e_4(name):
    p = synthetic_lp(name)
    r = H.solve(p, eps=1e-4, max_iterations=60000)
    assert r["status"] == "Optimal", r
    assert abs(r["objective"] - p["objective_star"]) <= 2e-4 * (1.0 + abs(p["objective_star"]))


@pytest.mark.parametrize("seed", range(12))
def test_mixed_bound_lps_at_1e_8_against_highs(seed):
    """free, boxed and fixed variables, ranged and free rows, maximise, offset: the generator of test_random_lps_gpu.py"""
    from test_random_lps_gpu import highs, random_lp
    p, A = random_lp(seed)
    ref = highs(p, A)
    r = H.solve(p, eps=1e-8, max_iterations=200000)
    assert r["status"] == "Optimal", r
    assert abs(r["objective"] - ref) <= 2e-6 * (1.0 + abs(ref))


def test_fixed_point_error_obeys_halperns_rate():
    """without restarts, from z = 0: r_k (k + 1) <= 2 ||z^0 - z*||_M for every k (Halpern's rate for a nonexpansive map; T is
    nonexpansive in the metric M of PDHG when eta sigma_max < 1), z* the LP's constructed optimum, a fixed point of T"""
    p = synthetic_lp("synthetic-2000x3000-seed1")
    B, dr, dc, c, lb, ub, lo, hi = H.scaled_problem(p)
    sigma_max, products = H.power_iteration(B)
    assert 1 <= products <= H.POWER_MAX_PRODUCTS
    it = H.HalpernIteration(B, c, lb, ub, lo, hi, H.STEP_SAFETY / sigma_max, H.initial_weight(c, lo, hi))
    xs, ys = p["x_star"] / dc, p["y_star"] / dr
    txs, tys, _ = it.operator(xs, ys, it.BT @ ys)
    assert np.linalg.norm(txs - xs) <= 1e-10 and np.linalg.norm(tys - ys) <= 1e-10
    d0 = np.sqrt(it.metric2(it.x0 - xs, it.y0 - ys, it.BT @ (it.y0 - ys)))
    for k in range(400):
        r2 = it.step()
        assert r2 >= 0.0
        assert it.r * (k + 1) <= 2.0 * d0, (k, it.r, d0)
