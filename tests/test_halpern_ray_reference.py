"""CPU: the numpy restatement of infeasibility detection in the reflected-Halpern mode (tests/halpern_ray_reference.py) -- its four
figures against the oracle's infeasibility information, and the verdicts and step counts the design note states for it."""
import numpy as np
import pytest

import halpern_ray_reference as R
from conftest import decode_problem
from cuopt_amd import synthetic
from oracle import orcbind
from test_halpern_reference import RAW

INF = float("inf")


def infeasible_9x4():
    """the reference's infeasible C-API LP (c_api_test.c:625-757: 9 constraints, 4 variables), as tests/test_solve_gpu.py states it"""
    rhs = np.array([0.5, 3.0, 6.0, 2.0, 2.0, 5.0, 10.0, 14.0, 1.0])
    sense = "GGLLLGLLG"
    return dict(m=9, n=4, offsets=[0, 2, 4, 6, 7, 9, 10, 12, 15, 17],
                indices=[0, 1, 0, 1, 0, 1, 3, 2, 3, 2, 0, 3, 0, 1, 2, 1, 2],
                values=[-0.5, 1.0, 2.0, -1.0, 3.0, 1.0, 1.0, 3.0, -1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0],
                c=[0.0] * 4, lb=[0.0] * 4, ub=[INF] * 4,
                lo=np.array([rhs[i] if s in "GE" else -INF for i, s in enumerate(sense)]),
                hi=np.array([rhs[i] if s in "LE" else INF for i, s in enumerate(sense)]))


def afiro():
    return decode_problem(RAW["afiro"])


def small_synthetic():
    p = synthetic.generate(200, 300, 4, seed=1)
    p.setdefault("lb", np.zeros(p["n"]))
    p.setdefault("ub", np.full(p["n"], np.inf))
    return p


@pytest.mark.parametrize("rule", [True, False])
def test_ray_info_matches_the_oracle(rule):
    """the LPs and the random vectors of test_infeasibility_information_matches_oracle, at that test's tolerance"""
    for p in (synthetic.generate(3000, 2500, 8, seed=41), infeasible_9x4()):
        p = dict(p)
        p.setdefault("lb", np.zeros(p["n"]))
        p.setdefault("ub", np.full(p["n"], np.inf))
        rng = np.random.default_rng(7)
        x = np.abs(rng.standard_normal(p["n"])) * (rng.random(p["n"]) < 0.8)
        y = rng.standard_normal(p["m"])
        got = R.ray_info(p, x, y, finite_bounds_rule=rule)
        ref = orcbind.evaluate_infeasibility(p, x, y, finite_bounds_rule=rule)
        for k in ref:
            assert got[k] == pytest.approx(ref[k], rel=1e-10, abs=1e-12), k
        # ... and with signs on both vectors, as a displacement has them
        xs = rng.standard_normal(p["n"])
        got = R.ray_info(p, xs, y, finite_bounds_rule=rule)
        ref = orcbind.evaluate_infeasibility(p, xs, y, finite_bounds_rule=rule)
        for k in ref:
            assert got[k] == pytest.approx(ref[k], rel=1e-10, abs=1e-12), k


TABLE = {"9x4": (infeasible_9x4, "PrimalInfeasible", 80),
         "afiro+rows": (lambda: R.with_contradictory_rows(afiro()), "PrimalInfeasible", 1040),
         "afiro+column": (lambda: R.with_ray_column(afiro()), "DualInfeasible", 320),
         "200x300 bounds": (lambda: R.with_row_columns_fixed(small_synthetic(), 116), "PrimalInfeasible", 6040)}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_table_of_the_design_note(name):
    """restarts on, the test every 40 steps, both ray tolerances 1e-8: verdict and step count"""
    make, status, steps = TABLE[name]
    p = make()
    r = R.detect(p, eps=1e-8, tol_p=1e-8, tol_d=1e-8, max_iterations=20000)
    print(name, r["status"], r["iterations"], r["figures"])
    assert (r["status"], r["iterations"]) == (status, steps)
    f = r["figures"]
    if status == "PrimalInfeasible":
        assert f["dual_ray_linear_objective"] > 0.0
        ratio, den = R.farkas_violation(p, r["dy"])
        assert den > 0.0 and ratio <= 1e-6
    else:
        assert f["primal_ray_linear_objective"] < 0.0


def test_a_feasible_lp_gets_no_certificate():
    r = R.detect(afiro(), eps=1e-8, max_iterations=20000)
    assert r["status"] == "Optimal"
