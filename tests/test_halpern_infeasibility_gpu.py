"""GPU: infeasibility detection in reflected Halpern mode (solver mode 4 with cuoptamd_settings::halpern_infeasibility;
docs/design/04d_halpern_mode.md, "Infeasibility detection") against its numpy restatement (tests/halpern_ray_reference.py): the four
figures against the certificate the solver hands out, the certificate against the restatement's displacement, the verdicts in every
SpMV layout, on the resident path and in the K-workgroup batch, no effect on feasible solves, and the interfaces."""
import functools

import numpy as np
import pytest

import halpern_reference as H
import halpern_ray_reference as R
from cuopt_amd import capi, synthetic
from cuopt_amd import linear_programming as lp
from test_halpern_gpu import AFIRO, LAYOUTS, V50, close_to, golden, same_solve, scaled_problem_of
from test_halpern_ray_reference import infeasible_9x4, small_synthetic
from test_halpern_reference import synthetic_lp
from test_halpern_resident_gpu import NEOS5, SUDOKU, lp_only
from test_small_batch_gpu import same

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
ON = dict(mode=4, halpern_infeasibility=1)
LIMIT = 40000  # (a condition, not a measurement: the restatement needs at most 6040 steps)
FIGURES = R.KEYS


def with_bounds(p):
    p = dict(p)
    p.setdefault("lb", np.zeros(p["n"]))
    p.setdefault("ub", np.full(p["n"], np.inf))
    return p


def big_synthetic(seed):
    return with_bounds(synthetic.generate(2000, 3000, 8, seed=seed))


def first_row_with_positive_lo(p):
    return int(np.flatnonzero(np.asarray(p["lo"], float) > 0.0)[0])


# name -> (the LP, the verdict of the design note's table)
TABLE = {"9x4": (infeasible_9x4, "PrimalInfeasible"),
         "afiro+rows": (lambda: R.with_contradictory_rows(golden(AFIRO)), "PrimalInfeasible"),
         "50v-10+rows": (lambda: R.with_contradictory_rows(lp_only(golden(V50))), "PrimalInfeasible"),
         "neos5+rows": (lambda: R.with_contradictory_rows(lp_only(golden(NEOS5))), "PrimalInfeasible"),
         "sudoku+rows": (lambda: R.with_contradictory_rows(lp_only(golden(SUDOKU))), "PrimalInfeasible"),
         "afiro+column": (lambda: R.with_ray_column(golden(AFIRO)), "DualInfeasible"),
         "50v-10+column": (lambda: R.with_ray_column(lp_only(golden(V50))), "DualInfeasible"),
         "neos5+column": (lambda: R.with_ray_column(lp_only(golden(NEOS5))), "DualInfeasible"),
         "sudoku+column": (lambda: R.with_ray_column(lp_only(golden(SUDOKU))), "DualInfeasible"),
         "200x300 bounds": (lambda: R.with_row_columns_fixed(small_synthetic(), 116), "PrimalInfeasible")}
for _seed in (1, 2, 3):
    TABLE["2000x3000-seed%d+rows" % _seed] = (functools.partial(lambda s: R.with_contradictory_rows(big_synthetic(s)), _seed), "PrimalInfeasible")
    TABLE["2000x3000-seed%d+column" % _seed] = (functools.partial(lambda s: R.with_ray_column(big_synthetic(s)), _seed), "DualInfeasible")
for _seed in (1, 2):
    TABLE["2000x3000-seed%d bounds" % _seed] = (
        functools.partial(lambda s: R.with_row_columns_fixed(big_synthetic(s), first_row_with_positive_lo(big_synthetic(s))), _seed), "PrimalInfeasible")


@functools.lru_cache(maxsize=None)
def table_lp(name):
    return TABLE[name][0]()


def solver_in(layout, monkeypatch, p, **kw):
    """a mode-4 solver whose two sides are in `layout` ("resident": the one-workgroup loop); skips where the LP cannot take the layout"""
    if layout == "resident":
        s = capi.Solver(p, halpern_resident=1, **kw)
        assert s.device.layout()["resident"], s.device.layout()
        return s
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    s = capi.Solver(p, **kw)
    lay = s.device.layout()
    if lay["resident"] or lay["A"]["layout"] != layout or lay["At"]["layout"] != layout:
        s.close()
        pytest.skip("this LP does not take the %s layout on both sides" % layout)
    return s


def figures_of(r):
    return {k: r[k] for k in FIGURES}


# ---- 1. the figures against the certificate ---------------------------------------------------------------------------------------
FIGURE_LPS = {"9x4": infeasible_9x4, "afiro+rows": lambda: table_lp("afiro+rows"),
              "3000x2500+rows": lambda: R.with_contradictory_rows(with_bounds(synthetic.generate(3000, 2500, 8, seed=41)))}


def paths_of(names, not_resident):
    """(name, layout) over the four layouts and, for the LPs of resident size, the one-workgroup loop"""
    return [(n, l) for n in sorted(names) for l in LAYOUTS + ("resident",) if not (l == "resident" and n in not_resident)]


@pytest.mark.parametrize("name,layout", paths_of(FIGURE_LPS, {"3000x2500+rows"}))
def test_figures_are_those_of_the_certificate(name, layout, monkeypatch):
    """one period with the option on: the four result fields are ray_info of the displacement the solver hands out (whatever the
    trajectory was), at the tolerance of test_infeasibility_information_matches_oracle"""
    p = FIGURE_LPS[name]()
    s = solver_in(layout, monkeypatch, p, tol=1e-8, **ON)
    r = s.advance(40)
    assert r["steps_taken"] == 40 and r["num_major_iterations"] == 1
    dx, dy = s.ray()
    ref = R.ray_info(p, dx, dy)
    print(name, layout, figures_of(r), ref)
    assert np.any(dx != 0.0) and np.any(dy != 0.0)
    for k in FIGURES:
        assert r[k] == pytest.approx(ref[k], rel=1e-10, abs=1e-12), k
    for rule in (True, False):  # (the device layer's entry point, both reduced-cost rules; the first one is what the period left)
        got = s.device.halpern_eval_infeasibility(rule_finite=rule)
        ref = R.ray_info(p, dx, dy, finite_bounds_rule=rule)
        for k in FIGURES:
            assert got[k] == pytest.approx(ref[k], rel=1e-10, abs=1e-12), (rule, k)
    s.close()


# ---- 2. the certificate against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS + ("resident",))
def test_ray_is_the_displacement_of_the_restatement(layout, monkeypatch):
    """afiro + rows after the first period: the restatement runs on the DEVICE's scaled problem, step size and weight; allowance of
    test_step_parity for vectors after a period (1e-10 of the infinity norm)"""
    p = table_lp("afiro+rows")
    s = solver_in(layout, monkeypatch, p, tol=1e-8, **ON)
    dev = s.device
    B, vec = scaled_problem_of(dev, p)
    ctl = dev.ctl()
    it = H.HalpernIteration(B, vec["C"], vec["LB"], vec["UB"], vec["LO"], vec["HI"], ctl.step_size, ctl.primal_weight)
    for _ in range(40):
        xk, yk = it.x, it.y
        it.step()
    s.advance(40)
    dx, dy = s.ray()
    for got, ref, what in ((dx, vec["DCOL"] * (it.tx - xk), "dx"), (dy, vec["DROW"] * (it.ty - yk), "dy")):
        ok, err = close_to(got, ref, 1e-10)
        print(layout, what, "rel err %.3e" % err)
        assert ok, (layout, what, err)
    s.close()


# ---- 3. verdicts ----------------------------------------------------------------------------------------------------------------------
def check_verdict(p, r, want, solver):
    assert r["status_name"] == want and r["steps_taken"] % 40 == 0 and 0 < r["steps_taken"] <= LIMIT and r["returned_average"] == 0
    dx, dy = solver.ray()
    if want == "PrimalInfeasible":
        assert r["dual_ray_linear_objective"] > 0.0
        assert r["max_dual_ray_infeasibility"] / r["dual_ray_linear_objective"] <= 1e-8
        ratio, den = R.farkas_violation(p, dy)  # the certificate itself, on the host
        assert den > 0.0 and ratio <= 1e-6, (ratio, den)
    else:
        assert r["primal_ray_linear_objective"] < 0.0
        assert r["max_primal_ray_infeasibility"] / -r["primal_ray_linear_objective"] <= 1e-8


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(TABLE))
def test_verdicts_per_layout(name, layout, monkeypatch):
    p, want = table_lp(name), TABLE[name][1]
    s = solver_in(layout, monkeypatch, p, tol=1e-8, iteration_limit=LIMIT, **ON)
    r = s.advance()
    print(name, layout, r["status_name"], r["steps_taken"], figures_of(r))
    check_verdict(p, r, want, s)
    s.close()
    off = solver_in(layout, monkeypatch, p, mode=4, tol=1e-8, iteration_limit=400)  # without the option: into the limit, as before
    assert off.advance()["status_name"] == "IterationLimit"
    with pytest.raises(capi.CuOptError) as e:
        off.ray()
    assert e.value.code == -7
    off.close()


# ---- 4. no effect on feasible solves ------------------------------------------------------------------------------------------------
def solved(p, layout, monkeypatch, **kw):
    s = solver_in(layout, monkeypatch, p, mode=4, **kw)
    r = s.advance()
    out = (r,) + s.solution() + (s.device.loop_stats(),)
    s.close()
    return out


FEASIBLE = {"afiro": lambda: golden(AFIRO), "50v-10": lambda: lp_only(golden(V50)), "synthetic-2000x3000": lambda: synthetic_lp("synthetic-2000x3000-seed1")}


@pytest.mark.parametrize("name,layout", paths_of(FEASIBLE, {"synthetic-2000x3000"}))
def test_feasible_solves_are_unchanged(name, layout, monkeypatch):
    p = FEASIBLE[name]()
    off = solved(p, layout, monkeypatch, tol=1e-8)
    on = solved(p, layout, monkeypatch, tol=1e-8, halpern_infeasibility=1)
    assert off[0]["status_name"] == "Optimal"
    same_solve(off, on)  # status, steps, restarts, major iterations, objectives; x, y and reduced costs bit for bit
    # the pass rides on the period's own synchronisation where the evaluation does (panels, resident), and on the evaluation's elsewhere
    print(name, layout, "loop syncs off / on", off[4]["loop_syncs"], on[4]["loop_syncs"])
    assert on[4]["loop_syncs"] == off[4]["loop_syncs"]


# ---- 5. the resident loop against the multi-launch kernels -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["afiro+rows", "afiro+column", "50v-10+rows", "50v-10+column"])
def test_resident_against_multi_launch(name, monkeypatch):
    """the iterates of the two paths are bit-equal (stream layout), only the sums' order differs: the same verdict at the same step"""
    p, want = table_lp(name), TABLE[name][1]
    a = solver_in("stream", monkeypatch, p, tol=1e-8, iteration_limit=LIMIT, **ON)
    b = solver_in("resident", monkeypatch, p, tol=1e-8, iteration_limit=LIMIT, **ON)
    ra, rb = a.advance(), b.advance()
    print(name, ra["steps_taken"], rb["steps_taken"], figures_of(ra), figures_of(rb))
    check_verdict(p, rb, want, b)
    assert (ra["status_name"], ra["steps_taken"], ra["num_restarts"]) == (rb["status_name"], rb["steps_taken"], rb["num_restarts"])
    for k in FIGURES:
        assert ra[k] == pytest.approx(rb[k], rel=1e-9, abs=1e-300), k
    for u, v in zip(a.ray(), b.ray()):
        np.testing.assert_array_equal(u, v)
    a.close()
    b.close()


# ---- 6. K workgroups ---------------------------------------------------------------------------------------------------------------------
BATCH_ON = dict(mode=4, halpern_resident=1, halpern_batch=1, halpern_infeasibility=1)


def test_k_workgroups():
    members = [lp_only(golden(V50)), lp_only(golden(NEOS5)), golden(AFIRO), lp_only(golden(V50)),
               table_lp("afiro+rows"), table_lp("neos5+rows"), table_lp("afiro+column"), table_lp("50v-10+column")]
    kws = [dict(tol=1e-6), dict(tol=1e-6), dict(tol=1e-8), dict(tol=1e-4)] + [dict(tol=1e-8)] * 4
    want = []
    for p, kw in zip(members, kws):
        s = capi.Solver(p, mode=4, halpern_resident=1, halpern_infeasibility=1, iteration_limit=LIMIT, **kw)
        assert s.device.layout()["resident"]
        want.append((s.advance(), s.solution(), s.ray() if s.result.status in (2, 3) else None))
        s.close()
    assert [w[0]["status_name"] for w in want] == ["Optimal"] * 4 + ["PrimalInfeasible"] * 2 + ["DualInfeasible"] * 2
    solvers = [capi.Solver(p, iteration_limit=LIMIT, **kw, **BATCH_ON) for p, kw in zip(members, kws)]
    batch = capi.SmallBatch(solvers)
    got = batch.advance()
    for l, s in enumerate(solvers):
        same(want[l][0], got[l])  # every field of the result but the times: verdict, counters, residuals, the four figures
        for u, v in zip(want[l][1], s.solution()):
            np.testing.assert_array_equal(u, v)
        if want[l][2] is not None:
            for u, v in zip(want[l][2], s.ray()):
                np.testing.assert_array_equal(u, v)
    st = batch.stats()
    print(st)
    assert st["halpern"] == 1 and st["syncs"] == st["resets"] + st["restart_rounds"] + st["periods"]
    assert st["eval_launches"] == st["periods"]
    batch.close()
    for s in solvers:
        s.close()


def test_a_branch_that_makes_a_node_infeasible():
    """the columns of row 116 of the 200 x 300 LP fixed at 0 through the batch's reset (bounds only, as a branching does it): that member
    is PrimalInfeasible, the others get what they got before"""
    small = small_synthetic()
    members = [small, golden(AFIRO), lp_only(golden(NEOS5))]
    solvers = [capi.Solver(p, tol=1e-6, iteration_limit=LIMIT, **BATCH_ON) for p in members]
    batch = capi.SmallBatch(solvers)
    first = batch.advance()
    sols = batch.solutions()
    assert [r["status_name"] for r in first] == ["Optimal"] * 3
    ub = np.array(small["ub"], float)
    ub[R.row_columns(small, 116)] = 0.0
    batch.reset(ub=[ub, None, None])
    second = batch.advance()
    print([(r["status_name"], r["steps_taken"]) for r in second])
    check_verdict(R.with_row_columns_fixed(small, 116), second[0], "PrimalInfeasible", solvers[0])
    again = batch.solutions()
    for l in (1, 2):
        assert (second[l]["status_name"], second[l]["steps_taken"], second[l]["primal_objective"]) == (
            first[l]["status_name"], first[l]["steps_taken"], first[l]["primal_objective"])
        for u, v in zip(sols[l], again[l]):
            np.testing.assert_array_equal(u, v)
    st = batch.stats()
    assert st["syncs"] == st["resets"] + st["restart_rounds"] + st["periods"]
    batch.close()
    for s in solvers:
        s.close()


# ---- 7. interfaces ---------------------------------------------------------------------------------------------------------------------
def test_interfaces():
    st = capi.Settings()
    try:
        assert lp.CUOPT_AMD_HALPERN_INFEASIBILITY == "amd_halpern_infeasibility"
        assert int(st.get(lp.CUOPT_AMD_HALPERN_INFEASIBILITY)) == 0
        st.set(lp.CUOPT_AMD_HALPERN_INFEASIBILITY, 1)  # cuOptSetIntegerParameter
        assert int(st.get(lp.CUOPT_AMD_HALPERN_INFEASIBILITY)) == 1
        for bad in (2, -1):
            with pytest.raises(capi.CuOptError):
                st.set(lp.CUOPT_AMD_HALPERN_INFEASIBILITY, bad)
    finally:
        st.close()
    p = infeasible_9x4()
    r = capi.solve(p, method=1, pdlp_solver_mode=4, amd_halpern_infeasibility=1, iteration_limit=LIMIT)
    assert r["return_code"] == 0 and r["status"] == "PrimalInfeasible" and r["solve_info"]["halpern_infeasibility"] == 1
    assert r["solve_info"]["pdlp_algorithm"] == "reflected_halpern" and r["dual_ray_linear_objective"] > 0.0
    r = capi.solve(p, method=1, pdlp_solver_mode=4, iteration_limit=400)
    assert r["status"] == "IterationLimit" and r["solve_info"]["halpern_infeasibility"] == 0
    r = capi.solve(p, method=1, pdlp_solver_mode=4, amd_halpern_infeasibility=1, infeasibility_detection=True)  # (stays a validation error)
    assert r["return_code"] == capi.CUOPT_VALIDATION_ERROR and "Halpern" in r["error_string"]
    settings = lp.SolverSettings()
    settings.set_parameter(lp.CUOPT_METHOD, lp.SolverMethod.PDLP)
    settings.set_parameter(lp.CUOPT_PDLP_SOLVER_MODE, lp.PDLPSolverMode.Halpern1)
    settings.set_parameter(lp.CUOPT_AMD_HALPERN_INFEASIBILITY, 1)
    settings.set_parameter(lp.CUOPT_ITERATION_LIMIT, LIMIT)
    dm = lp.DataModel()
    dm.set_csr_constraint_matrix(np.asarray(p["values"], float), np.asarray(p["indices"], np.int32), np.asarray(p["offsets"], np.int32))
    dm.set_objective_coefficients(np.asarray(p["c"], float))
    dm.set_constraint_lower_bounds(p["lo"])
    dm.set_constraint_upper_bounds(p["hi"])
    dm.set_variable_lower_bounds(np.asarray(p["lb"], float))
    dm.set_variable_upper_bounds(np.asarray(p["ub"], float))
    assert lp.Solve(dm, settings).get_termination_reason() == "PrimalInfeasible"
    # the averaging modes ignore the field; detect_infeasibility stays refused under mode 4, and the refusal points at the field
    averaging = capi.Solver(golden(AFIRO), mode=1, halpern_infeasibility=1)
    assert averaging.advance()["status_name"] == "Optimal"
    averaging.close()
    with pytest.raises(capi.CuOptError) as e:
        capi.Solver(p, mode=4, detect_infeasibility=1, halpern_infeasibility=1)
    assert e.value.code == -7 and "Halpern" in str(e.value) and "detect_infeasibility" in str(e.value) and "halpern_infeasibility" in str(e.value)
    s = capi.Solver(p, mode=4)
    s.advance(40)
    with pytest.raises(capi.CuOptError) as e:  # the option is off
        s.ray()
    assert e.value.code == -7
    s.close()
    s = capi.Solver(p, iteration_limit=LIMIT, **ON)
    with pytest.raises(capi.CuOptError) as e:  # nothing was evaluated yet
        s.ray()
    assert e.value.code == -7
    assert s.advance()["status_name"] == "PrimalInfeasible"
    s.reset(tol=1e-8, iteration_limit=400)  # a reset without the field switches the detection off again
    assert s.advance()["status_name"] == "IterationLimit"
    s.reset(tol=1e-8, iteration_limit=LIMIT, halpern_infeasibility=1)
    assert s.advance()["status_name"] == "PrimalInfeasible"
    s.close()


def test_a_lockstep_batch_refuses_the_field(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    p = synthetic_lp("synthetic-2000x3000-seed1")
    kw = dict(mode=4, tol=1e-4, halpern_lockstep=1, halpern_infeasibility=1)
    parent = capi.Solver(p, **kw)
    clones = [parent.clone(ub=np.full(p["n"], 50.0 + i)) for i in range(3)]  # (a clone keeps its parent's settings)
    with pytest.raises(capi.CuOptError) as e:
        capi.SharedMatrixBatch([parent] + clones)
    assert e.value.code == -7 and "halpern_infeasibility" in str(e.value)
    for c in clones:
        c.close()
    parent.close()
    lps = [dict(p, ub=np.full(p["n"], 50.0 + i)) for i in range(4)]  # cuoptamd_batch_solve: one after the other through the clones
    out = capi.batch_solve(lps, **kw)
    assert [r["status_name"] for r in out] == ["Optimal"] * 4 and capi.batch_solve_last_path() == "shared_matrix"
