"""GPU: the restarted reflected-Halpern mode (solver mode 4) inside the resident one-workgroup loop (cuoptamd_settings::halpern_resident,
"amd_halpern_resident" behind cuOptSolve) -- selection, the steps bit for bit against the stream layout's multi-launch kernels and at
1e-10 against the numpy restatement, the restart decisions, whole solves, one synchronisation per period, reset, the three
interfaces, the batch refusals and the speed against the multi-launch path.

Where a resident run is compared bit for bit with a multi-launch one, both sides are created under CUOPT_AMD_SPMV_LAYOUT=stream: the
step size comes out of the power iteration, which runs the layout's plain products on either kind of context."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import halpern_reference as H
from conftest import set_tune
from cuopt_amd import capi, synthetic
from cuopt_amd import linear_programming as lp
from test_halpern_gpu import AFIRO, COD, V50, close_to, golden, restatement, same_solve, scaled_problem_of
from test_halpern_reference import RAW, known_objective
from test_random_lps_gpu import highs, random_lp

pytestmark = pytest.mark.gpu
NEOS5, SUDOKU = "mip-neos5-free-bound-relaxation", "mip-sudoku-relaxation"
FOUR = (AFIRO, V50, NEOS5, SUDOKU)
RESIDENT_GOLDENS = sorted(k for k in RAW if k != COD)  # 13 of the 14 goldens are of resident size
SHAPES = [(1800, 2000, 2), (1000, 900, 8), (200, 500, 6), (2048, 2048, 2), (40, 30, 5)]  # test_one_attempt_is_bit_identical_to_multi_launch's
BUFFERS = ("X", "Y", "ATY", "AVG_X", "AVG_Y")


def lp_only(p):
    return {k: v for k, v in p.items() if k != "var_types"}


def v50_with_tighter_bounds(factor):
    """50v-10 with its large finite upper bounds (212, 46230) scaled down.  HiGHS on the host: feasible with objectives 2914.46,
    2956.71, 3047.79, 3253.94 at factors 0.008, 0.006, 0.005, 0.004 (2879.07 unchanged; infeasible from 0.003 down)"""
    p = golden(V50)
    ub = np.asarray(p["ub"], float)
    return dict(p, ub=np.where(np.isfinite(ub) & (ub > 1.0), ub * factor, ub))


def halpern_context(p, resident, monkeypatch, eta=None, omega=None):
    """a device context in Halpern mode right before its first step: on the resident path, or kept off it (stream layout)"""
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    if p.get("maximize"):  # (the device layer takes the min-form objective, as the host driver hands it over)
        p = dict(p, c=-np.asarray(p["c"], float), maximize=False)
    capi.lib.pdlpdev_create_no_resident(0 if resident else 1)
    try:
        dev = capi.Device(p)
    finally:
        capi.lib.pdlpdev_create_no_resident(0)
    assert dev.layout()["resident"] == resident, dev.layout()
    dev.call("scaling_compute", 1, 10, 1, 1.0)
    dev.call("scale_problem")
    dev.set_halpern(True)
    if eta is None:
        sigma, _ = dev.spectral_norm()
        eta = H.STEP_SAFETY / sigma
        nr = dev.init_norms()
        omega = np.sqrt(nr[1]) / np.sqrt(nr[2]) if nr[1] > 0 and nr[2] > 0 else 1.0
    dev.call("set_step", eta, omega)
    dev.call("project_primal")
    dev.call("compute_aty")
    dev.halpern_restart(-1.0)
    return dev, p, eta, omega


def resident_solver(p, monkeypatch, stream=True, **kw):
    if stream:
        monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    s = capi.Solver(p, mode=4, halpern_resident=1, **kw)
    assert s.device.layout()["resident"], s.device.layout()
    return s


def multi_launch_solver(p, monkeypatch, **kw):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    s = capi.Solver(p, mode=4, **kw)
    lay = s.device.layout()
    assert not lay["resident"] and lay["A"]["layout"] == "stream" and lay["At"]["layout"] == "stream", lay
    return s


def finished(s):
    r = s.advance()
    x, y, z = s.solution()
    stats = s.device.loop_stats()
    s.close()
    return r, x, y, z, stats


# ---- 1. selection ------------------------------------------------------------------------------------------------------------------
def test_selection(monkeypatch):
    monkeypatch.delenv("CUOPT_AMD_SMALL", raising=False)
    for name in (AFIRO, SUDOKU, V50):  # tiers 0, 1, 2
        s = capi.Solver(golden(name), mode=4, halpern_resident=1)
        assert s.device.layout()["resident"], name
        s.close()
        s = capi.Solver(golden(name), mode=4)  # without the setting: the multi-launch kernels, as before
        assert not s.device.layout()["resident"], name
        s.close()
    for p in (golden(COD), synthetic.generate(3000, 3000, 6)):  # not of resident size: silently the multi-launch path
        s = capi.Solver(p, mode=4, halpern_resident=1)
        assert not s.device.layout()["resident"]
        s.close()
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")
    s = capi.Solver(golden(AFIRO), mode=4, halpern_resident=1)
    assert not s.device.layout()["resident"]
    assert s.advance()["status_name"] == "Optimal"
    s.close()
    monkeypatch.delenv("CUOPT_AMD_SMALL")
    # the averaging iteration ignores the field: same layout, the same 40 steps bit for bit
    got = []
    for kw in (dict(), dict(halpern_resident=1)):
        s = capi.Solver(golden(V50), mode=1, tol=0.0, **kw)
        lay = s.device.layout()
        r = s.advance(40)
        got.append((lay, r["steps_taken"], r["attempted_steps"], r["step_size"], r["primal_weight"]) + s.solution())
        s.close()
    assert got[0][:5] == got[1][:5] and got[0][0]["resident"]
    for u, v in zip(got[0][5:], got[1][5:]):
        np.testing.assert_array_equal(u, v)


# ---- 2. the steps, bit for bit against the stream layout's multi-launch kernels -------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_steps_are_bit_identical_to_the_multi_launch_kernels(shape, monkeypatch):
    p = synthetic.generate(*shape, seed=12)
    ref, _, eta, omega = halpern_context(p, False, monkeypatch)
    dev, _, _, _ = halpern_context(p, True, monkeypatch, eta, omega)
    n, m = int(p["n"]), int(p["m"])
    size = dict(X=n, Y=m, ATY=n, AVG_X=n, AVG_Y=m)
    for target in (1, 2, 40, 120):
        a, b = dev.run(target), ref.run(target)
        assert (a.k, a.steps_taken, a.attempts, a.error) == (b.k, b.steps_taken, b.attempts, b.error) == (target, target, target, 0)
        for buf in BUFFERS:
            np.testing.assert_array_equal(dev.download(buf, size[buf]), ref.download(buf, size[buf]), err_msg="%s after %d steps" % (buf, target))
        h, g = dev.halpern(), ref.halpern()
        print(shape, target, "r", h["r"], g["r"], "r_first", h["r_first"], g["r_first"])
        assert h["k"] == g["k"] == target
        assert h["r"] == pytest.approx(g["r"], rel=1e-9) and h["r_first"] == pytest.approx(g["r_first"], rel=1e-9)
        assert h["r2_min"] >= 0.0
    dev.close()
    ref.close()


# ---- 3. the steps against the restatement ----------------------------------------------------------------------------------------
STEP_LPS = {"afiro": lambda: golden(AFIRO), "50v-10": lambda: golden(V50), "neos5": lambda: golden(NEOS5), "sudoku": lambda: golden(SUDOKU),
            "mixed-40x60": lambda: random_lp(3)[0]}


@pytest.mark.parametrize("name", sorted(STEP_LPS))
def test_step_parity_with_the_restatement(name, monkeypatch):
    """test_step_parity's assertions on the resident context: x, y, A^T y and T(z^k) after steps 1, 2, 40, 120 at 1e-10 of the vector's
    infinity norm, r_k at rtol 1e-9, r_k^2 >= 0"""
    dev, p, eta, omega = halpern_context(STEP_LPS[name](), True, monkeypatch)
    B, vec = scaled_problem_of(dev, p)
    it = H.HalpernIteration(B, vec["C"], vec["LB"], vec["UB"], vec["LO"], vec["HI"], eta, omega)
    done = 0
    for target in (1, 2, 40, 120):
        ctl = dev.run(target)
        assert ctl.steps_taken == target and ctl.attempts == target and ctl.error == 0
        while done < target:
            it.step()
            done += 1
        for buf, ref in (("X", it.x), ("Y", it.y), ("ATY", it.aty), ("AVG_X", it.tx), ("AVG_Y", it.ty)):
            ok, err = close_to(dev.download(buf, len(ref)), ref, 1e-10)
            print(name, target, buf, "rel err %.3e" % err)
            assert ok, (name, target, buf, err)
        h = dev.halpern()
        print(name, target, "r", h["r"], it.r)
        assert h["k"] == target and h["r"] == pytest.approx(it.r, rel=1e-9)
        assert h["r_first"] == pytest.approx(it.r_first, rel=1e-9) and h["r_first"] > 0 and h["r2_min"] >= 0.0
    dev.close()


# ---- 4. restart decisions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FOUR)
def test_restart_decisions_follow_the_restatement(name, monkeypatch):
    """the first 10 major iterations on a resident solver: the same restart flags, the primal weight after each at rtol 1e-9.  (Over
    these periods the restatement's r / r_first stays at least 1.3e-2 away from the two thresholds on all four LPs: a 1e-9
    difference in r cannot flip a flag.)  sudoku is solved to 1e-13 at its fifth major iteration (200 steps), by the restatement
    and on the device alike: there the four periods in front of it are compared, and the solver has to end where the restatement
    ends."""
    p = golden(name)
    s = resident_solver(p, monkeypatch, stream=False, tol=1e-13)
    dev = s.device
    B, vec = scaled_problem_of(dev, p)
    ctl = dev.ctl()
    it = H.HalpernIteration(B, vec["C"], vec["LB"], vec["UB"], vec["LO"], vec["HI"], ctl.step_size, ctl.primal_weight)
    ref = H.run(p, it, vec["DROW"], vec["DCOL"], eps=1e-13, max_major=10)
    flags, weights, restarts = [], [], 0
    for _ in range(10):
        r = s.advance(40)
        if r["status"] != 0:
            break
        flags.append(r["num_restarts"] > restarts)
        restarts = r["num_restarts"]
        weights.append(r["primal_weight"])
    print(name, flags, weights, r["status_name"], r["steps_taken"], ref["status"], ref["iterations"])
    assert flags == ref["flags"]
    if name == SUDOKU:
        assert len(flags) == 4 and r["status_name"] == "Optimal" == ref["status"] and r["steps_taken"] == ref["iterations"] == 200
    else:
        assert len(flags) == 10
    np.testing.assert_allclose(weights, ref["weights"], rtol=1e-9)
    s.close()


# ---- 5. whole solves ---------------------------------------------------------------------------------------------------------------
def test_goldens_solve_in_the_resident_loop(monkeypatch):
    ran = 0
    for name in RESIDENT_GOLDENS:
        p = golden(name)
        ref = known_objective(name)
        s = resident_solver(p, monkeypatch, stream=False)
        r = s.advance()
        x, _, _ = s.solution()
        s.close()
        status, its, _ = restatement(name)
        print(name, r["status_name"], r["steps_taken"], "restatement", its, "objective", r["primal_objective"], ref)
        assert r["status_name"] == "Optimal" == status
        assert abs(r["primal_objective"] - ref) <= 2e-4 * (1.0 + abs(ref))
        assert 0.5 * its - 80 <= r["steps_taken"] <= 2.0 * its + 80
        assert r["returned_average"] == 0 and r["attempted_steps"] == r["steps_taken"] and r["step_size"] == r["initial_step_size"]
        if name == AFIRO:
            assert r["steps_taken"] == its
        ran += 1
    assert ran == 13


@pytest.mark.parametrize("tol", [1e-4, 1e-8])
@pytest.mark.parametrize("name", FOUR)
def test_solves_are_bit_identical_to_the_multi_launch_path(name, tol, monkeypatch):
    p = golden(name)
    a = finished(resident_solver(p, monkeypatch, tol=tol, iteration_limit=400000))
    b = finished(multi_launch_solver(p, monkeypatch, tol=tol, iteration_limit=400000))
    print(name, tol, a[0]["status_name"], a[0]["steps_taken"], b[0]["steps_taken"], a[0]["num_restarts"], b[0]["num_restarts"])
    assert a[0]["status_name"] == b[0]["status_name"] == "Optimal"
    for k in ("steps_taken", "num_restarts", "num_major_iterations"):
        assert a[0][k] == b[0][k], k
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])
    for k in ("primal_objective", "dual_objective"):
        assert abs(a[0][k] - b[0][k]) <= 1e-9 * (1.0 + abs(b[0][k])), k


@pytest.mark.parametrize("seed", range(12))
def test_mixed_bound_lps_at_1e_8_against_highs(seed, monkeypatch):
    p, A = random_lp(seed)
    ref = highs(p, A)
    r = capi.solve(p, method=1, pdlp_solver_mode=4, amd_halpern_resident=1, tol=1e-8, iteration_limit=200000)
    print(seed, r["status"], r["steps_taken"], abs(r["objective"] - ref))
    assert r["status"] == "Optimal" and r["solve_info"]["pdlp_algorithm"] == "reflected_halpern" and r["solve_info"]["halpern_resident"] == 1
    assert abs(r["objective"] - ref) <= 2e-6 * (1.0 + abs(ref))


# ---- 6. one synchronisation per period ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [AFIRO, V50])
def test_one_synchronisation_per_period(name, monkeypatch):
    p = golden(name)
    base = finished(resident_solver(p, monkeypatch))
    assert base[0]["status_name"] == "Optimal"
    same_solve(base, finished(resident_solver(p, monkeypatch, use_graph=0)))
    set_tune(monkeypatch, period_path="0")
    apart = finished(resident_solver(p, monkeypatch))
    set_tune(monkeypatch, period_path=None)
    same_solve(base, apart)
    majors, restarts = base[0]["num_major_iterations"], base[0]["num_restarts"]
    print(name, "loop syncs", base[4]["loop_syncs"], apart[4]["loop_syncs"], "periods", majors, "restarts", restarts)
    assert base[4]["loop_syncs"] == 1 + restarts + majors  # the anchor of the start, one per restart, ONE per period
    assert apart[4]["loop_syncs"] == 1 + restarts + 2 * majors  # steps, then the evaluation


# ---- 7. reset and re-solve ---------------------------------------------------------------------------------------------------------------
def test_reset_and_re_solve(monkeypatch):
    p = golden(V50)
    base = finished(resident_solver(p, monkeypatch))
    s = resident_solver(p, monkeypatch)
    first = (s.advance(),) + s.solution()
    s.reset()
    again = (s.advance(),) + s.solution()
    same_solve(base, first)
    same_solve(base, again)
    ub = v50_with_tighter_bounds(0.006)["ub"]  # other bounds on the same matrix: what a fresh solver on that LP gives
    s.reset(ub=ub)
    assert s.device.layout()["resident"]
    changed = (s.advance(),) + s.solution()
    s.close()
    fresh = finished(resident_solver(dict(p, ub=ub), monkeypatch))
    assert changed[0]["status_name"] == "Optimal"
    same_solve(fresh, changed)
    assert abs(changed[0]["primal_objective"] - 2956.71279777136) <= 2e-4 * 2957.7 < changed[0]["primal_objective"] - base[0]["primal_objective"]
    # the refused resets of the mode are still refused, and the solver stays usable
    q = golden(AFIRO)
    s = resident_solver(q, monkeypatch)
    for kw in (dict(detect_infeasibility=1), dict(save_best_primal_so_far=1), dict(first_primal_feasible=1), dict(initial_k=3)):
        with pytest.raises(capi.CuOptError) as e:
            s.reset(**kw)
        assert e.value.code == -7 and "Halpern" in str(e.value) and list(kw)[0] in str(e.value)
    r = s.advance()
    assert r["status_name"] == "Optimal" and r["steps_taken"] == restatement(AFIRO)[1]
    with pytest.raises(capi.CuOptError) as e:
        s.get_warm_start()
    assert e.value.code == -7 and "Halpern" in str(e.value)
    s.close()


# ---- 8. interfaces -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [AFIRO, V50])
def test_interfaces(name):
    p = lp_only(golden(name))
    ref = known_objective(name)
    _, its, _ = restatement(name)
    r = capi.solve(p, method=1, pdlp_solver_mode=4, amd_halpern_resident=1)
    assert r["return_code"] == 0 and r["status"] == "Optimal" and abs(r["objective"] - ref) <= 2e-4 * (1.0 + abs(ref))
    assert r["solve_info"]["pdlp_algorithm"] == "reflected_halpern" and r["solve_info"]["halpern_resident"] == 1 and r["solve_info"]["engine"] == "pdlp"
    assert 0.5 * its - 80 <= r["steps_taken"] <= 2.0 * its + 80 and r["returned_average"] == 0
    c = capi.solve(p, pdlp_solver_mode=4, amd_halpern_resident=1)  # the default method: Concurrent
    assert c["return_code"] == 0 and c["status"] == "Optimal" and abs(c["objective"] - ref) <= 2e-4 * (1.0 + abs(ref))
    assert c["solve_info"]["pdlp_algorithm"] == "reflected_halpern" and c["solve_info"]["halpern_resident"] == 1
    os.environ["CUOPT_AMD_DUAL_SIMPLEX"] = "0"  # ... and PDLP alone behind the same request
    try:
        e = capi.solve(p, pdlp_solver_mode=4, amd_halpern_resident=1)
    finally:
        del os.environ["CUOPT_AMD_DUAL_SIMPLEX"]
    assert e["status"] == "Optimal" and e["solve_info"]["engine"] == "pdlp" and abs(e["objective"] - ref) <= 2e-4 * (1.0 + abs(ref))
    assert e["solve_info"]["halpern_resident"] == 1
    for method in (lp.SolverMethod.PDLP, lp.SolverMethod.Concurrent):
        settings = lp.SolverSettings()
        settings.set_parameter(lp.CUOPT_METHOD, method)
        settings.set_parameter(lp.CUOPT_PDLP_SOLVER_MODE, lp.PDLPSolverMode.Halpern1)
        settings.set_parameter(lp.CUOPT_AMD_HALPERN_RESIDENT, 1)
        assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_RESIDENT) == 1
        dm = lp.DataModel()
        dm.set_csr_constraint_matrix(p["values"], p["indices"], p["offsets"])
        dm.set_objective_coefficients(p["c"])
        dm.set_constraint_lower_bounds(p["lo"])
        dm.set_constraint_upper_bounds(p["hi"])
        dm.set_variable_lower_bounds(p["lb"])
        dm.set_variable_upper_bounds(p["ub"])
        dm.set_maximize(p.get("maximize", False))
        dm.set_objective_offset(p.get("objective_offset", 0.0))
        sol = lp.Solve(dm, settings)
        assert sol.get_termination_reason() == "Optimal" and abs(sol.get_primal_objective() - ref) <= 2e-4 * (1.0 + abs(ref))
        if method == lp.SolverMethod.PDLP:  # the same solver as capi.Solver(mode=4, halpern_resident=1): the same count
            assert sol.get_lp_stats()["nb_iterations"] == r["steps_taken"]
            assert sol.get_pdlp_warm_start_data() is None
    assert lp.SolverSettings().get_parameter(lp.CUOPT_AMD_HALPERN_RESIDENT) == 0
    off = capi.solve(p, method=1, pdlp_solver_mode=4)  # without the parameter: what ran is the multi-launch path
    assert off["status"] == "Optimal" and off["solve_info"]["halpern_resident"] == 0
    avg = capi.solve(p, method=1, amd_halpern_resident=1)  # ignored by the averaging modes
    assert avg["status"] == "Optimal" and avg["solve_info"]["halpern_resident"] == 0 and avg["solve_info"]["pdlp_algorithm"] == "pdhg_average"


# ---- 9. batches ----------------------------------------------------------------------------------------------------------------------
def test_batches(monkeypatch):
    variants = [v50_with_tighter_bounds(f) for f in (0.008, 0.006, 0.005, 0.004)]
    solvers = [resident_solver(q, monkeypatch) for q in variants]
    with pytest.raises(capi.CuOptError) as e:
        capi.SharedMatrixBatch(solvers)
    assert e.value.code == -7 and "Halpern" in str(e.value)
    ctx = (C.c_void_p * 4)(*[s.device.handle for s in solvers])
    out = C.c_void_p()
    rc = capi.lib.pdlpdev_small_batch_create(C.byref(out), ctx, 4)
    assert rc == -7 and "Halpern" in capi.lib.pdlpdev_last_error().decode() and not out.value
    singles = [(s.advance(),) + s.solution() for s in solvers]  # the solvers stay usable
    for s in solvers:
        s.close()
    assert [r[0]["status_name"] for r in singles] == ["Optimal"] * 4
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    res = capi.batch_solve(variants, mode=4, halpern_resident=1)
    assert [r["status_name"] for r in res] == ["Optimal"] * 4
    for r, one in zip(res, singles):
        for k in ("steps_taken", "num_restarts", "num_major_iterations", "primal_objective", "dual_objective"):
            assert r[k] == one[0][k], k
        np.testing.assert_array_equal(r["x"], one[1])
        np.testing.assert_array_equal(r["y"], one[2])


# ---- 10. speed -------------------------------------------------------------------------------------------------------------------
def test_resident_halpern_loop_is_faster_per_step(monkeypatch):
    """test_resident_loop_is_faster_per_iteration's measurement and bar (2.0x) for mode 4 on 50v-10: the setting against the
    multi-launch path, which is the code the mode ran before the setting existed"""
    p = lp_only(golden(V50))
    rate = {}
    for resident in (True, False):
        s = capi.Solver(p, mode=4, tol=0.0, halpern_resident=int(resident))
        assert s.device.layout()["resident"] == resident
        s.advance(400)
        t0 = time.perf_counter()
        s.advance(4000)
        s.device.call("synchronize")
        rate[resident] = 4000 / (time.perf_counter() - t0)
        s.close()
    s = capi.Solver(p, mode=1, tol=0.0)  # (next to them: the averaging iteration's resident loop; no bar on that ratio)
    assert s.device.layout()["resident"]
    s.advance(400)
    t0 = time.perf_counter()
    s.advance(4000)
    s.device.call("synchronize")
    averaging = 4000 / (time.perf_counter() - t0)
    s.close()
    print("steps/s: mode 4 resident %.0f, mode 4 multi-launch %.0f (%.2fx), Stable2 resident %.0f" % (rate[True], rate[False], rate[True] / rate[False], averaging))
    assert rate[True] > 2.0 * rate[False]
