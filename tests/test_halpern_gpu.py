"""GPU: the restarted reflected-Halpern mode (solver mode 4) against its numpy restatement (tests/halpern_reference.py) -- the fused
kernels of a step in every SpMV layout, the step size, the restart decisions, whole solves through the three interfaces, and the
plumbing around them (graph replay, the fused period path, reset, refusals).  The resident small-LP path is never taken by the mode.

Every case runs under each of the four SpMV layouts.  A forced layout takes every LP of this file (the 14 goldens down to their
one-row members, the synthetic LPs, the mixed-bound 40 x 60 LPs, the dense-segment LP, C3), so each case ASSERTS that both sides
got the layout it asked for; a creation that fails under a forced layout is a failure of the test."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import halpern_reference as H
from conftest import decode_problem, set_tune
from cuopt_amd import capi, synthetic
from cuopt_amd import linear_programming as lp
from oracle import orcbind
from test_halpern_reference import RAW, SYNTHETIC, known_objective, synthetic_lp
from test_random_lps_gpu import highs, random_lp

pytestmark = pytest.mark.gpu
LAYOUTS = ("stream", "panel", "jag", "pb")
AFIRO, V50, COD = "afiro", "mip-50v-10-free-bound-relaxation", "mip-cod105_max-relaxation"


def golden(name):
    return decode_problem(RAW[name])


@functools.lru_cache(maxsize=None)
def restatement(name, eps=1e-4):
    p = golden(name) if name in RAW else synthetic_lp(name)
    r = H.solve(p, eps=eps, max_iterations=200000)
    return r["status"], r["iterations"], r["objective"]


def halpern_device(p, layout, monkeypatch):
    """a context in Halpern mode, in `layout` on both sides, right before its first step, and the restatement fed with ITS scaled
    problem, step size and weight"""
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    if p.get("maximize"):  # (the device layer takes the min-form objective, as the host driver hands it over)
        p = dict(p, c=-np.asarray(p["c"], float), maximize=False)
    capi.lib.pdlpdev_create_no_resident(1)
    try:
        dev = capi.Device(p)
    finally:
        capi.lib.pdlpdev_create_no_resident(0)
    assert_layout(dev, layout)
    dev.call("scaling_compute", 1, 10, 1, 1.0)
    dev.call("scale_problem")
    dev.set_halpern(True)
    sigma, products = dev.spectral_norm()
    B, vec = scaled_problem_of(dev, p)
    eta = H.STEP_SAFETY / sigma
    nr = dev.init_norms()
    omega = np.sqrt(nr[1]) / np.sqrt(nr[2]) if nr[1] > 0 and nr[2] > 0 else 1.0
    dev.call("set_step", eta, omega)
    dev.call("project_primal")
    dev.call("compute_aty")
    dev.halpern_restart(-1.0)
    it = H.HalpernIteration(B, vec["C"], vec["LB"], vec["UB"], vec["LO"], vec["HI"], eta, omega)
    return dev, it, sigma, products


def assert_layout(dev, layout):
    lay = dev.layout()
    assert not lay["resident"] and lay["A"]["layout"] == layout and lay["At"]["layout"] == layout, lay


def scaled_problem_of(dev, p):
    m, n = int(p["m"]), int(p["n"])
    vals = dev.download("A_VALUES", len(p["values"]))
    B = sp.csr_matrix((vals, np.asarray(p["indices"]), np.asarray(p["offsets"])), shape=(m, n))
    vec = {k: dev.download(k, n if k in ("C", "LB", "UB", "DCOL") else m) for k in ("C", "LB", "UB", "LO", "HI", "DROW", "DCOL")}
    return B, vec


def close_to(got, ref, rtol):
    """rtol relative to the vector's infinity norm"""
    scale = float(np.max(np.abs(ref))) if len(ref) else 0.0
    err = float(np.max(np.abs(got - ref))) if len(ref) else 0.0
    return err <= rtol * scale, err / scale if scale > 0 else err


@functools.lru_cache(maxsize=None)
def dense_rows_lp():
    """two rows with runs of thousands of consecutive columns: dense row segments (tests/test_dense_segments_gpu.py's LP)"""
    p = synthetic.generate_structured("dense_rows", m=70000, n=70000, k=8, seed=11)
    p.setdefault("lb", np.zeros(p["n"]))
    p.setdefault("ub", np.full(p["n"], np.inf))
    return p


STEP_LPS = {"afiro": lambda: golden(AFIRO), "50v-10": lambda: golden(V50), "cod105": lambda: golden(COD),
            "mixed-40x60": lambda: random_lp(3)[0], "synthetic-2000x3000": lambda: synthetic_lp("synthetic-2000x3000-seed1"),
            "dense-rows-70000": dense_rows_lp}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(STEP_LPS))
def test_step_parity(name, layout, monkeypatch):
    """120 steps without restarts: x, y, A^T y after steps 1, 2, 40, 120 at 1e-10 of the vector's infinity norm, T(z^k) of the last
    step likewise, r_k at rtol 1e-9, and r_k^2 >= 0 on every step (the device keeps the minimum)"""
    p = STEP_LPS[name]()
    dense = name.startswith("dense")
    if dense:  # (1.4 % of the nonzeros: under the 2 % from which the dense path switches itself on)
        set_tune(monkeypatch, dense="1")
    dev, it, _, _ = halpern_device(p, layout, monkeypatch)
    assert dev.dense_info()["on"] == dense
    done = 0
    for target in (1, 2, 40, 120):
        ctl = dev.run(target)
        assert ctl.steps_taken == target and ctl.attempts == target and ctl.error == 0
        while done < target:
            it.step()
            done += 1
        for buf, ref in (("X", it.x), ("Y", it.y), ("ATY", it.aty), ("AVG_X", it.tx), ("AVG_Y", it.ty)):
            ok, err = close_to(dev.download(buf, len(ref)), ref, 1e-10)
            print(name, layout, target, buf, "rel err %.3e" % err)
            assert ok, (name, layout, target, buf, err)
        h = dev.halpern()
        print(name, layout, target, "r", h["r"], it.r)
        assert h["k"] == target and h["r"] == pytest.approx(it.r, rel=1e-9)
        assert h["r_first"] == pytest.approx(it.r_first, rel=1e-9) and h["r_first"] > 0 and h["r2_min"] >= 0.0
    dev.close()


SVD = {}  # name -> sigma_max of the scaled matrix by a dense SVD (the scaling does not depend on the layout: checked below)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(RAW) + ["synthetic-2000x3000-seed1"])
def test_step_size_against_a_dense_svd(name, layout, monkeypatch):
    """0.9979 <= eta sigma_max < 1: the power iteration (the layout's own plain products) approaches sigma_max from below and
    stops at a relative move of 1e-6"""
    p = golden(name) if name in RAW else synthetic_lp(name)
    dev, it, sigma, products = halpern_device(p, layout, monkeypatch)
    if name not in SVD:
        SVD[name] = (it.B.data.copy(), np.linalg.svd(it.B.toarray(), compute_uv=False)[0])
    np.testing.assert_array_equal(it.B.data, SVD[name][0])
    exact = SVD[name][1]
    print(name, "eta sigma_max = %.6f after %d products" % (H.STEP_SAFETY / sigma * exact, products))
    assert 1 <= products <= 5000
    assert 0.9979 <= H.STEP_SAFETY / sigma * exact < 1.0
    assert dev.spectral_norm() == (sigma, products)  # deterministic
    dev.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", [AFIRO, V50, "synthetic-2000x3000-seed1"])
def test_restart_decisions_follow_the_restatement(name, layout, monkeypatch):
    """the first 10 major iterations: the same restart flags, and the primal weight after each restart at rtol 1e-9"""
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    p = golden(name) if name in RAW else synthetic_lp(name)
    s = capi.Solver(p, mode=4, tol=1e-13)
    dev = s.device
    assert_layout(dev, layout)
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
    print(name, flags, weights)
    assert flags == ref["flags"] and len(flags) == 10
    np.testing.assert_allclose(weights, ref["weights"], rtol=1e-9)
    s.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_solves_through_the_host_driver(layout, monkeypatch):
    """all 14 goldens and the three synthetic LPs: Optimal, the known objective, iterations in the band around the restatement's"""
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    ran = 0
    for name in sorted(RAW) + sorted(SYNTHETIC):
        p = golden(name) if name in RAW else synthetic_lp(name)
        ref = known_objective(name) if name in RAW else p["objective_star"]
        s = capi.Solver(p, mode=4)
        assert_layout(s.device, layout)
        r = s.advance()
        x, y, _ = s.solution()
        status, its, _ = restatement(name)
        print(name, layout, r["status_name"], r["steps_taken"], "restatement", its, "objective", r["primal_objective"], ref)
        assert r["status_name"] == "Optimal" == status
        assert abs(r["primal_objective"] - ref) <= 2e-4 * (1.0 + abs(ref))
        assert 0.5 * its - 80 <= r["steps_taken"] <= 2.0 * its + 80
        assert r["returned_average"] == 0 and r["attempted_steps"] == r["steps_taken"] and r["step_size"] == r["initial_step_size"]
        cx = np.asarray(p["c"], float) * x  # (the objective re-computed on the host from the returned point, summed in another order)
        assert abs(float(cx.sum()) + p.get("objective_offset", 0.0) - r["primal_objective"]) <= 1e-9 * (1.0 + float(np.abs(cx).sum()))
        s.close()
        ran += 1
    assert ran == 17


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", [AFIRO, V50])
def test_solves_through_cuoptsolve_and_the_python_mirror(name, layout, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)  # (test_solves_through_the_host_driver asserts that these LPs get it)
    p = {k: v for k, v in golden(name).items() if k != "var_types"}  # (the LP relaxation of a golden that is a MIP)
    ref = known_objective(name)
    _, its, _ = restatement(name)
    r = capi.solve(p, method=1, pdlp_solver_mode=4)
    assert r["return_code"] == 0 and r["status"] == "Optimal" and abs(r["objective"] - ref) <= 2e-4 * (1.0 + abs(ref))
    assert r["solve_info"]["pdlp_algorithm"] == "reflected_halpern" and r["solve_info"]["engine"] == "pdlp"
    assert 0.5 * its - 80 <= r["steps_taken"] <= 2.0 * its + 80 and r["returned_average"] == 0
    c = capi.solve(p, pdlp_solver_mode=4)  # the default method: Concurrent (the dual simplex races, the emulation aims at 1e-8)
    assert c["return_code"] == 0 and c["status"] == "Optimal" and abs(c["objective"] - ref) <= 2e-4 * (1.0 + abs(ref))
    assert c["solve_info"]["pdlp_algorithm"] == "reflected_halpern"
    os.environ["CUOPT_AMD_DUAL_SIMPLEX"] = "0"  # ... and PDLP alone behind the same request: the emulation under mode 4
    try:
        e = capi.solve(p, pdlp_solver_mode=4)
    finally:
        del os.environ["CUOPT_AMD_DUAL_SIMPLEX"]
    assert e["status"] == "Optimal" and e["solve_info"]["engine"] == "pdlp" and abs(e["objective"] - ref) <= 2e-4 * (1.0 + abs(ref))
    settings = lp.SolverSettings()
    settings.set_parameter(lp.CUOPT_METHOD, lp.SolverMethod.PDLP)
    settings.set_parameter(lp.CUOPT_PDLP_SOLVER_MODE, lp.PDLPSolverMode.Halpern1)
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
    assert 0.5 * its - 80 <= sol.get_lp_stats()["nb_iterations"] <= 2.0 * its + 80
    assert sol.get_pdlp_warm_start_data() is None


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("seed", range(12))
def test_mixed_bound_lps_at_1e_8_against_highs(seed, layout, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    p, A = random_lp(seed)
    ref = highs(p, A)
    s = capi.Solver(p, mode=4)  # (the layout this LP gets under the setting)
    assert_layout(s.device, layout)
    s.close()
    r = capi.solve(p, method=1, pdlp_solver_mode=4, tol=1e-8, iteration_limit=200000)
    print(seed, r["status"], r["steps_taken"], abs(r["objective"] - ref))
    assert r["status"] == "Optimal" and r["solve_info"]["pdlp_algorithm"] == "reflected_halpern"
    assert abs(r["objective"] - ref) <= 2e-6 * (1.0 + abs(ref))


@functools.lru_cache(maxsize=None)
def c3_lp():
    return synthetic.generate(**synthetic.CONFIGS["c3"])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_c3_solve_and_host_verification(layout, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    p = c3_lp()
    r = capi.solve(p, method=1, pdlp_solver_mode=4, tol=1e-4, iteration_limit=20000)
    print("c3", r["status"], r["steps_taken"], r["num_restarts"], r["solve_time"])
    assert r["status"] == "Optimal"
    known = p["objective_star"]
    assert abs(r["objective"] - known) <= 2e-4 * (1.0 + abs(known))
    A = sp.csr_matrix((p["values"], p["indices"], p["offsets"]), shape=(p["m"], p["n"]))
    x, y = r["x"], r["y"]
    assert float(p["c"] @ x) == pytest.approx(r["primal_objective"], rel=1e-9)
    ax = A @ x
    viol = np.maximum(np.maximum(p["lo"] - ax, ax - p["hi"]), 0.0)
    bcomb = np.maximum(np.where(np.isfinite(p["lo"]), np.abs(p["lo"]), 0), np.where(np.isfinite(p["hi"]), np.abs(p["hi"]), 0))
    assert np.linalg.norm(viol) == pytest.approx(r["l2_primal_residual"], rel=1e-6, abs=1e-9)
    assert np.linalg.norm(viol) <= 1e-4 + 1e-4 * np.linalg.norm(bcomb)
    assert np.all(x >= p["lb"]) and np.all(x <= p["ub"])
    g = p["c"] - A.T @ y
    bv = np.where(g > 0, p["lb"], p["ub"])
    rc = np.where((g == 0) | np.isfinite(bv), g, 0.0)
    assert np.linalg.norm(g - rc) <= 1e-4 + 1e-4 * np.linalg.norm(p["c"])
    assert r["gap"] <= 1e-4 + 1e-4 * (abs(r["primal_objective"]) + abs(r["dual_objective"]))


def same_solve(a, b):
    for k in ("status", "steps_taken", "num_restarts", "num_major_iterations", "primal_objective", "dual_objective", "primal_weight", "step_size"):
        assert a[0][k] == b[0][k], k
    for u, v in zip(a[1:4], b[1:4]):
        np.testing.assert_array_equal(u, v)


def solved(p, layout=None, **kw):
    s = capi.Solver(p, mode=4, **kw)
    if layout:
        assert_layout(s.device, layout)
    r = s.advance()
    x, y, z = s.solution()
    stats = s.device.loop_stats()
    s.close()
    return r, x, y, z, stats


@pytest.mark.parametrize("layout", LAYOUTS)
def test_graph_replay_period_path_and_reset_are_bit_identical(layout, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    for p in (golden(AFIRO), synthetic_lp("synthetic-2000x3000-seed1")):
        base = solved(p, layout)
        assert base[0]["status_name"] == "Optimal"
        same_solve(base, solved(p, layout, use_graph=0))
        set_tune(monkeypatch, period_path="0")
        apart = solved(p, layout)
        set_tune(monkeypatch, period_path=None)
        same_solve(base, apart)
        # synchronisations inside the loop: the anchor of the start, one per restart, and per period ONE where pdlpdev_run_period
        # evaluates behind the steps (the panel layout's guarded evaluation kernels) -- two (steps, then evaluation) everywhere else
        # and with period_path=0.  This is what shows that the two runs compared above took the two different paths.
        majors, restarts = base[0]["num_major_iterations"], base[0]["num_restarts"]
        fused = layout == "panel"
        print(layout, "loop syncs", base[4]["loop_syncs"], apart[4]["loop_syncs"], "periods", majors, "restarts", restarts)
        assert base[4]["loop_syncs"] == 1 + restarts + (1 if fused else 2) * majors
        assert apart[4]["loop_syncs"] == 1 + restarts + 2 * majors
        s = capi.Solver(p, mode=4)
        first = (s.advance(),) + s.solution()
        s.reset()
        again = (s.advance(),) + s.solution()
        s.close()
        same_solve(base, first)
        same_solve(base, again)


def test_refusals_name_the_mode():
    p = golden(AFIRO)
    for kw in (dict(detect_infeasibility=1), dict(save_best_primal_so_far=1), dict(first_primal_feasible=1)):
        with pytest.raises(capi.CuOptError) as e:
            capi.Solver(p, mode=4, **kw)
        assert e.value.code == -7 and "Halpern" in str(e.value) and list(kw)[0] in str(e.value)
    with pytest.raises(capi.CuOptError) as e:
        capi.Solver(p, mode=4, rank=0, world=2, comm_id=capi.softcomm_id(2))
    assert e.value.code == -7 and "Halpern" in str(e.value)
    r = capi.solve(p, method=1, pdlp_solver_mode=4, amd_num_gpus=2)  # cuoptamd_solve_sharded
    assert r["return_code"] == capi.CUOPT_VALIDATION_ERROR and "Halpern" in r["error_string"]
    r = capi.solve(p, method=1, pdlp_solver_mode=4, infeasibility_detection=True)
    assert r["return_code"] == capi.CUOPT_VALIDATION_ERROR and "Halpern" in r["error_string"]
    for kw in (dict(initial_k=3), dict(strict_infeasibility=1), dict(unbounded_from_feasible_iterates=1)):
        with pytest.raises(capi.CuOptError) as e:  # settings of the averaging iteration: refused by name, not ignored
            capi.Solver(p, mode=4, **kw)
        assert e.value.code == -7 and "Halpern" in str(e.value) and list(kw)[0] in str(e.value)
    h = capi.hyper_preset(4)
    h.update_step_size_on_initial_solution = 1
    with pytest.raises(capi.CuOptError) as e:
        capi.Solver(p, hyper=h)
    assert e.value.code == -7 and "update_step_size_on_initial_solution" in str(e.value)
    s = capi.Solver(p, mode=4)
    for kw in (dict(detect_infeasibility=1), dict(save_best_primal_so_far=1), dict(first_primal_feasible=1), dict(initial_k=3)):
        with pytest.raises(capi.CuOptError) as e:  # a refused reset leaves the solver as it was
            s.reset(**kw)
        assert e.value.code == -7 and "Halpern" in str(e.value) and list(kw)[0] in str(e.value)
    first = s.advance()
    assert first["status_name"] == "Optimal" and first["steps_taken"] == restatement(AFIRO)[1]
    with pytest.raises(capi.CuOptError) as e:
        s.get_warm_start()
    assert e.value.code == -7 and "Halpern" in str(e.value)
    s.close()
    snap = capi.Solver(p, mode=1)
    snap.advance()
    ws = snap.get_warm_start()
    snap.close()
    with pytest.raises(capi.CuOptError) as e:
        capi.Solver(p, mode=4, warm_start=ws)
    assert e.value.code == -7 and "Halpern" in str(e.value)


def test_batches_run_halpern_solvers_one_after_the_other():
    p = synthetic_lp("synthetic-2000x3000-seed1")
    parent = capi.Solver(p, mode=4)
    clones = [parent.clone(ub=np.full(p["n"], 50.0 + i)) for i in range(3)]
    with pytest.raises(capi.CuOptError) as e:
        capi.SharedMatrixBatch([parent] + clones)
    assert e.value.code == -7 and "Halpern" in str(e.value)
    alone = parent.advance()
    assert alone["status_name"] == "Optimal" and clones[0].advance()["status_name"] == "Optimal"
    for c in clones:
        c.close()
    parent.close()
    lps = []
    for i in range(4):
        q = dict(p)
        q["ub"] = np.full(p["n"], 50.0 + i)
        lps.append(q)
    out = capi.batch_solve(lps, mode=4)
    assert [r["status_name"] for r in out] == ["Optimal"] * 4
    one = solved(lps[2])
    assert out[2]["steps_taken"] == one[0]["steps_taken"]
    np.testing.assert_array_equal(out[2]["x"], one[1])


def test_presets_of_the_reference_are_unchanged():
    fields = [f for f, _ in capi.Hyper._fields_]
    old = fields[:fields.index("algorithm")]
    assert len(old) == orcbind.H["ORC_H_COUNT"] and fields[len(old):] == ["algorithm", "halpern_power_max_products", "halpern_step_safety", "halpern_power_tolerance"]
    for mode in range(4):
        h, o = capi.hyper_preset(mode), orcbind.hyper_preset(mode)
        assert [float(getattr(h, f)) for f in old] == [float(v) for v in o]
        assert h.algorithm == 0
    h, base = capi.hyper_preset(4), capi.hyper_preset(1)
    changed = {f for f in fields if getattr(h, f) != getattr(base, f)}
    assert changed == {"algorithm", "min_iteration_restart", "primal_weight_update_smoothing"}
    assert (h.algorithm, h.major_iteration, h.halpern_step_safety, h.primal_weight_update_smoothing) == (1, 40, 0.998, 0.99)


def test_timing_hook_brackets_the_halpern_kernels(monkeypatch):
    made = halpern_device(synthetic_lp("synthetic-2000x3000-seed1"), "stream", monkeypatch)
    dev, it, _, _ = made
    dev.run(3)
    before = (dev.download("X", it.x.size), dev.halpern(), dev.download("AVG_X", it.x.size), dev.download("AVG_Y", it.y.size))
    for k in ("PRIMAL", "SPMV_A_DUAL", "SPMV_AT_STEP", "STEP_DECISION"):
        assert dev.time_kernel(k, reps=3) > 0.0
    dev.ctl()
    after = (dev.download("X", it.x.size), dev.halpern(), dev.download("AVG_X", it.x.size), dev.download("AVG_Y", it.y.size))
    assert before[1] == after[1]
    for u, v in zip(before[::2] + before[3:], after[::2] + after[3:]):  # the iterate and T(z^k) of the last real step
        np.testing.assert_array_equal(u, v)
    dev.run(4)  # state was put back: the fourth step is the restatement's
    for _ in range(4):
        it.step()
    assert close_to(dev.download("Y", it.y.size), it.y, 1e-10)[0]
    dev.close()
