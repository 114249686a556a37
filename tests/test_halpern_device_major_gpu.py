"""GPU: verdict and restart of a reflected-Halpern major iteration on the device, P periods per host synchronisation
(cuoptamd_settings::halpern_device_major, "amd_halpern_device_major" behind cuOptSolve).

The reference of every comparison is the host-decided path of the same solver with the option at 0; for the decisions also a float64
restatement of halpern_major_head's tests (below) and the numpy restatement of the mode (tests/halpern_reference.py)."""
import functools
import math

import numpy as np
import pytest

import halpern_reference as H
from cuopt_amd import capi, synthetic
from test_halpern_gpu import AFIRO, COD, V50, golden, scaled_problem_of
from test_halpern_resident_gpu import NEOS5, SUDOKU, FOUR, v50_with_tighter_bounds
from test_random_lps_gpu import highs, random_lp

pytestmark = pytest.mark.gpu
EV = dict(CX=0, DUAL_SUM=1, PRES2=2, DRES2=3, X2=4, Y2=5, LINF_P=6, LINF_D=7)  # PDLPDEV_EV_*
FIGURES = ("primal_objective", "dual_objective", "gap", "relative_gap", "l2_primal_residual", "l2_dual_residual",
           "l2_relative_primal_residual", "l2_relative_dual_residual")
COUNTS = ("status", "steps_taken", "num_restarts", "num_major_iterations", "step_size", "primal_weight")
BUFFERS = ("X", "Y", "ATY", "AVG_X", "AVG_Y")


def bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def ulp_up(v):
    return float(np.nextafter(v, np.inf))


# ---- 1. the decision kernel alone ----------------------------------------------------------------------------------------------------
def params(**kw):
    p = capi.HalpernMajorParams()
    base = dict(absolute_gap_tolerance=1e-4, relative_gap_tolerance=1e-4, absolute_primal_tolerance=1e-4, relative_primal_tolerance=1e-4,
                absolute_dual_tolerance=1e-4, relative_dual_tolerance=1e-4, norm_b=3.0, norm_c=7.0, objective_scale=1.0, objective_offset=0.0,
                sufficient_reduction=0.2, necessary_reduction=0.8, artificial_threshold=0.36, per_constraint_residual=0, want_linf=1,
                iteration_limit=2 ** 31 - 1, iteration_offset=0)
    base.update(kw)
    for k, v in base.items():
        setattr(p, k, v)
    return p


def head(ev, steps, error, r, r_first, k, r_prev, P, target, stopped):
    """halpern_major_head's tests in float64 (pdlp_solver.cpp: to_convergence, verdict, check_limits' iteration limit, the three
    restart tests), as the decision has to make them -> (verdict, restart, r_prev afterwards, stopped afterwards); None: nothing moves"""
    if stopped:
        return None
    if error or steps < target:
        return (capi.MAJOR_STEP_ERROR if error else capi.MAJOR_FELL_SHORT), 0, r_prev, 1
    pobj, dobj = np.float64(ev[EV["CX"]]), np.float64(ev[EV["DUAL_SUM"]])
    if P.objective_scale != 1.0 or P.objective_offset != 0.0:
        pobj = np.float64(P.objective_scale) * pobj + np.float64(P.objective_offset)
        dobj = np.float64(P.objective_scale) * dobj + np.float64(P.objective_offset)
    with np.errstate(all="ignore"):
        gap, abs_obj = np.abs(pobj - dobj), np.abs(pobj) + np.abs(dobj)
        gap_ok = gap <= np.float64(P.absolute_gap_tolerance) + np.float64(P.relative_gap_tolerance) * abs_obj
        if P.per_constraint_residual:
            primal_ok = np.float64(ev[EV["LINF_P"]]) <= P.absolute_primal_tolerance
            dual_ok = np.float64(ev[EV["LINF_D"]]) <= P.absolute_dual_tolerance
        else:
            primal_ok = np.sqrt(np.float64(ev[EV["PRES2"]])) <= np.float64(P.absolute_primal_tolerance) + np.float64(P.relative_primal_tolerance) * np.float64(P.norm_b)
            dual_ok = np.sqrt(np.float64(ev[EV["DRES2"]])) <= np.float64(P.absolute_dual_tolerance) + np.float64(P.relative_dual_tolerance) * np.float64(P.norm_c)
    total = P.iteration_offset + steps
    if total > 1 and gap_ok and primal_ok and dual_ok:
        return capi.MAJOR_OPTIMAL, 0, r_prev, 1
    if steps >= P.iteration_limit:
        return capi.MAJOR_ITERATION_LIMIT, 0, r_prev, 1
    r, r_first = np.float64(r), np.float64(r_first)
    restart = bool(r <= np.float64(P.sufficient_reduction) * r_first) or \
        bool(r <= np.float64(P.necessary_reduction) * r_first and r_prev >= 0.0 and r > r_prev) or \
        bool(np.float64(k) >= np.float64(P.artificial_threshold) * np.float64(total))
    return capi.MAJOR_GO_ON, int(restart), (-1.0 if restart else float(r)), 0


FAR = [5.0, 1.0, 4.0, 9.0, 2.0, 2.0, 0.5, 0.5]  # an evaluation far from optimal: cx 5, dual 1, residuals 2 and 3


def decision_cases():
    """(label, ev, steps, error, r, r_first, k, r_prev, params, target, stopped)"""
    out = []
    r_first = 0.7
    suff = float(np.float64(0.2) * np.float64(r_first))
    for label, r in (("sufficient-at", suff), ("sufficient-ulp-above", ulp_up(suff))):
        out.append((label, FAR, 4000, 0, r, r_first, 1, -1.0, params(), 4000, 0))
    r_mid = 0.5  # inside the necessary band: 0.14 < 0.5 <= 0.56
    for label, prev in (("necessary-no-previous", -1.0), ("necessary-previous-below", 0.4), ("necessary-previous-equal", 0.5), ("necessary-previous-above", 0.6)):
        out.append((label, FAR, 4000, 0, r_mid, r_first, 1, prev, params(), 4000, 0))
    for total in (40, 100, 4000):
        edge = float(np.float64(0.36) * np.float64(total))
        for label, k in (("at", math.ceil(edge)), ("below", math.ceil(edge) - 1), ("above", math.ceil(edge) + 1)):
            out.append(("artificial-%s-%d" % (label, total), FAR, total, 0, 0.69, r_first, k, -1.0, params(), total, 0))
    # the termination rule's bounds: the gap exactly at its bound, each residual's root exactly at its bound and one ulp above
    P = params()
    opt = [1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0]
    pb = float(np.float64(1e-4) + np.float64(1e-4) * np.float64(P.norm_b))
    db = float(np.float64(1e-4) + np.float64(1e-4) * np.float64(P.norm_c))

    def square_with_root(b, above):
        """a float whose correctly rounded root is exactly b (or the float behind b)"""
        want = ulp_up(b) if above else b
        s = float(np.float64(want) * np.float64(want))
        for _ in range(8):
            root = float(np.sqrt(np.float64(s)))
            if root == want:
                return s
            s = ulp_up(s) if root < want else float(np.nextafter(s, -np.inf))
        raise AssertionError("no square with that root")

    for label, ev in (("optimal", opt),
                      ("primal-at", [1.0, 1.0, square_with_root(pb, False), 0.0, 1.0, 1.0, 0.0, 0.0]),
                      ("primal-ulp-above", [1.0, 1.0, square_with_root(pb, True), 0.0, 1.0, 1.0, 0.0, 0.0]),
                      ("dual-at", [1.0, 1.0, 0.0, square_with_root(db, False), 1.0, 1.0, 0.0, 0.0]),
                      ("dual-ulp-above", [1.0, 1.0, 0.0, square_with_root(db, True), 1.0, 1.0, 0.0, 0.0])):
        out.append((label, ev, 80, 0, 0.69, r_first, 3, -1.0, params(), 80, 0))
    # the gap |p - d| against abs + rel (|p| + |d|) with d = 1: the largest p that still holds the bound (found by bisection on the
    # floats, with the restatement's own expression) and the float behind it
    lo, hi = 1.0, 1.0 + 4e-4  # (the bound is about 3.0003e-4)
    while ulp_up(lo) < hi:
        mid = float(np.float64(lo) + (np.float64(hi) - np.float64(lo)) / 2)
        ok = np.abs(np.float64(mid) - 1.0) <= np.float64(1e-4) + np.float64(1e-4) * (np.abs(np.float64(mid)) + 1.0)
        lo, hi = (mid, hi) if ok else (lo, mid)
    for label, p_ in (("gap-at", lo), ("gap-ulp-above", hi)):
        out.append((label, [p_, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0], 80, 0, 0.69, r_first, 3, -1.0, params(), 80, 0))
    zero = dict(absolute_gap_tolerance=0.0, relative_gap_tolerance=0.0, absolute_primal_tolerance=0.0, relative_primal_tolerance=0.0,
                absolute_dual_tolerance=0.0, relative_dual_tolerance=0.0)
    out.append(("tolerances-zero-exact-point", opt, 80, 0, 0.69, r_first, 3, -1.0, params(**zero), 80, 0))
    out.append(("tolerances-zero-far-point", FAR, 80, 0, 0.69, r_first, 3, -1.0, params(**zero), 80, 0))
    out.append(("per-constraint-at", [1.0, 1.0, 9.0, 9.0, 1.0, 1.0, 1e-4, 1e-4], 80, 0, 0.69, r_first, 3, -1.0, params(per_constraint_residual=1), 80, 0))
    out.append(("per-constraint-above", [1.0, 1.0, 0.0, 0.0, 1.0, 1.0, ulp_up(1e-4), 0.0], 80, 0, 0.69, r_first, 3, -1.0, params(per_constraint_residual=1), 80, 0))
    out.append(("iteration-limit-exact", FAR, 120, 0, 0.69, r_first, 3, -1.0, params(iteration_limit=120), 120, 0))
    out.append(("iteration-limit-ahead", FAR, 120, 0, 0.69, r_first, 3, -1.0, params(iteration_limit=121), 120, 0))
    out.append(("optimal-at-the-limit", opt, 120, 0, 0.69, r_first, 3, -1.0, params(iteration_limit=120), 120, 0))
    out.append(("iteration-offset", FAR, 40, 0, 0.69, r_first, 30, -1.0, params(iteration_offset=4000), 40, 0))
    nan = float("nan")
    out.append(("nan-objective", [nan, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0], 80, 0, 0.69, r_first, 3, -1.0, params(), 80, 0))
    out.append(("nan-residual", [1.0, 1.0, nan, 0.0, 1.0, 1.0, 0.0, 0.0], 80, 0, 0.69, r_first, 3, 0.5, params(), 80, 0))
    out.append(("nan-r", FAR, 80, 0, nan, r_first, 3, 0.5, params(), 80, 0))
    out.append(("step-error", opt, 41, 1, 0.69, r_first, 3, 0.5, params(), 80, 0))
    out.append(("fell-short", opt, 79, 0, 0.69, r_first, 3, 0.5, params(), 80, 0))
    out.append(("stopped", opt, 80, 0, 0.1, r_first, 3, 0.5, params(), 80, 1))
    out.append(("stopped-with-the-error-up", FAR, 80, 1, 0.1, r_first, 3, 0.5, params(), 80, 1))
    # objective scale -1 with an offset (a maximisation): both objectives mapped before gap and bound are formed
    out.append(("scale-minus-one-optimal", [2.5, 2.5, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0], 80, 0, 0.69, r_first, 3, -1.0, params(objective_scale=-1.0, objective_offset=10.0), 80, 0))
    out.append(("scale-minus-one-cancels", [10.0, 10.0 + 2e-3, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0], 80, 0, 0.69, r_first, 3, -1.0, params(objective_scale=-1.0, objective_offset=10.0), 80, 0))
    out.append(("offset-only", [1.0, 1.0 + 2e-4, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0], 80, 0, 0.69, r_first, 3, -1.0, params(objective_offset=1e3), 80, 0))
    out.append(("no-linf-request", [1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 7.0, 7.0], 80, 0, 0.69, r_first, 3, -1.0, params(want_linf=0, per_constraint_residual=1), 80, 0))
    return out


CASES = decision_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_decision_kernel_against_the_float64_restatement(case):
    label, ev, steps, error, r, r_first, k, r_prev, P, target, stopped = case
    ctl, hal = capi.Ctl(), capi.Halpern()
    ctl.steps_taken, ctl.attempts, ctl.error, ctl.primal_weight, ctl.step_size, ctl.target_steps = steps, steps, error, 1.75, 0.01, target
    hal.r, hal.r_first, hal.k = r, r_first, k
    before = capi.HalpernMajorRecord()
    before.steps_taken, before.verdict, before.restart, before.r, before.new_weight = -7, 99, 5, 123.0, 4.5  # (what a stopped burst must keep)
    rec, r_prev_out, stopped_out, restart_out = capi.debug_halpern_major_decide(ev, ctl, hal, r_prev, P, target=target, stopped=stopped, record=before)
    ev_seen = list(ev)
    if not P.want_linf:
        ev_seen[EV["LINF_P"]] = ev_seen[EV["LINF_D"]] = 0.0
    want = head(ev_seen, steps, error, r, r_first, k, r_prev, P, target, stopped)
    print(label, "verdict", rec.verdict, "restart", rec.restart, "r_prev", r_prev_out, "stopped", stopped_out, "want", want)
    if want is None:  # the burst has stopped: nothing may change
        assert (rec.steps_taken, rec.verdict, rec.restart, rec.r, rec.new_weight) == (-7, 99, 5, 123.0, 4.5)
        assert bits(r_prev_out) == bits(r_prev) and stopped_out == 1 and restart_out == 0
        return
    verdict, restart, r_prev_want, stopped_want = want
    assert (rec.verdict, rec.restart, stopped_out, restart_out) == (verdict, restart, stopped_want, restart)
    assert bits(r_prev_out) == bits(r_prev_want)
    assert (rec.steps_taken, rec.k) == (steps, k) and bits(rec.r) == bits(r) and bits(rec.r_first) == bits(r_first)
    assert rec.primal_weight == 1.75 and list(rec.dist) == [0.0, 0.0] and rec.new_weight == 0.0
    if verdict in (capi.MAJOR_STEP_ERROR, capi.MAJOR_FELL_SHORT):
        assert list(rec.ev) == [0.0] * 8  # (nothing was evaluated for this record)
    else:
        np.testing.assert_array_equal(bits(list(rec.ev)), bits(ev_seen))


def test_the_cases_hit_every_branch_of_the_restatement():
    """the inputs are only worth something if both sides of every edge are among them (no GPU arithmetic involved: the restatement)"""
    seen = {}
    for label, ev, steps, error, r, r_first, k, r_prev, P, target, stopped in CASES:
        seen[label] = head(ev if P.want_linf else ev[:6] + [0.0, 0.0], steps, error, r, r_first, k, r_prev, P, target, stopped)
    go, opt, lim = capi.MAJOR_GO_ON, capi.MAJOR_OPTIMAL, capi.MAJOR_ITERATION_LIMIT
    assert seen["sufficient-at"][:2] == (go, 1) and seen["sufficient-ulp-above"][:2] == (go, 0)
    assert [seen["necessary-" + s][1] for s in ("no-previous", "previous-below", "previous-equal", "previous-above")] == [0, 1, 0, 0]
    for total in (40, 100, 4000):
        assert [seen["artificial-%s-%d" % (s, total)][1] for s in ("at", "below", "above")] == [1, 0, 1]
    for side in ("primal", "dual", "gap"):
        assert seen[side + "-at"][0] == opt and seen[side + "-ulp-above"][0] == go, side
    assert seen["tolerances-zero-exact-point"][0] == opt and seen["tolerances-zero-far-point"][0] == go
    assert seen["per-constraint-at"][0] == opt and seen["per-constraint-above"][0] == go and seen["no-linf-request"][0] == opt
    assert seen["iteration-limit-exact"][0] == lim and seen["iteration-limit-ahead"][0] == go and seen["optimal-at-the-limit"][0] == opt
    assert seen["iteration-offset"][:2] == (go, 0)  # (k = 30 of 40 steps: above 0.36 * 40, below 0.36 * 4040)
    assert seen["nan-objective"][0] == go and seen["nan-residual"][0] == go and seen["nan-r"][:2] == (go, 0)
    assert seen["step-error"][0] == capi.MAJOR_STEP_ERROR and seen["fell-short"][0] == capi.MAJOR_FELL_SHORT
    assert seen["stopped"] is None and seen["stopped-with-the-error-up"] is None
    assert seen["scale-minus-one-optimal"][0] == opt and seen["scale-minus-one-cancels"][0] == go and seen["offset-only"][0] == opt


# ---- 2. whole solves, bit for bit ------------------------------------------------------------------------------------------------------
def lp_of(name):
    return synthetic.generate(3000, 3000, 6) if name == "synthetic-3000x3000x6" else golden(name)


def solver_for(name, path, monkeypatch, **kw):
    """a mode-4 solver on the resident loop, or on the multi-launch path under a forced layout"""
    if path == "resident":
        monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
        s = capi.Solver(lp_of(name), mode=4, halpern_resident=1, **kw)
        assert s.device.layout()["resident"], s.device.layout()
    else:
        monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", path)
        s = capi.Solver(lp_of(name), mode=4, **kw)
        lay = s.device.layout()
        assert not lay["resident"] and lay["A"]["layout"] == path and lay["At"]["layout"] == path, lay
    return s


def finished(s, read_device=False):
    r = s.advance()
    out = dict(result=r, solution=s.solution(), stats=s.device.loop_stats(), major=s.halpern_device_major())
    if s.halpern_device_major():
        out["burst"] = s.device.halpern_burst_stats()
    if read_device:
        dev = s.device
        size = dict(X=s.n, Y=s.m, ATY=s.n, AVG_X=s.n, AVG_Y=s.m)
        out["buffers"] = {b: dev.download(b, size[b]) for b in BUFFERS}
        c = dev.ctl()
        out["ctl"] = {k: getattr(c, k) for k, _ in capi.Ctl._fields_}
        out["hal"] = dev.halpern()
    s.close()
    return out


REFERENCE = {}


def reference(name, path, tol, monkeypatch):
    """the option-off solve: computed once, shared, never modified"""
    key = (name, path, tol)
    if key not in REFERENCE:
        REFERENCE[key] = finished(solver_for(name, path, monkeypatch, tol=tol, iteration_limit=400000), read_device=True)
    return REFERENCE[key]


def assert_same_solve(got, ref, what):
    for k in COUNTS:
        assert got["result"][k] == ref["result"][k], (what, k, got["result"][k], ref["result"][k])
    for k in FIGURES:
        assert bits(got["result"][k]) == bits(ref["result"][k]), (what, k, got["result"][k], ref["result"][k])
    for u, v, label in zip(got["solution"], ref["solution"], ("x", "y", "reduced costs")):
        assert np.array_equal(bits(u), bits(v)), (what, label, int(np.sum(bits(u) != bits(v))))


PANEL_TOL = {COD: 1e-6, "synthetic-3000x3000x6": 1e-6}


def test_the_references_have_periods_and_restarts_to_speak_of(monkeypatch):
    a = reference(V50, "resident", 1e-4, monkeypatch)["result"]
    b = reference("synthetic-3000x3000x6", "panel", PANEL_TOL["synthetic-3000x3000x6"], monkeypatch)["result"]
    c = reference(COD, "panel", PANEL_TOL[COD], monkeypatch)["result"]
    for label, r in (("50v-10 resident 1e-4", a), ("synthetic panel", b), ("cod105 panel", c)):
        print(label, r["status_name"], "periods", r["num_major_iterations"], "restarts", r["num_restarts"], "steps", r["steps_taken"])
    assert a["status_name"] == "Optimal" and a["num_major_iterations"] >= 10 and a["num_restarts"] >= 3
    assert any(r["status_name"] == "Optimal" and r["num_major_iterations"] >= 10 and r["num_restarts"] >= 3 for r in (b, c))


@pytest.mark.parametrize("P", [1, 3, 16])
@pytest.mark.parametrize("tol", [1e-4, 1e-8])
@pytest.mark.parametrize("name", FOUR)
def test_resident_solves_are_bit_identical_to_the_host_decided_path(name, tol, P, monkeypatch):
    ref = reference(name, "resident", tol, monkeypatch)
    got = finished(solver_for(name, "resident", monkeypatch, tol=tol, iteration_limit=400000, halpern_device_major=P))
    print(name, tol, P, got["result"]["status_name"], got["result"]["steps_taken"], got["result"]["num_restarts"], "syncs", got["stats"]["loop_syncs"],
          ref["stats"]["loop_syncs"], got.get("burst"))
    assert got["major"] == P and ref["major"] == 0 and ref["result"]["status_name"] == "Optimal"
    assert_same_solve(got, ref, (name, tol, P))


@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("name", [COD, "synthetic-3000x3000x6"])
def test_panel_solves_are_bit_identical_to_the_host_decided_path(name, P, monkeypatch):
    tol = PANEL_TOL[name]
    ref = reference(name, "panel", tol, monkeypatch)
    got = finished(solver_for(name, "panel", monkeypatch, tol=tol, iteration_limit=400000, halpern_device_major=P))
    print(name, tol, P, got["result"]["status_name"], got["result"]["steps_taken"], got["result"]["num_restarts"], "syncs", got["stats"]["loop_syncs"],
          ref["stats"]["loop_syncs"], got.get("burst"))
    assert got["major"] == P and ref["major"] == 0
    assert_same_solve(got, ref, (name, tol, P))


# ---- 3. restart decisions against the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FOUR)
def test_restart_decisions_follow_the_restatement(name, monkeypatch):
    """test_halpern_resident_gpu's check with the decisions made on the device (P = 1: advance(40) is one burst of one period)"""
    p = golden(name)
    monkeypatch.delenv("CUOPT_AMD_SPMV_LAYOUT", raising=False)
    s = capi.Solver(p, mode=4, halpern_resident=1, tol=1e-13, halpern_device_major=1)
    assert s.device.layout()["resident"] and s.halpern_device_major() == 1
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
    print(name, flags, weights, r["status_name"], r["steps_taken"], ref["status"], ref["iterations"], dev.halpern_burst_stats())
    assert flags == ref["flags"]
    if name == SUDOKU:
        assert len(flags) == 4 and r["status_name"] == "Optimal" == ref["status"] and r["steps_taken"] == ref["iterations"] == 200
    else:
        assert len(flags) == 10
    np.testing.assert_allclose(weights, ref["weights"], rtol=1e-9)
    assert dev.halpern_burst_stats()["bursts"] == len(flags) + (1 if name == SUDOKU else 0)
    s.close()


# ---- 4. synchronisations ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 4, 16])
@pytest.mark.parametrize("name,path", [(V50, "resident"), (AFIRO, "resident"), ("synthetic-3000x3000x6", "panel")])
def test_one_synchronisation_per_burst(name, path, P, monkeypatch):
    tol = 1e-4 if path == "resident" else PANEL_TOL[name]
    ref = reference(name, path, tol, monkeypatch)
    M, restarts = ref["result"]["num_major_iterations"], ref["result"]["num_restarts"]
    assert ref["result"]["status_name"] == "Optimal"
    assert ref["stats"]["loop_syncs"] == 1 + restarts + M  # the option at 0: the anchor of the start, one per restart, one per period
    got = finished(solver_for(name, path, monkeypatch, tol=tol, iteration_limit=400000, halpern_device_major=P))
    print(name, path, P, "M", M, "restarts", restarts, "syncs", got["stats"]["loop_syncs"], got["burst"])
    assert got["result"]["num_major_iterations"] == M
    assert got["stats"]["loop_syncs"] == 1 + math.ceil(M / P)
    assert got["burst"]["bursts"] == math.ceil(M / P) and got["burst"]["records"] == M
    assert got["burst"]["empty_periods"] == got["burst"]["periods"] - M == math.ceil(M / P) * P - M


# ---- 5. nothing moves behind the stop --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,path", [(AFIRO, "resident"), ("synthetic-3000x3000x6", "panel")])
def test_nothing_moves_behind_the_stop(name, path, monkeypatch):
    tol = 1e-4 if path == "resident" else PANEL_TOL[name]
    one = finished(solver_for(name, path, monkeypatch, tol=tol, halpern_device_major=1), read_device=True)
    many = finished(solver_for(name, path, monkeypatch, tol=tol, halpern_device_major=16), read_device=True)
    off = reference(name, path, tol, monkeypatch)
    M = one["result"]["num_major_iterations"]
    print(name, path, "M", M, one["burst"], many["burst"])
    assert M % 16 != 0 and many["burst"]["empty_periods"] == 16 - M % 16  # (the last period is not the burst's last)
    assert many["burst"]["records"] == M == one["burst"]["records"]  # the ring holds exactly M records
    for other, label in ((many, "P = 16"), (off, "option off")):
        assert_same_solve(other, one, label)
        for b in BUFFERS:
            assert np.array_equal(bits(other["buffers"][b]), bits(one["buffers"][b])), (label, b)
        for k, v in one["ctl"].items():
            assert bits(other["ctl"][k]) == bits(v) if isinstance(v, float) else other["ctl"][k] == v, (label, k, other["ctl"][k], v)
        for k, v in one["hal"].items():
            assert bits(other["hal"][k]) == bits(v) if isinstance(v, float) else other["hal"][k] == v, (label, k, other["hal"][k], v)


# ---- 6. budgets and limits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("step", [100, 80])
def test_budgets_reach_the_same_end(step, P, monkeypatch):
    ref = reference(V50, "resident", 1e-4, monkeypatch)
    s = solver_for(V50, "resident", monkeypatch, tol=1e-4, iteration_limit=400000, halpern_device_major=P)
    r, calls = s.advance(step), 1
    while r["status"] == 0:
        assert r["steps_taken"] == calls * step
        r, calls = s.advance(step), calls + 1
    got = dict(result=r, solution=s.solution())
    print(step, P, calls, s.device.halpern_burst_stats(), s.device.loop_stats())
    assert s.device.halpern_burst_stats()["records"] > 0
    s.close()
    assert_same_solve(got, ref, (step, P))


@pytest.mark.parametrize("P", [1, 4])
def test_the_iteration_limit_ends_where_the_host_ends_it(P, monkeypatch):
    ref = finished(solver_for(V50, "resident", monkeypatch, tol=1e-8, iteration_limit=100))
    got = finished(solver_for(V50, "resident", monkeypatch, tol=1e-8, iteration_limit=100, halpern_device_major=P))
    print(P, got["result"]["status_name"], got["result"]["steps_taken"], got["burst"])
    assert ref["result"]["status_name"] == "IterationLimit" == got["result"]["status_name"] and got["result"]["steps_taken"] == 120
    assert_same_solve(got, ref, P)
    assert got["burst"]["records"] == 3


def test_a_persistent_solver_is_reset_and_solved_again(monkeypatch):
    ub = v50_with_tighter_bounds(0.006)["ub"]
    runs = {}
    for P in (0, 4):
        s = solver_for(V50, "resident", monkeypatch, tol=1e-4, halpern_device_major=P)
        first = dict(result=s.advance(), solution=s.solution())
        s.reset(ub=ub, tol=1e-4, halpern_device_major=P, halpern_resident=1)
        assert s.halpern_device_major() == P
        second = dict(result=s.advance(), solution=s.solution())
        s.reset(tol=1e-4, halpern_device_major=0, halpern_resident=1)  # ... and the option taken off again by a reset
        assert s.halpern_device_major() == 0
        third = dict(result=s.advance(), solution=s.solution())
        s.close()
        runs[P] = (first, second, third)
    assert runs[0][1]["result"]["status_name"] == "Optimal" and runs[0][1]["result"]["steps_taken"] != runs[0][0]["result"]["steps_taken"]
    for a, b, label in zip(runs[4], runs[0], ("first", "other bounds", "option off again")):
        assert_same_solve(a, b, label)
    assert_same_solve(runs[0][2], runs[0][1], "a reset without new bounds keeps them")


def test_a_clone_of_a_parent_that_has_the_option(monkeypatch):
    name, tol = "synthetic-3000x3000x6", PANEL_TOL["synthetic-3000x3000x6"]
    ref = reference(name, "panel", tol, monkeypatch)
    parent = solver_for(name, "panel", monkeypatch, tol=tol, iteration_limit=400000, halpern_device_major=4)
    child = parent.clone()
    assert child.halpern_device_major() == 4 == parent.halpern_device_major()
    got_child = dict(result=child.advance(), solution=child.solution(), burst=child.device.halpern_burst_stats())
    got_parent = dict(result=parent.advance(), solution=parent.solution(), burst=parent.device.halpern_burst_stats())
    child.close()
    parent.close()
    print(got_child["burst"], got_parent["burst"])
    assert got_child["burst"]["records"] == got_parent["burst"]["records"] == ref["result"]["num_major_iterations"]  # (each its own ring)
    assert_same_solve(got_child, ref, "clone")
    assert_same_solve(got_parent, ref, "parent")


# ---- 7. the step error -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["resident", "panel"])
def test_a_step_error_ends_as_numerical_error_where_the_host_ends_it(path, monkeypatch):
    """an initial_step_size that overflows r^2 on the first step: the burst stops on the step error (a record that counts for no major
    iteration), the host-decided path evaluates and ends the solve exactly as with the option off -- a status of the solver"""
    name = AFIRO if path == "resident" else "synthetic-3000x3000x6"
    ref = finished(solver_for(name, path, monkeypatch, initial_step_size=1e200))
    got = finished(solver_for(name, path, monkeypatch, initial_step_size=1e200, halpern_device_major=4))
    print(path, ref["result"]["status_name"], ref["result"]["steps_taken"], got["result"]["status_name"], got["result"]["steps_taken"], got["burst"])
    assert ref["result"]["status_name"] == "NumericalError" == got["result"]["status_name"]
    assert got["result"]["steps_taken"] == ref["result"]["steps_taken"] and got["result"]["num_major_iterations"] == ref["result"]["num_major_iterations"]
    assert got["burst"]["bursts"] >= 1


# ---- 8. eligibility and refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,kw", [("stream", {}), ("jag", {}), ("panel", dict(per_constraint_residual=1))], ids=["stream", "jagged", "panel-per-constraint"])
def test_other_contexts_keep_the_host_decided_path(layout, kw, monkeypatch):
    name = "synthetic-3000x3000x6" if layout == "panel" else V50
    kw = dict(kw, iteration_limit=4000)  # (a bounded solve either way: what is compared is that the two runs are the same run)
    ref = finished(solver_for(name, layout, monkeypatch, **kw))
    got = finished(solver_for(name, layout, monkeypatch, halpern_device_major=4, **kw))
    print(layout, ref["result"]["status_name"], ref["result"]["steps_taken"], ref["stats"])
    assert got["major"] == 0 and "burst" not in got
    assert_same_solve(got, ref, layout)
    assert got["stats"]["loop_syncs"] == ref["stats"]["loop_syncs"]
    p = {k: v for k, v in lp_of(name).items() if k != "var_types"}
    extra = dict(per_constraint_residual=True) if layout == "panel" else {}
    r = capi.solve(p, method=1, pdlp_solver_mode=4, amd_halpern_device_major=4, iteration_limit=4000, **extra)
    assert r["return_code"] == 0 and r["solve_info"]["halpern_device_major"] == 0 and r["solve_info"]["pdlp_algorithm"] == "reflected_halpern"


REFUSED = [dict(halpern_infeasibility=1), dict(accept_enabled=1), dict(halpern_sharded=1), dict(halpern_batch=1), dict(halpern_lockstep=1)]


@pytest.mark.parametrize("kw", REFUSED, ids=[list(k)[0] for k in REFUSED])
def test_refusals_name_the_option(kw, monkeypatch):
    p = golden(AFIRO)
    with pytest.raises(capi.CuOptError) as e:
        capi.Solver(p, mode=4, halpern_resident=1, halpern_device_major=2, **kw)
    assert e.value.code == -7 and "halpern_device_major" in str(e.value), str(e.value)
    s = capi.Solver(p, mode=4, halpern_resident=1, halpern_device_major=2)
    ref = finished(capi.Solver(p, mode=4, halpern_resident=1))
    with pytest.raises(capi.CuOptError) as e:
        s.reset(halpern_resident=1, halpern_device_major=2, **kw)
    assert e.value.code == -7 and "halpern_device_major" in str(e.value), str(e.value)
    for bad in (-1, 17):
        with pytest.raises(capi.CuOptError) as e:
            s.reset(halpern_resident=1, halpern_device_major=bad)
        assert e.value.code == -1 and "halpern_device_major" in str(e.value), str(e.value)
    assert s.halpern_device_major() == 2  # a refused reset leaves the solver as it was: it finishes its solve
    assert_same_solve(finished(s), ref, "after refused resets")


def test_out_of_range_sharded_and_batch_refusals(monkeypatch):
    p = golden(AFIRO)
    for bad in (-1, 17):
        with pytest.raises(capi.CuOptError) as e:
            capi.Solver(p, mode=4, halpern_device_major=bad)
        assert e.value.code == -1 and "halpern_device_major" in str(e.value)
    with pytest.raises(capi.CuOptError) as e:  # any world > 1 (refused before anything is set up)
        capi.Solver(p, mode=4, halpern_device_major=2, halpern_sharded=0, rank=0, world=2, comm_id=bytes(128))
    assert e.value.code == -7 and "halpern_device_major" in str(e.value)
    # a batch refuses a member that has the option set, by name
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    q = synthetic.generate(3000, 3000, 6)
    parent = capi.Solver(q, mode=4, halpern_device_major=2)
    child = parent.clone()
    with pytest.raises(capi.CuOptError) as e:
        capi.SharedMatrixBatch([parent, child])
    assert e.value.code == -7 and "halpern_device_major" in str(e.value)
    child.close()
    parent.close()


def test_the_averaging_iteration_ignores_the_field():
    got = []
    for kw in (dict(), dict(halpern_device_major=4)):
        s = capi.Solver(golden(V50), mode=1, tol=0.0, **kw)
        r = s.advance(40)
        got.append((s.halpern_device_major(), r["steps_taken"], r["attempted_steps"], r["step_size"], r["primal_weight"]) + s.solution())
        s.close()
    assert got[0][:5] == got[1][:5] and got[0][0] == 0 and got[0][1] == 40
    for u, v in zip(got[0][5:], got[1][5:]):
        assert np.array_equal(bits(u), bits(v))


# ---- 9. through cuOptSolve and the Python mirror ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_mixed_bound_lps_through_cuoptsolve_against_highs(seed):
    p, A = random_lp(seed)
    ref = highs(p, A)
    r = capi.solve(p, method=1, pdlp_solver_mode=4, amd_halpern_resident=1, amd_halpern_device_major=4, tol=1e-8, iteration_limit=200000)
    print(seed, r["status"], r["steps_taken"], abs(r["objective"] - ref), r["solve_info"])
    assert r["status"] == "Optimal" and r["solve_info"]["pdlp_algorithm"] == "reflected_halpern" and r["solve_info"]["halpern_resident"] == 1
    assert r["solve_info"]["halpern_device_major"] == 4
    assert abs(r["objective"] - ref) <= 2e-6 * (1.0 + abs(ref))
    off = capi.solve(p, method=1, pdlp_solver_mode=4, amd_halpern_resident=1, tol=1e-8, iteration_limit=200000)
    assert off["solve_info"]["halpern_device_major"] == 0 and off["steps_taken"] == r["steps_taken"] and off["objective"] == r["objective"]
    np.testing.assert_array_equal(off["x"], r["x"])


def test_the_simplex_grade_emulation_drops_the_parameter():
    """a Concurrent request on a small LP is served at 1e-8 with the requested tolerances as acceptance set (the host keeps the accepted
    point): the parameter is dropped there, and the info field says so"""
    p, _ = random_lp(0)
    r = capi.solve(p, pdlp_solver_mode=4, amd_halpern_resident=1, amd_halpern_device_major=4, amd_dual_simplex=0)
    print(r["status"], r["solve_info"])
    assert r["return_code"] == 0 and r["status"] == "Optimal"
    assert r["solve_info"]["simplex_grade_emulation"] is True and r["solve_info"]["halpern_device_major"] == 0
