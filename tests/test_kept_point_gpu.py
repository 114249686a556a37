"""GPU: the KEPT iterate -- save_best_primal_so_far and the acceptance set (accept_enabled / accept_tolerance), one snapshot mechanism
(pdlpdev_save_best -> the best buffers -> PDLPDEV_BEST) -- on every solve path, against tests/kept_point_reference.py.

For each path a twin without either feature is recorded major iteration by major iteration (tests/kept_point_case.py: both iterates, their
reduced costs, their evaluations), the reference replays the host rules on the records and names the record and the side (current /
average) that must have been kept, and the solve with the feature on must return exactly that: every field of the result but the clocks
(ints and doubles compared exactly) and x, y and the reduced costs bit for bit.  On the single-LP paths the reported l2_primal_residual,
primal_objective and l2_dual_residual are also held against the extended-precision evaluation of the returned point
(tests/eval_reference.py) within bounds derived there -- no measured tolerance.  A sharded solve has no bitwise twin (its reductions
take another order): its returned point must carry the reported statistics within the same derived bounds and be no worse in primal
residual than the same solve without the feature.

The scenarios are derived from the records, not fixed: the looser tolerance set is the one the better iterate of a chosen major iteration
just meets, the iteration limit lies three major iterations behind the acceptance the REFERENCE then finds; the best-primal limits are
the horizon and the latest limit at which the kept point is not the last major iteration's.  The assertions that keep the tests from
being vacuous: the accepted x differs from the final current x and from the other iterate of its major iteration; over the LPs of this
file the recording rule stores at two different major iterations of one LP at least, keeps CURRENT and keeps AVERAGE, and one LP ends
with a kept point that is not the last major iteration's (test_the_best_primal_scenarios_are_not_vacuous)."""
import functools

import numpy as np
import pytest
from conftest import set_tune

import kept_point_case as kc
import kept_point_reference as kr
from cuopt_amd import capi, synthetic
from kept_point_reference import AVERAGE, CURRENT

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

LIMIT = 6000  # (of the members that are to end Optimal)


@functools.lru_cache(maxsize=None)
def multi_launch_lp(maximize=False):
    p = synthetic.generate(3000, 3000, 6, seed=2, hard=True)  # not resident (test_small_batch_gpu.test_who_is_turned_away)
    return dict(p, c=-p["c"], maximize=True) if maximize else p


@functools.lru_cache(maxsize=None)
def synthetic_resident(name):
    return {"1000x1000": lambda: synthetic.generate(1000, 1000, 8, seed=4), "200x500": lambda: synthetic.generate(200, 500, 6, seed=6)}[name]()


RESIDENT = ("afiro", "1000x1000", "200x500")


def resident_lp(golden_problems, name):
    return golden_problems["afiro"]["problem"] if name == "afiro" else synthetic_resident(name)


def periods(mode, count):
    return count * capi.hyper_preset(mode).major_iteration


def rule_finite(t):
    return t.hyper.handle_some_primal_gradients_on_finite_bounds_as_residuals == 0


def solve_and_check(t, limit, what, statistics=True, **feature):
    """one Solver on t's LP with the feature on, against what the reference selects from t's records"""
    kept, want, point = kc.expected(t, limit, **feature)
    s = capi.Solver(t.p, mode=t.mode, **kc.feature_settings(t, limit, **feature))
    assert s.device.layout() == t.layout
    r, sol = s.advance(), s.solution()
    print("KEPT %s: %s, status %s" % (what, kept and (t.records[kept[0]]["iteration"], "current" if kept[1] == CURRENT else "average"), r["status_name"]))
    kc.check(r, sol, want, point, what)
    kc.check_same_trajectory(s, t, limit, what)
    if statistics:
        kc.check_statistics(t.p, r, sol, what, rule_finite(t))
    s.close()
    return kept


def acceptance(t, target, both=False):
    """the acceptance scenario of trajectory t and the assertions that a wrong buffer would be visible"""
    accept, kept, limit = kc.acceptance_scenario(t, target, both)
    x = t.points[kept][0]
    assert t.index_of(limit) - kept[0] >= 3 and t.records[kept[0]]["iteration"] > 1
    assert not np.array_equal(x, t.points[(t.index_of(limit), CURRENT)][0]), "the accepted x is the final current x"
    if not t.halpern:
        assert not np.array_equal(x, t.points[(kept[0], AVERAGE if kept[1] == CURRENT else CURRENT)][0])
    return accept, kept, limit


# ---- the multi-launch single LP --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("primal_tolerance", [0.0, 1e-3], ids=["least-residual", "feasible-then-objective"])
@pytest.mark.parametrize("maximize", [False, True], ids=["minimize", "maximize"])
def test_multi_launch_best_primal(maximize, primal_tolerance):
    """tolerances of zero: no iterate is ever feasible and the least residual decides.  A relative primal tolerance alone (gap and dual
    tolerances stay zero: the verdict is PrimalFeasible at best, which ends nothing): feasible beats infeasible, then the objective
    decides -- the higher one for the maximisation (c negated and the flag set: the same minimisation on the device, the objective
    reported with the other sign)"""
    p = multi_launch_lp(maximize)
    t = kc.record_trajectory("multi-launch maximize=%d" % maximize, p, periods(1, 10), tol=0.0, relative_primal_tolerance=primal_tolerance)
    assert not t.resident
    feasible = [any(s["verdict"] == kr.PRIMAL_FEASIBLE for s in rec["sides"].values()) for rec in t.records]
    assert (sum(feasible) >= 2 and not all(feasible)) if primal_tolerance else not any(feasible), feasible
    for limit in kc.best_primal_limits(t):
        kept = solve_and_check(t, limit, "multi-launch best primal, limit %d" % limit, save_best_primal_so_far=True)
        assert kept is not None


@pytest.mark.parametrize("per_constraint", [0, 1])
def test_multi_launch_acceptance_set(per_constraint):
    t = kc.record_trajectory("multi-launch", multi_launch_lp(), periods(1, 8), tol=1e-9, per_constraint_residual=per_constraint)
    assert not t.resident
    accept, kept, limit = acceptance(t, periods(1, 5))
    assert solve_and_check(t, limit, "multi-launch acceptance set, per_constraint_residual=%d" % per_constraint, accept_tolerance=accept) == kept
    # a set that BOTH iterates of the accepting major iteration meet: the KKT score decides which one is kept
    chosen = [c for c in (acceptance(t, target, both=True) for target in range(periods(1, 2), periods(1, 5) + 1, periods(1, 1))) if kc.both_accepted(t, c[0], c[1])]
    assert chosen, "no major iteration at which the reference accepts both iterates"
    assert solve_and_check(t, chosen[0][2], "multi-launch acceptance set met by both iterates", accept_tolerance=chosen[0][0]) == chosen[0][1]
    # save_best_primal_so_far switches the set off: the best primal point comes back, with the limit's status
    kept = solve_and_check(t, limit, "multi-launch, both features", save_best_primal_so_far=True, accept_tolerance=accept)
    assert kept == kr.replay_best_primal(t.upto(limit))[-1]


# ---- the resident one-workgroup loop ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RESIDENT)
def test_resident_best_primal(golden_problems, name):
    t = kc.record_trajectory("resident " + name, resident_lp(golden_problems, name), periods(1, 6), tol=0.0)
    assert t.resident
    for limit in kc.best_primal_limits(t):
        assert solve_and_check(t, limit, "resident %s best primal, limit %d" % (name, limit), save_best_primal_so_far=True) is not None


@pytest.mark.parametrize("name", RESIDENT)
def test_resident_acceptance_set(golden_problems, name):
    t = kc.record_trajectory("resident " + name, resident_lp(golden_problems, name), periods(1, 6), tol=1e-9)
    assert t.resident
    accept, kept, limit = acceptance(t, periods(1, 3))
    assert solve_and_check(t, limit, "resident %s acceptance set" % name, accept_tolerance=accept) == kept


def test_the_best_primal_scenarios_are_not_vacuous(golden_problems):
    """over the LPs of this file: stores at two different major iterations of one LP, CURRENT kept and AVERAGE kept, and a kept point that
    is not the last major iteration's at the end of one solve"""
    ts = [kc.record_trajectory("multi-launch maximize=%d" % mx, multi_launch_lp(mx), periods(1, 10), tol=0.0, relative_primal_tolerance=0.0) for mx in (False, True)]
    ts += [kc.record_trajectory("resident " + name, resident_lp(golden_problems, name), periods(1, 6), tol=0.0) for name in RESIDENT]
    stores = [kr.replay_best_primal(t.records, bool(t.p.get("maximize"))) for t in ts]
    for t, s in zip(ts, stores):
        print("STORES", t.p["m"], t.p["n"], [(t.records[i]["iteration"], "current" if w == CURRENT else "average") for i, w in s], kc.best_primal_limits(t))
    assert any(len({i for i, _ in s}) >= 2 for s in stores)
    assert any(w == CURRENT for s in stores for _, w in s) and any(w == AVERAGE for s in stores for _, w in s)
    assert any(kc.kept_is_not_the_last(t, limit) for t in ts for limit in kc.best_primal_limits(t))


# ---- the K-workgroup batch of resident LPs -----------------------------------------------------------------------------------------------
def small_members(golden_problems):
    """twelve members over the three matrices: best primal (ends on its limit), the acceptance set (ends on its limit), neither and best
    primal under tolerances that are met (end Optimal) -> [(p, settings, (trajectory, limit, feature) or None)]"""
    out = []
    for name in RESIDENT:
        p = resident_lp(golden_problems, name)
        tb = kc.record_trajectory("resident " + name, p, periods(1, 6), tol=0.0)
        ta = kc.record_trajectory("resident " + name, p, periods(1, 6), tol=1e-9)
        accept, _, limit = acceptance(ta, periods(1, 3))
        best_limit = kc.best_primal_limits(tb)[0]
        out += [(p, kc.feature_settings(tb, best_limit, save_best_primal_so_far=True), (tb, best_limit, dict(save_best_primal_so_far=True))),
                (p, kc.feature_settings(ta, limit, accept_tolerance=accept), (ta, limit, dict(accept_tolerance=accept))),
                (p, dict(tol=1e-4, iteration_limit=LIMIT), None),
                (p, dict(tol=1e-4, iteration_limit=LIMIT, save_best_primal_so_far=1), None)]
    return out


@pytest.mark.parametrize("chunks", [(2 ** 31 - 1,), (90, 90, 2 ** 31 - 1)], ids=["one-call", "90-90-rest"])
def test_small_batch_members_keep_what_their_single_solves_keep(golden_problems, chunks):
    members = small_members(golden_problems)
    K = len(members)
    ones = [capi.Solver(p, **kw) for p, kw, _ in members]
    many = [capi.Solver(p, **kw) for p, kw, _ in members]
    for s in many:
        assert s.device.layout()["resident"]
    batch = capi.SmallBatch(many)
    want = []
    for s in ones:
        for c in chunks:
            r = s.advance(c)
        want.append((r, s.solution()))
    for c in chunks:
        got = batch.advance(c)
    sols, views = batch.solutions(), batch.solution_views()
    for l, (p, kw, scenario) in enumerate(members):
        what = "member %d %s" % (l, sorted(kw.items()))
        kc.same_result(got[l], dict(want[l][0], setup_seconds=0), what)
        for source in (many[l].solution(), sols[l], views[l]):
            for u, v in zip(want[l][1], source):
                np.testing.assert_array_equal(u, v, err_msg=what)
        if scenario is not None:  # ... and both are what the reference selects
            t, limit, feature = scenario
            kept, res, point = kc.expected(t, limit, **feature)
            assert kept is not None
            kc.check(got[l], sols[l], res, point, what)
    statuses = [r["status_name"] for r in got]
    assert statuses == ["IterationLimit", "Optimal", "Optimal", "Optimal"] * 3, statuses
    assert [r["accepted_at_looser_tolerances"] for r in got] == [0, 1, 0, 0] * 3
    # branching on the device from what the last solve RETURNED (the kept point where a limit ended it) against the trip through the
    # host: Solver.reset(full bounds, the solution read back) -- then a second solve under the same settings
    var, lo, hi = np.full(K, -1, np.int32), np.zeros(K), np.zeros(K)
    for l, (p, kw, _) in enumerate(members):
        x = want[l][1][0]
        lb, ub = np.array(p["lb"], float), np.array(p["ub"], float)
        j = int(np.argmax(np.abs(x)))
        ub[j] = max(min(ub[j], x[j] - 0.5 * abs(x[j]) - 0.125), lb[j])  # (the variable's value is cut off)
        var[l], lo[l], hi[l] = j, lb[j], ub[j]
        ones[l].reset(lb=lb, ub=ub, init_x=want[l][1][0], init_y=want[l][1][1])
    batch.branch(var, lo, hi)
    want = [(s.advance(), s.solution()) for s in ones]
    got = batch.advance()
    sols = batch.solutions()
    print("SECOND SOLVES", [r["status_name"] for r in got])
    for l in range(K):
        kc.same_result(dict(got[l], setup_seconds=0), dict(want[l][0], setup_seconds=0), "member %d after the branch" % l)
        for u, v in zip(want[l][1], sols[l]):
            np.testing.assert_array_equal(u, v, err_msg="member %d after the branch" % l)
    batch.close()
    for s in ones + many:
        s.close()


def test_batch_solve_keeps_the_best_primal_point_on_both_routes(golden_problems, monkeypatch):
    names = RESIDENT + RESIDENT
    ts = [kc.record_trajectory("resident " + name, resident_lp(golden_problems, name), periods(1, 6), tol=0.0) for name in names]
    limit = periods(1, 6)
    runs = {}
    for route in (0, 1):
        set_tune(monkeypatch, small_batch=route)
        runs[route] = capi.batch_solve([t.p for t in ts], save_best_primal_so_far=1, tol=0.0, iteration_limit=limit)
        assert (capi.batch_solve_last_path() == "small") == bool(route), capi.batch_solve_last_path()
    for l, t in enumerate(ts):
        kept, want, point = kc.expected(t, limit, save_best_primal_so_far=True)
        for route in (0, 1):
            g = runs[route][l]
            kc.check({k: v for k, v in g.items() if k not in ("x", "y", "reduced_cost")}, (g["x"], g["y"], g["reduced_cost"]), want, point, "LP %d, small_batch=%d" % (l, route))


# ---- lockstep batches over one matrix ----------------------------------------------------------------------------------------------------
def lockstep_case(p, key, K, layout, mode=1, **create):
    """a parent and K - 1 clones of LP p with per-member settings (clone(**setting_overrides)): best primal, the acceptance set, neither,
    best primal at the horizon -- each member against what the reference selects from the twin's records"""
    tb = kc.record_trajectory(key, p, periods(mode, 6), mode=mode, tol=0.0, **create)
    ta = kc.record_trajectory(key, p, periods(mode, 6), mode=mode, tol=1e-9, **create)
    for t in (tb, ta):
        assert t.layout["A"]["layout"] == layout and t.layout["At"]["layout"] == layout, t.layout
    accept, _, limit = acceptance(ta, periods(mode, 3))
    best = dict(save_best_primal_so_far=True) if mode != 4 else {}  # (the Halpern mode refuses it)
    specs = [(ta, limit, dict(accept_tolerance=accept)), (tb, kc.best_primal_limits(tb)[0], best), (tb, periods(mode, 5), {}), (tb, periods(mode, 6), best)][:K]
    parent = capi.Solver(p, mode=mode, **kc.feature_settings(*specs[0][:2], **specs[0][2]))
    solvers = [parent] + [parent.clone(**kc.feature_settings(t, lim, **feature)) for t, lim, feature in specs[1:]]
    assert parent.device.layout() == ta.layout
    batch = capi.SharedMatrixBatch(solvers)
    got = batch.advance()
    for l, (t, lim, feature) in enumerate(specs):
        kept, want, point = kc.expected(t, lim, **feature)
        assert (kept is not None) == bool(feature)
        kc.check(got[l], solvers[l].solution(), want, point, "%s member %d of %d %s" % (key, l, K, sorted(feature)))
        kc.check_same_trajectory(solvers[l], t, lim, "member %d" % l)
    batch.close()
    for s in solvers[1:]:
        s.close()
    parent.close()


@pytest.mark.parametrize("K", [2, 4])
def test_lockstep_batch_on_the_panels(K, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    lockstep_case(synthetic.generate(6000, 5000, 8, seed=33), "lockstep panel", K, "panel")


def test_lockstep_batch_on_the_jagged_layout(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "jag")
    lockstep_case(synthetic.generate(4000, 3500, 6, seed=12, band=200), "lockstep jag", 4, "jag", batch_lanes=4)


# ---- reflected Halpern mode: the acceptance set keeps T(z^k) ---------------------------------------------------------------------------
def test_halpern_multi_launch_acceptance_set():
    t = kc.record_trajectory("multi-launch", multi_launch_lp(), periods(4, 8), mode=4, tol=1e-9)
    assert not t.resident
    accept, kept, limit = acceptance(t, periods(4, 5))
    assert solve_and_check(t, limit, "Halpern multi-launch acceptance set", accept_tolerance=accept) == kept


@pytest.mark.parametrize("name", RESIDENT)
def test_halpern_resident_acceptance_set(golden_problems, name):
    t = kc.record_trajectory("resident " + name, resident_lp(golden_problems, name), periods(4, 6), mode=4, tol=1e-9, halpern_resident=1)
    assert t.resident
    accept, kept, limit = acceptance(t, periods(4, 3))
    assert solve_and_check(t, limit, "Halpern resident %s acceptance set" % name, accept_tolerance=accept) == kept


def test_halpern_small_batch_acceptance_set(golden_problems):
    """K workgroups of the resident Halpern loop: per matrix one member with the acceptance set (ends on its limit with the kept
    T(z^k)) and one without (the limit's own point)"""
    specs = []
    for name in RESIDENT:
        t = kc.record_trajectory("resident batch " + name, resident_lp(golden_problems, name), periods(4, 6), mode=4, tol=1e-9, halpern_resident=1, halpern_batch=1)
        accept, _, limit = acceptance(t, periods(4, 3))
        specs += [(t, limit, dict(accept_tolerance=accept)), (t, periods(4, 5), {})]
    solvers = [capi.Solver(t.p, mode=4, **kc.feature_settings(t, limit, **feature)) for t, limit, feature in specs]
    batch = capi.SmallBatch(solvers)
    assert batch.stats()["halpern"] == 1
    for c in (90, 2 ** 31 - 1):
        got = batch.advance(c)
    sols = batch.solutions()
    for l, (t, limit, feature) in enumerate(specs):
        kept, want, point = kc.expected(t, limit, **feature)
        assert (kept is not None) == bool(feature) and want["returned_average"] == 0
        for source in (solvers[l].solution(), sols[l]):
            kc.check(got[l], source, want, point, "Halpern batch member %d" % l)
    batch.close()
    for s in solvers:
        s.close()


def test_halpern_lockstep_acceptance_set(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    lockstep_case(synthetic.generate(6000, 5000, 8, seed=33), "Halpern lockstep panel", 2, "panel", mode=4, halpern_lockstep=1)


# ---- a reordered LP: the kept point comes back in the caller's order -------------------------------------------------------------------
REORDERED_ROWS = 131072  # the smallest power of two at which the analysis reorders a shuffled band (65536 and below stay as they arrive, on the CSR stream)


def test_reordered_lp_returns_the_kept_point_in_the_callers_order():
    """a shuffled banded LP the set-up's analysis puts back in order: the twin works on P A Q too, its average iterate and reduced costs
    are downloaded in the DEVICE's order and carried into the caller's by the maps here, independently of the solver's own way back"""
    q = synthetic.shuffled(synthetic.generate(REORDERED_ROWS, REORDERED_ROWS, 10, seed=2, band=2000), seed=5)
    t = kc.record_trajectory("reordered", q, periods(1, 3), tol=0.0)
    assert t.reordered
    for limit in kc.best_primal_limits(t):
        assert solve_and_check(t, limit, "reordered best primal, limit %d" % limit, save_best_primal_so_far=True) is not None
    t = kc.record_trajectory("reordered", q, periods(1, 5), tol=1e-9)
    accept, kept, limit = acceptance(t, periods(1, 2))
    assert solve_and_check(t, limit, "reordered acceptance set", accept_tolerance=accept) == kept


# ---- a sharded solve ---------------------------------------------------------------------------------------------------------------------
def test_sharded_best_primal(monkeypatch):
    """world 2 through the in-process communicator: no bitwise twin, so the returned (x, y) must carry the reported statistics within
    the derived bounds, and its primal residual must not exceed that of the same sharded solve without the feature"""
    set_tune(monkeypatch, soft_communicator=1)
    p = multi_launch_lp()
    kw = dict(method=1, tol=0.0, iteration_limit=periods(1, 5), amd_num_gpus=2)
    plain = capi.solve(p, **kw)
    best = capi.solve(p, save_best_primal_so_far=True, **kw)
    assert plain["status"] == best["status"] == "IterationLimit" and plain["gpus"] == best["gpus"] == 2
    for r, what in ((plain, "sharded, the limit's point"), (best, "sharded best primal")):
        kc.check_statistics(p, r, (r["x"], r["y"]), what, capi.hyper_preset(1).handle_some_primal_gradients_on_finite_bounds_as_residuals == 0)
    assert best["l2_primal_residual"] <= plain["l2_primal_residual"]
