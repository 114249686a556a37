"""TEST UTILITY of tests/test_kept_point_gpu.py: the major iterations of a trajectory RECORDED on the device (the records
tests/kept_point_reference.py replays), the scenarios derived from them, and the comparison of a solve that had one of the two features
on against what the reference selects.

How a trajectory is recorded.  cuoptamd_solver_advance runs the major iteration that is due at the end of its budget before it returns
(restart included), so the iterates as the head of that major iteration saw them are gone by then.  The twin -- a solver without either
feature, otherwise under the scenario's settings -- is therefore reset once per major iteration b of the schedule with iteration_limit =
b and run to that limit: the head at b ends the solve in front of its restart, the result carries the current iterate's statistics
(T(z^k)'s in reflected Halpern mode) and the device still holds both iterates and the reduced costs that head evaluated.  The average
iterate's statistics come from pdlpdev_major_eval with the request the head made; the recording asserts that this second evaluation
reproduces the head's figures for the current iterate bit for bit and leaves both iterates and their reduced costs untouched, and that
the last record equals, bit for bit, a freshly created solver run to the same limit without any probing.  The features only snapshot:
a solve with one of them on takes the same trajectory (asserted through its step and attempt counts)."""
import numpy as np

import eval_reference as er
import kept_point_reference as kr
from cuopt_amd import capi
from kept_point_reference import AVERAGE, CURRENT

SKIP_FIELDS = ("setup_seconds", "loop_seconds", "status_name")
STATISTICS = ("primal_objective", "dual_objective", "gap", "l2_primal_residual", "l2_dual_residual")


def boundaries(hyper, horizon, halpern):
    """the iterations up to `horizon` at which a major iteration is due (major_due_at; Halpern: T(z^k) exists after a step)"""
    mi, mr = hyper.major_iteration, hyper.min_iteration_restart
    assert horizon % mi == 0, "a limit between two major iterations ends the solve at the next one"
    if halpern:
        return list(range(mi, horizon + 1, mi))
    return [b for b in range(horizon + 1) if b <= mr or b % mi == 0]


def caller_order(solver):
    """(columns, rows) -> functions that carry a vector of the device's order into the caller's"""
    info = solver.reorder_info(maps=True)
    if not info["reordered"]:
        return (lambda v: v), (lambda v: v), False

    def back(new2old):
        def f(v):
            out = np.empty_like(v)
            out[new2old] = v
            return out
        return f
    return back(info["col_new2old"]), back(info["row_new2old"]), True


class Trajectory:
    """records[i] (kept_point_reference's), results[i] (the twin's result dict at the limit of record i), points[(i, side)] = (x, y,
    reduced costs) in the caller's order -- read-only, shared among the tests"""

    def __init__(self, p, mode, settings, hyper):
        self.p, self.mode, self.settings, self.hyper = p, mode, settings, hyper
        self.halpern = mode == 4
        self.records, self.results, self.points = [], [], {}
        self.resident = self.reordered = False
        self.layout = None

    def index_of(self, limit):
        return [r["iteration"] for r in self.records].index(limit)

    def upto(self, limit):
        return self.records[:self.index_of(limit) + 1]


_cache = {}


def tolerances(st):
    return [getattr(st, k) for k in kr.TOLERANCE_KEYS]


def record_trajectory(key, p, horizon, mode=1, **settings):
    """the Trajectory of LP p under `settings` (neither feature among them) with a record per major iteration up to `horizon`; cached
    under `key` (which names everything else the trajectory depends on: the layout the environment forces)"""
    key = (key, horizon, mode, tuple(sorted(settings.items())))
    if key in _cache:
        return _cache[key]
    assert not settings.get("save_best_primal_so_far") and not settings.get("accept_enabled")
    solver = capi.Solver(p, mode=mode, iteration_limit=horizon, **settings)
    t = Trajectory(p, mode, dict(settings), solver.hyper)
    dev = solver.device
    t.layout = dev.layout()
    t.resident = t.layout["resident"]
    cols, rows, t.reordered = caller_order(solver)
    st = solver.settings
    tol, pc = tolerances(st), int(st.per_constraint_residual)
    rule_finite = solver.hyper.handle_some_primal_gradients_on_finite_bounds_as_residuals == 0
    eps_p, eps_d = (st.relative_primal_tolerance, st.relative_dual_tolerance) if pc else (-1.0, -1.0)
    scale, offset = (-1.0 if p.get("maximize") else 1.0), float(p.get("objective_offset", 0.0))
    n, m = p["n"], p["m"]
    for i, b in enumerate(boundaries(solver.hyper, horizon, t.halpern)):
        solver.reset(iteration_limit=b, **settings)
        r = solver.advance()
        assert r["status_name"] == "IterationLimit" and r["steps_taken"] == b, (b, r["status_name"], r["steps_taken"])
        sol = solver.solution()
        head = dict(r, abs_objective=abs(r["primal_objective"]) + abs(r["dual_objective"]), linf_rel_primal_residual=np.nan, linf_rel_dual_residual=np.nan)
        if t.halpern:
            # T(z^k), which lives in the average slots, is the one point of this iteration: the limit returns it
            assert r["returned_average"] == 0
            for f, u, v in zip((cols, rows, cols), sol, dev.solution(capi.AVERAGE, n, m)):
                np.testing.assert_array_equal(u, f(v))
            sides = {CURRENT: head, AVERAGE: head}
            t.points[(i, CURRENT)] = t.points[(i, AVERAGE)] = sol
        else:
            before = dev.solution(capi.CURRENT, n, m), dev.solution(capi.AVERAGE, n, m)
            ctl = dev.ctl()
            request = 0 if b <= 1 else (1 if ctl.its_since_restart == 0 else 2)  # major_eval_request
            ev_c, ev_a = dev.major_eval(request, rule_finite=rule_finite, eps_p=eps_p, eps_d=eps_d)
            after = dev.solution(capi.CURRENT, n, m), dev.solution(capi.AVERAGE, n, m)
            for u, v in zip(before[0] + before[1], after[0] + after[1]):
                np.testing.assert_array_equal(u, v, err_msg="the second evaluation at %d moved an iterate or its reduced costs" % b)
            cur, avg = kr.to_convergence(ev_c, scale, offset), kr.to_convergence(ev_a, scale, offset)
            for k in STATISTICS:
                assert cur[k] == r[k], ("the second evaluation at %d is not the head's" % b, k, cur[k], r[k])
            points = [tuple(f(v) for f, v in zip((cols, rows, cols), pt)) for pt in before]
            for u, v in zip(sol, points[0]):
                np.testing.assert_array_equal(u, v)
            sides = {CURRENT: cur, AVERAGE: avg}
            t.points[(i, CURRENT)], t.points[(i, AVERAGE)] = points
        sides = {w: dict(s, verdict=kr.verdict(s, tol, pc, r["norm_b"], r["norm_c"])) for w, s in sides.items()}
        assert not any(s["verdict"] == kr.OPTIMAL for s in sides.values()), "the scenario's own tolerances are met at %d" % b
        t.records.append(dict(iteration=b, primal_weight=r["primal_weight"], norm_b=r["norm_b"], norm_c=r["norm_c"], sides=sides,
                              counters={k: r[k] for k in ("steps_taken", "attempted_steps", "step_size", "primal_weight", "num_restarts", "num_major_iterations")}))
        t.results.append(r)
    solver.close()
    # the recording did not move the trajectory: an unprobed, freshly created solver run to the horizon
    fresh = capi.Solver(p, mode=mode, iteration_limit=horizon, **settings)
    same_result(fresh.advance(), t.results[-1], "the probed twin against an unprobed solver")
    for u, v in zip(fresh.solution(), t.points[(len(t.records) - 1, AVERAGE if t.halpern else CURRENT)]):
        np.testing.assert_array_equal(u, v)
    fresh.close()
    for pt in t.points.values():
        for a in pt:
            a.setflags(write=False)
    _cache[key] = t
    return t


def same_result(got, want, what):
    for k, v in want.items():
        if k in SKIP_FIELDS:
            continue
        assert got[k] == v, (what, k, got[k], v)


# ---- scenarios derived from a record --------------------------------------------------------------------------------------------------
def need(side, rec, per_constraint):
    """the least uniform tolerance eps (all six of the set) under which `side` is accepted, up to rounding"""
    gap = side["gap"] / (1.0 + side["abs_objective"])
    if per_constraint:
        return max(gap, side["linf_rel_primal_residual"], side["linf_rel_dual_residual"])
    return max(gap, side["l2_primal_residual"] / (1.0 + rec["norm_b"]), side["l2_dual_residual"] / (1.0 + rec["norm_c"]))


def acceptance_scenario(t, target, both=False):
    """(accept_tolerance, index of the accepting record, iteration_limit): the looser set is the uniform tolerance the better iterate of
    the major iteration at `target` just meets (both: the worse one, so that both iterates meet it there), the accepting record M_a is
    the one the REFERENCE rule then finds (at `target` or before), the limit lies three major iterations behind it"""
    pc = bool(t.settings.get("per_constraint_residual"))
    rec = t.records[t.index_of(target)]
    eps = (max if both else min)(need(rec["sides"][w], rec, pc) for w in ((AVERAGE,) if t.halpern else (CURRENT, AVERAGE))) * (1.0 + 1e-9)
    accept = [eps] * 6
    kept = kr.replay_accepted(t.records, accept, pc, halpern=t.halpern)
    assert kept is not None and t.records[kept[0]]["iteration"] <= target, (kept, eps)
    limit = t.records[kept[0]]["iteration"] + 3 * t.hyper.major_iteration
    assert limit <= t.records[-1]["iteration"], "the recorded horizon is too short"
    print("ACCEPTANCE eps=%.3e accepted at %d (%s), limit %d" % (eps, t.records[kept[0]]["iteration"], "current" if kept[1] == CURRENT else "average", limit))
    return accept, kept, limit


def kept_is_not_the_last(t, limit):
    """the best primal point at iteration_limit = limit comes from a major iteration in front of the last one"""
    recs = t.upto(limit)
    return kr.replay_best_primal(recs, bool(t.p.get("maximize")))[-1][0] < len(recs) - 1


def best_primal_limits(t):
    """the horizon and, in front of it when there is one, the latest limit at which the kept point is NOT the last major iteration's"""
    horizon, mi = t.records[-1]["iteration"], t.hyper.major_iteration
    earlier = [b for b in range(2 * mi, horizon, mi) if kept_is_not_the_last(t, b)]
    return ([] if kept_is_not_the_last(t, horizon) else earlier[-1:]) + [horizon]


def expected(t, limit, save_best_primal_so_far=False, accept_tolerance=None):
    """what a solve of t's LP under t's settings plus the feature must return at iteration_limit = limit: (kept, result dict, (x, y,
    reduced costs)); kept = (index of the record, side) or None"""
    recs = t.upto(limit)
    kept, res = kr.finish_solve(recs, kr.ITERATION_LIMIT, save_best_primal_so_far=save_best_primal_so_far, accept_tolerance=accept_tolerance,
                                per_constraint=bool(t.settings.get("per_constraint_residual")), maximize=bool(t.p.get("maximize")), halpern=t.halpern)
    want = dict(t.results[len(recs) - 1])  # (norms, initial step and weight, the ray fields: the twin's)
    want.update(res)
    point = t.points[kept] if kept is not None else t.points[(len(recs) - 1, AVERAGE if t.halpern else CURRENT)]
    return kept, want, point


def feature_settings(t, limit, save_best_primal_so_far=False, accept_tolerance=None):
    kw = dict(t.settings, iteration_limit=limit)
    if save_best_primal_so_far:
        kw["save_best_primal_so_far"] = 1
    if accept_tolerance is not None:
        kw.update(accept_enabled=1, accept_tolerance=tuple(accept_tolerance))
    return kw


def check(result, solution, want, point, what):
    """the core assertion: the result is the one the reference assembles (every field but the clocks, ints and doubles exactly) and the
    point is the recorded one, bit for bit"""
    same_result(result, want, what)
    for u, v, name in zip(solution, point, ("x", "y", "reduced costs")):
        np.testing.assert_array_equal(u, v, err_msg="%s: %s" % (what, name))


def check_same_trajectory(solver, t, limit, what):
    """the feature only snapshots: the device took the steps and attempts of the twin"""
    c, final = solver.device.ctl(), t.results[t.index_of(limit)]
    assert (c.steps_taken, c.attempts) == (final["steps_taken"], final["attempted_steps"]), (what, c.steps_taken, c.attempts)


def both_accepted(t, accept, kept):
    """both iterates of the accepting major iteration meet the set: the KKT score chose"""
    rec, pc = t.records[kept[0]], bool(t.settings.get("per_constraint_residual"))
    return all(kr.accepted_by_looser(rec["sides"][w], accept, pc, rec["norm_b"], rec["norm_c"]) for w in (CURRENT, AVERAGE))


# ---- the reported statistics against the extended-precision evaluation ------------------------------------------------------------------
def statistics_bounds(p, x, y, rule_finite=True):
    """(reference, bounds) for l2_primal_residual, primal_objective and l2_dual_residual of the point (x, y) of LP p (a maximisation is
    evaluated as the minimisation the device solves, its objective negated back).  Derived from eval_reference's per-element bounds, with
    u = 2^-53:
      l2_primal_residual  a row's violation is a 1-Lipschitz function of (A x)_i, so the vector of violations is off by at most
                          ||bound_ax||_2 in norm; the subtraction of the bound, the squares, their sum over m rows in any order and
                          the root add at most (m + 8) u relative.
      primal_objective    sum_j c_j x_j with five roundings per term (as for a matrix entry) in any order: (n + 16) u sum |c_j x_j|,
                          and one rounding for the sign and offset.
      l2_dual_residual    a column's residual g_j - rc_j is off by at most bound_aty_j -- and by |g_j| more where the reduced-cost
                          DECISION is a near tie (eval_reference.near_tie: it may fall either way); sum and root as above with n."""
    q = dict(p, c=-np.asarray(p["c"])) if p.get("maximize") else p
    ref = er.evaluate(q, x, y, rule_finite=rule_finite, eps_p=-1.0, eps_d=-1.0)
    m, n = p["m"], p["n"]
    sign, offset = (-1.0 if p.get("maximize") else 1.0), float(p.get("objective_offset", 0.0))
    pres, dres, pobj = np.sqrt(ref["PRES2"]), np.sqrt(ref["DRES2"]), sign * ref["CX"] + offset
    g = np.abs(np.asarray(q["c"], dtype=np.float64) - ref["aty"]) + ref["bound_aty"]
    per_col = ref["bound_aty"] + np.where(ref["near_tie"], g, 0.0)
    bounds = dict(l2_primal_residual=np.linalg.norm(ref["bound_ax"]) * (1 + 1e-6) + (m + 8) * er.U * pres,
                  primal_objective=(n + 16) * er.U * float(np.abs(np.asarray(q["c"]) * np.asarray(x)).sum()) + 2 * er.U * abs(pobj),
                  l2_dual_residual=np.linalg.norm(per_col) * (1 + 1e-6) + (n + 8) * er.U * dres)
    return dict(l2_primal_residual=pres, primal_objective=pobj, l2_dual_residual=dres), bounds


def check_statistics(p, result, solution, what, rule_finite=True):
    """the reported statistics are those of the returned point, within the derived bounds"""
    ref, bounds = statistics_bounds(p, solution[0], solution[1], rule_finite)
    for k in ("l2_primal_residual", "primal_objective", "l2_dual_residual"):
        err = abs(result[k] - ref[k])
        print("STATISTIC %s %s reported=%.17g reference=%.17g error=%.3e bound=%.3e" % (what, k, result[k], ref[k], err, bounds[k]))
        assert err <= bounds[k], (what, k, result[k], ref[k], err, bounds[k])
