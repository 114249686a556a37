"""TEST UTILITY: which point a solve must have KEPT, restated in plain Python from records of its major iterations.

Two features share one snapshot (pdlpdev_save_best -> the best buffers -> returned_which = PDLPDEV_BEST): save_best_primal_so_far (the
recording rule of major_head with best_of / Quality) and the acceptance set (accept_enabled / accept_tolerance: keep_accepted_point from
major_head, or from halpern_major_head with T(z^k)).  finish_solve hands the kept point back when a limit ends the solve.  What is
restated here is cuopt_amd/csrc/pdlp_solver.cpp: to_convergence, verdict (without the infeasibility information: no scenario of the
tests switches detection on), kkt_score, accepted_by_looser, best_of, the two recording rules and finish_solve.  numpy only (square
roots and absolute values of doubles: the same IEEE operations the host code performs, so the statistics are bit for bit the host's).

A RECORD is one major iteration of a trajectory, a dict:
    iteration             total_iterations at the head
    primal_weight         the weight of the KKT score (ctl.primal_weight at the head)
    norm_b, norm_c        the norms of the termination rule
    counters              dict(steps_taken, attempted_steps, step_size, primal_weight, num_restarts, num_major_iterations): what a result
                          filled at this head carries besides the statistics of a point
    sides                 {CURRENT: side, AVERAGE: side}; a side is a dict with verdict (OPTIMAL, PRIMAL_FEASIBLE or NO_VERDICT),
                          primal_objective, dual_objective, gap, abs_objective, l2_primal_residual, l2_dual_residual,
                          linf_rel_primal_residual, linf_rel_dual_residual.  Reflected Halpern mode: both sides are T(z^k).
Records come in the order of the trajectory; the last one is the major iteration at which the limit ended the solve."""
import numpy as np

CURRENT, AVERAGE = 0, 1
# pdlp_termination_status_t as the host driver uses it (NO_VERDICT: "keep going", which the reference encodes as NumericalError)
OPTIMAL, ITERATION_LIMIT, TIME_LIMIT, NO_VERDICT, PRIMAL_FEASIBLE = 1, 4, 5, 6, 7

TOLERANCE_KEYS = ("absolute_gap_tolerance", "relative_gap_tolerance", "absolute_primal_tolerance", "relative_primal_tolerance",
                  "absolute_dual_tolerance", "relative_dual_tolerance")


def to_convergence(ev, objective_scale=1.0, objective_offset=0.0):
    """to_convergence: the eight raw outputs of an evaluation (CX, DUAL_SUM, PRES2, DRES2, X2, Y2, LINF_PRES_REL, LINF_DRES_REL) -> a side
    without its verdict"""
    pobj, dobj = float(ev[0]), float(ev[1])
    if objective_scale != 1.0 or objective_offset != 0.0:
        pobj = objective_scale * pobj + objective_offset
        dobj = objective_scale * dobj + objective_offset
    return dict(primal_objective=pobj, dual_objective=dobj, gap=abs(pobj - dobj), abs_objective=abs(pobj) + abs(dobj),
                l2_primal_residual=float(np.sqrt(np.float64(ev[2]))), l2_dual_residual=float(np.sqrt(np.float64(ev[3]))),
                linf_rel_primal_residual=float(ev[6]), linf_rel_dual_residual=float(ev[7]))


def _meets(side, tol, per_constraint, norm_b, norm_c):
    """the three inequalities of check_termination_criteria_kernel under the six tolerances `tol` -> (gap, primal, dual)"""
    gap_ok = side["gap"] <= tol[0] + tol[1] * side["abs_objective"]
    if per_constraint:
        return gap_ok, side["linf_rel_primal_residual"] <= tol[2], side["linf_rel_dual_residual"] <= tol[4]
    return gap_ok, side["l2_primal_residual"] <= tol[2] + tol[3] * norm_b, side["l2_dual_residual"] <= tol[4] + tol[5] * norm_c


def verdict(side, tol, per_constraint, norm_b, norm_c):
    """verdict() with detect_infeasibility off: Optimal, PrimalFeasible, or keep going"""
    gap_ok, primal_ok, dual_ok = _meets(side, tol, per_constraint, norm_b, norm_c)
    if gap_ok and primal_ok and dual_ok:
        return OPTIMAL
    return PRIMAL_FEASIBLE if primal_ok else NO_VERDICT


def accepted_by_looser(side, accept_tolerance, per_constraint, norm_b, norm_c):
    return all(_meets(side, accept_tolerance, per_constraint, norm_b, norm_c))


def kkt_score(side, w):
    w2 = w * w
    return float(np.sqrt(np.float64(w2 * side["l2_primal_residual"] * side["l2_primal_residual"] +
                                    side["l2_dual_residual"] * side["l2_dual_residual"] / w2 + side["gap"] * side["gap"])))


def quality(side):
    """Quality of major_head: (feasible, residual, objective)"""
    return (side["verdict"] == PRIMAL_FEASIBLE, side["l2_primal_residual"], side["primal_objective"])


def best_of(a, b, maximize):
    """best_of: 0 when a wins, 1 when b does.  Feasible beats infeasible; two feasible ones: the objective (a wins only when strictly
    lower -- maximize: when not strictly lower); otherwise the least residual (a wins only when strictly less)."""
    if a[0] and not b[0]:
        return 0
    if b[0] and not a[0]:
        return 1
    if a[0] and b[0]:
        a_lower = a[2] < b[2]
        return 0 if ((not maximize and a_lower) or (maximize and not a_lower)) else 1
    return 0 if a[1] < b[1] else 1


def terminates(record):
    """check_termination of major_head without first_primal_feasible and infeasibility detection: (done, side).  Nothing but the limits
    during the first two iterations; both Optimal -> the lower KKT score, ties to the average; else the average, else the current."""
    if record["iteration"] <= 1:
        return False, None
    cur, avg = record["sides"][CURRENT], record["sides"][AVERAGE]
    w = record["primal_weight"]
    if cur["verdict"] == OPTIMAL and avg["verdict"] == OPTIMAL:
        return True, CURRENT if kkt_score(cur, w) < kkt_score(avg, w) else AVERAGE
    if avg["verdict"] == OPTIMAL:
        return True, AVERAGE
    if cur["verdict"] == OPTIMAL:
        return True, CURRENT
    return False, None


def replay_best_primal(records, maximize=False):
    """the recording rule of major_head (record_best_primal_so_far): [(index of the record, side)] of every store, in order.  The candidate
    of a major iteration is the better of its two iterates (the average where neither is better); it replaces the stored point unless the
    stored one is at least as good -- equal quality does not replace --, and the first record always stores.  A major iteration that
    terminates the solve by its verdict records nothing."""
    stores = []
    best = (False, np.inf, -np.inf if maximize else np.inf)  # (best_quality of a fresh solver)
    for i, rec in enumerate(records):
        if terminates(rec)[0]:
            break
        qc, qa = quality(rec["sides"][CURRENT]), quality(rec["sides"][AVERAGE])
        side = CURRENT if best_of(qc, qa, maximize) == 0 else AVERAGE
        cand = qc if side == CURRENT else qa
        over = cand if best_of(cand, best, maximize) == 0 else best
        if over != best or not stores:
            best = over
            stores.append((i, side))
    return stores


def replay_accepted(records, accept_tolerance, per_constraint=False, save_best_primal_so_far=False, halpern=False):
    """the acceptance set: (index of the record, side) of the FIRST iterate that met the looser tolerances, or None.  Not during the first
    two iterations (total_iterations > 1), not at a major iteration that terminates by its verdict, never again once a point is kept.
    Averaging modes: both iterates are looked at, the KKT score decides when both meet the set (ties to the average), and
    save_best_primal_so_far switches the set off (same snapshot buffers).  Reflected Halpern mode: T(z^k) alone, which lives in the
    average slots (the caller's result then says returned_average = 0)."""
    if save_best_primal_so_far and not halpern:
        return None
    for i, rec in enumerate(records):
        done = rec["iteration"] > 1 and (rec["sides"][AVERAGE]["verdict"] == OPTIMAL if halpern else terminates(rec)[0])
        if done:
            return None
        if rec["iteration"] <= 1:
            continue
        nb, nc = rec["norm_b"], rec["norm_c"]
        aa = accepted_by_looser(rec["sides"][AVERAGE], accept_tolerance, per_constraint, nb, nc)
        if halpern:
            if aa:
                return i, AVERAGE
            continue
        ac = accepted_by_looser(rec["sides"][CURRENT], accept_tolerance, per_constraint, nb, nc)
        if ac and aa:
            w = rec["primal_weight"]
            return i, (CURRENT if kkt_score(rec["sides"][CURRENT], w) < kkt_score(rec["sides"][AVERAGE], w) else AVERAGE)
        if ac or aa:
            return i, (AVERAGE if aa else CURRENT)
    return None


def fill_result(record, side, status, halpern=False):
    """fill_result at the head of `record` for iterate `side`: the fields of a result it sets (the ray fields, zero without detection,
    are left out)"""
    s, c = record["sides"][side], record["counters"]
    return dict(status=status, returned_average=0 if halpern else int(side == AVERAGE), steps_taken=c["steps_taken"], attempted_steps=c["attempted_steps"],
                primal_objective=s["primal_objective"], dual_objective=s["dual_objective"], gap=s["gap"], relative_gap=s["gap"] / (1.0 + s["abs_objective"]),
                l2_primal_residual=s["l2_primal_residual"], l2_dual_residual=s["l2_dual_residual"],
                l2_relative_primal_residual=s["l2_primal_residual"] / (1.0 + record["norm_b"]),
                l2_relative_dual_residual=s["l2_dual_residual"] / (1.0 + record["norm_c"]), step_size=c["step_size"], primal_weight=c["primal_weight"],
                num_restarts=c["num_restarts"], num_major_iterations=c["num_major_iterations"], accepted_at_looser_tolerances=0)


def finish_solve(records, ending_status, save_best_primal_so_far=False, accept_tolerance=None, per_constraint=False, maximize=False, halpern=False):
    """finish_solve at the last record, where `ending_status` ends the solve -> (kept, result).  kept = (index, side) of the point that
    comes back, or None when it is the ending's own: the current iterate of a limit (T(z^k) in Halpern mode), the iterate that
    terminates().  On IterationLimit / TimeLimit the stored point wins: the best primal one with ITS statistics and counters but the final
    num_restarts / num_major_iterations and the ending's status; else the accepted one, additionally with the final steps_taken /
    attempted_steps, status Optimal and accepted_at_looser_tolerances = 1."""
    last = records[-1]
    final = last["counters"]
    limit = ending_status in (ITERATION_LIMIT, TIME_LIMIT)
    stores = replay_best_primal(records, maximize) if save_best_primal_so_far and not halpern else []
    accepted = replay_accepted(records, accept_tolerance, per_constraint, save_best_primal_so_far, halpern) if accept_tolerance is not None else None
    if limit and stores:
        i, side = stores[-1]
        out = fill_result(records[i], side, ending_status)
        out.update(num_restarts=final["num_restarts"], num_major_iterations=final["num_major_iterations"])
        return (i, side), out
    if limit and accepted is not None:
        i, side = accepted
        out = fill_result(records[i], side, OPTIMAL, halpern)
        out.update(num_restarts=final["num_restarts"], num_major_iterations=final["num_major_iterations"], steps_taken=final["steps_taken"],
                   attempted_steps=final["attempted_steps"], accepted_at_looser_tolerances=1)
        return (i, side), out
    if limit:
        return None, fill_result(last, AVERAGE if halpern else CURRENT, ending_status, halpern)
    done, side = (True, AVERAGE) if halpern else terminates(last)
    assert done and ending_status == OPTIMAL, "only the limits and Optimal are restated"
    return None, fill_result(last, side, OPTIMAL, halpern)
