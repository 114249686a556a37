"""CPU: tests/kept_point_reference.py on hand-written records, one per branch of the rules it restates (pdlp_solver.cpp: best_of and the
recording rule of major_head, accepted_by_looser in both residual modes, keep_accepted_point in both iterations, finish_solve)."""
import numpy as np
import pytest

import kept_point_reference as kr
from kept_point_reference import AVERAGE, CURRENT, ITERATION_LIMIT, NO_VERDICT, OPTIMAL, PRIMAL_FEASIBLE, TIME_LIMIT


def side(pres=1.0, dres=1.0, pobj=0.0, dobj=0.0, verdict=NO_VERDICT, linf_p=0.0, linf_d=0.0):
    return dict(verdict=verdict, primal_objective=pobj, dual_objective=dobj, gap=abs(pobj - dobj), abs_objective=abs(pobj) + abs(dobj),
                l2_primal_residual=pres, l2_dual_residual=dres, linf_rel_primal_residual=linf_p, linf_rel_dual_residual=linf_d)


def record(it, cur, avg, w=1.0, restarts=0):
    """major iterations at 0, 1, 40, 80, ...: counters that tell the records apart"""
    return dict(iteration=it, primal_weight=w, norm_b=3.0, norm_c=4.0, sides={CURRENT: cur, AVERAGE: avg},
                counters=dict(steps_taken=it, attempted_steps=it + 2, step_size=0.5 + it, primal_weight=w, num_restarts=restarts,
                              num_major_iterations=1 + it // 40 + (it > 0)))


def test_to_convergence_and_verdict():
    ev = [3.0, 1.0, 16.0, 9.0, 0.0, 0.0, 0.25, 0.5]
    c = kr.to_convergence(ev)
    assert (c["primal_objective"], c["dual_objective"], c["gap"], c["abs_objective"]) == (3.0, 1.0, 2.0, 4.0)
    assert (c["l2_primal_residual"], c["l2_dual_residual"], c["linf_rel_primal_residual"], c["linf_rel_dual_residual"]) == (4.0, 3.0, 0.25, 0.5)
    m = kr.to_convergence(ev, objective_scale=-1.0, objective_offset=10.0)  # a maximisation with an offset
    assert (m["primal_objective"], m["dual_objective"], m["gap"], m["abs_objective"]) == (7.0, 9.0, 2.0, 16.0)
    # l2 mode: eps_abs + eps_rel * norm; gap: eps_abs + eps_rel * (|p| + |d|)
    assert kr.verdict(c, [0.0, 0.5, 1.0, 1.0, 0.0, 0.75], False, 3.0, 4.0) == OPTIMAL  # 2 <= 2, 4 <= 4, 3 <= 3: equality meets
    assert kr.verdict(c, [0.0, 0.49, 1.0, 1.0, 0.0, 0.75], False, 3.0, 4.0) == PRIMAL_FEASIBLE
    assert kr.verdict(c, [0.0, 0.5, 0.9, 1.0, 0.0, 0.75], False, 3.0, 4.0) == NO_VERDICT
    # per-constraint mode: the l-infinity figures against the ABSOLUTE tolerances, the norms play no part
    assert kr.verdict(c, [2.0, 0.0, 0.25, 9.0, 0.5, 9.0], True, 3.0, 4.0) == OPTIMAL
    assert kr.verdict(c, [2.0, 0.0, 0.24, 9.0, 0.5, 9.0], True, 3.0, 4.0) == NO_VERDICT
    assert kr.verdict(c, [2.0, 0.0, 0.25, 9.0, 0.49, 9.0], True, 3.0, 4.0) == PRIMAL_FEASIBLE


def test_kkt_score():
    s = side(pres=3.0, dres=8.0, pobj=5.0, dobj=5.0 - 12.0)
    assert kr.kkt_score(s, 2.0) == float(np.sqrt(4.0 * 9.0 + 64.0 / 4.0 + 144.0))


def test_best_of():
    feas, infeas = (True, 5.0, 1.0), (False, 0.1, -9.0)
    assert kr.best_of(feas, infeas, False) == 0 and kr.best_of(infeas, feas, False) == 1  # feasible beats infeasible, whatever the rest
    lo, hi = (True, 5.0, 1.0), (True, 0.0, 2.0)
    assert kr.best_of(lo, hi, False) == 0 and kr.best_of(hi, lo, False) == 1  # two feasible ones: the objective, not the residual
    assert kr.best_of(lo, hi, True) == 1 and kr.best_of(hi, lo, True) == 0    # maximize flips it
    assert kr.best_of(lo, lo, False) == 1 and kr.best_of(lo, lo, True) == 0   # equal objectives: b when minimising, a when maximising
    a, b = (False, 1.0, 0.0), (False, 2.0, -5.0)
    assert kr.best_of(a, b, False) == 0 and kr.best_of(b, a, True) == 1 and kr.best_of(a, a, False) == 1  # else the least residual


def test_best_primal_recording_rule():
    recs = [record(0, side(pres=9.0), side(pres=9.0)),    # the first record always stores; equal iterates: the average
            record(1, side(pres=7.0), side(pres=8.0)),    # the current iterate is better and beats the stored point
            record(40, side(pres=7.5), side(pres=7.0)),   # equal quality (same residual AND objective as the stored point) does not replace
            record(80, side(pres=6.0), side(pres=5.0)),   # the average
            record(120, side(pres=6.0, pobj=3.0, verdict=PRIMAL_FEASIBLE), side(pres=0.1)),  # feasible beats the lower residual
            record(160, side(pres=0.0, pobj=4.0, verdict=PRIMAL_FEASIBLE), side(pres=0.0, pobj=2.0, verdict=PRIMAL_FEASIBLE)),
            record(200, side(pres=0.0, pobj=2.0, verdict=PRIMAL_FEASIBLE), side(pres=9.0))]  # equal objective: stays (minimising)
    assert kr.replay_best_primal(recs) == [(0, AVERAGE), (1, CURRENT), (3, AVERAGE), (4, CURRENT), (5, AVERAGE)]
    # the maximize flip: among feasible points the HIGHER objective wins, so 160 takes its current iterate and 200 changes nothing ...
    assert kr.replay_best_primal(recs, maximize=True) == [(0, AVERAGE), (1, CURRENT), (3, AVERAGE), (4, CURRENT), (5, CURRENT)]
    # ... and an equal objective with another residual does replace when maximising (best_of answers the candidate, which differs)
    recs[6] = record(200, side(pres=0.5, pobj=4.0, verdict=PRIMAL_FEASIBLE), side(pres=9.0))
    assert kr.replay_best_primal(recs, maximize=True)[-1] == (6, CURRENT) and kr.replay_best_primal(recs[:6] + [record(200, side(pres=0.5, pobj=2.0, verdict=PRIMAL_FEASIBLE), side(pres=9.0))])[-1] == (5, AVERAGE)
    # a major iteration that terminates by its verdict records nothing
    recs.append(record(240, side(verdict=OPTIMAL, pres=0.0, pobj=-1.0), side(pres=0.0, pobj=-2.0, verdict=PRIMAL_FEASIBLE)))
    assert kr.replay_best_primal(recs)[-1][0] < 7


LOOSE = [1.0, 0.0, 1.0, 0.0, 1.0, 0.0]  # (absolute only: gap, primal, dual <= 1)


def test_acceptance_set():
    ok, no = side(pres=0.5, dres=0.5), side(pres=2.0, dres=0.5)
    # met at iteration 1 already: ignored (total_iterations > 1); then the first acceptance only
    recs = [record(0, ok, ok), record(1, ok, ok), record(40, no, no), record(80, ok, no), record(120, no, ok)]
    assert kr.replay_accepted(recs, LOOSE) == (3, CURRENT)
    assert kr.replay_accepted(recs[:3], LOOSE) is None
    assert kr.replay_accepted([recs[2], record(80, no, ok)], LOOSE) == (1, AVERAGE)
    # both iterates meet the set: the KKT score decides (weight 2: 4 p^2 + d^2 / 4), ties to the average
    p_heavy, d_heavy = side(pres=0.9, dres=0.1), side(pres=0.1, dres=0.9)
    assert kr.replay_accepted([record(40, p_heavy, d_heavy, w=2.0)], LOOSE) == (0, AVERAGE)
    assert kr.replay_accepted([record(40, d_heavy, p_heavy, w=2.0)], LOOSE) == (0, CURRENT)
    assert kr.replay_accepted([record(40, d_heavy, p_heavy, w=0.5)], LOOSE) == (0, AVERAGE)
    assert kr.replay_accepted([record(40, ok, ok)], LOOSE) == (0, AVERAGE)
    # relative parts: eps_rel * norm_b (3), norm_c (4), |p| + |d|
    rel, no = side(pres=3.0, dres=4.0, pobj=2.0, dobj=1.0), side(pres=99.0, dres=99.0)
    assert kr.replay_accepted([record(40, rel, no)], [0.0, 1.0 / 3.0, 0.0, 1.0, 0.0, 1.0]) == (0, CURRENT)
    assert kr.replay_accepted([record(40, rel, no)], [0.0, 0.33, 0.0, 1.0, 0.0, 1.0]) is None
    assert kr.replay_accepted([record(40, rel, no)], [0.0, 0.34, 0.0, 0.99, 0.0, 1.0]) is None
    # per-constraint residuals: the l-infinity figures against a[2] and a[4]; the l2 residuals play no part
    pc, no = side(pres=50.0, dres=50.0, linf_p=0.5, linf_d=0.25), side(pres=99.0, dres=99.0, linf_p=9.0, linf_d=9.0)
    assert kr.replay_accepted([record(40, pc, no)], [1.0, 0.0, 0.5, 0.0, 0.25, 0.0], per_constraint=True) == (0, CURRENT)
    assert kr.replay_accepted([record(40, pc, no)], [1.0, 0.0, 0.5, 9.0, 0.24, 9.0], per_constraint=True) is None
    assert kr.replay_accepted([record(40, pc, no)], LOOSE) is None
    # save_best_primal_so_far switches the set off in the averaging modes
    assert kr.replay_accepted(recs, LOOSE, save_best_primal_so_far=True) is None
    # a major iteration that terminates by its verdict keeps nothing
    assert kr.replay_accepted([record(40, side(pres=0.5, dres=0.5, verdict=OPTIMAL), ok)], LOOSE) is None


def test_acceptance_set_of_the_halpern_mode():
    ok, no = side(pres=0.5, dres=0.5), side(pres=2.0, dres=0.5)
    # only T(z^k), which lives in the average slots: a current side that meets the set counts for nothing
    recs = [record(40, ok, no), record(80, ok, ok), record(120, ok, ok)]
    assert kr.replay_accepted(recs, LOOSE, halpern=True) == (1, AVERAGE)
    assert kr.replay_accepted(recs[:1], LOOSE, halpern=True) is None
    kept, res = kr.finish_solve(recs, ITERATION_LIMIT, accept_tolerance=LOOSE, halpern=True)
    assert kept == (1, AVERAGE) and res["returned_average"] == 0 and res["status"] == OPTIMAL and res["accepted_at_looser_tolerances"] == 1
    kept, res = kr.finish_solve(recs[:1], ITERATION_LIMIT, accept_tolerance=LOOSE, halpern=True)
    assert kept is None and res["returned_average"] == 0 and res["status"] == ITERATION_LIMIT and res["l2_primal_residual"] == 2.0


def test_finish_solve():
    recs = [record(0, side(pres=9.0, pobj=1.0), side(pres=9.0, pobj=1.0)), record(40, side(pres=2.0, pobj=5.0, dobj=4.0), side(pres=0.5, dres=0.25, pobj=7.0, dobj=3.0), restarts=1),
            record(80, side(pres=3.0, pobj=6.0), side(pres=4.0), restarts=2), record(120, side(pres=8.0, pobj=-1.0), side(pres=6.0), restarts=3)]
    final = recs[-1]["counters"]
    # best primal: the stored point's statistics AND counters, but the final restarts / major iterations and the ending's status
    for status in (ITERATION_LIMIT, TIME_LIMIT):
        kept, res = kr.finish_solve(recs, status, save_best_primal_so_far=True, accept_tolerance=LOOSE)
        assert kept == (1, AVERAGE) and res["status"] == status and res["returned_average"] == 1 and res["accepted_at_looser_tolerances"] == 0
        assert (res["steps_taken"], res["attempted_steps"], res["step_size"]) == (40, 42, 40.5)
        assert (res["num_restarts"], res["num_major_iterations"]) == (final["num_restarts"], final["num_major_iterations"]) == (3, 5)
        assert (res["primal_objective"], res["dual_objective"], res["gap"], res["relative_gap"]) == (7.0, 3.0, 4.0, 4.0 / 11.0)
        assert (res["l2_primal_residual"], res["l2_relative_primal_residual"], res["l2_relative_dual_residual"]) == (0.5, 0.5 / 4.0, 0.25 / 5.0)
    # the acceptance set: additionally the final steps, status Optimal, the flag
    kept, res = kr.finish_solve(recs, ITERATION_LIMIT, accept_tolerance=[4.0, 0.0, 1.0, 0.0, 1.0, 0.0])
    assert kept == (1, AVERAGE) and res["status"] == OPTIMAL and res["accepted_at_looser_tolerances"] == 1 and res["returned_average"] == 1
    assert (res["steps_taken"], res["attempted_steps"], res["step_size"]) == (120, 122, 40.5)
    assert (res["num_restarts"], res["num_major_iterations"], res["primal_objective"]) == (3, 5, 7.0)
    # nothing kept: the limit's own point, the current iterate of the last major iteration
    kept, res = kr.finish_solve(recs, ITERATION_LIMIT, accept_tolerance=[0.0] * 6)
    assert kept is None and res["status"] == ITERATION_LIMIT and res["returned_average"] == 0 and (res["l2_primal_residual"], res["primal_objective"], res["steps_taken"]) == (8.0, -1.0, 120)
    kept, res = kr.finish_solve(recs, ITERATION_LIMIT)
    assert kept is None and res["l2_primal_residual"] == 8.0
    # any other ending returns the ending's own point, whatever is stored
    recs.append(record(160, side(pres=0.0, verdict=PRIMAL_FEASIBLE), side(pres=0.0, pobj=2.0, dobj=2.0, verdict=OPTIMAL), restarts=3))
    for kw in (dict(save_best_primal_so_far=True), dict(accept_tolerance=[4.0, 0.0, 1.0, 0.0, 1.0, 0.0])):
        kept, res = kr.finish_solve(recs, OPTIMAL, **kw)
        assert kept is None and res["status"] == OPTIMAL and res["returned_average"] == 1 and res["steps_taken"] == 160 and res["accepted_at_looser_tolerances"] == 0
    with pytest.raises(AssertionError):
        kr.finish_solve(recs[:4], OPTIMAL)
