"""GPU: the major iterations of a K-workgroup Halpern batch decided on the device, P periods per host synchronisation --
cuoptamd_batch_set_halpern_device_major, pdlpdev_small_batch_run_halpern_burst, k_pdhg_resident_halpern_burst_batch /
k_major_small_halpern_burst_batch / k_halpern_major_decide_batch / k_halpern_major_restart_batch / k_halpern_major_restart_finish_batch.

The contract is the batch's and the single burst's: every member gets, BIT FOR BIT, what its own Solver(mode=4, halpern_resident=1)
solve with the option at 0 gives it -- status, step / restart / major-iteration counts, step size, primal weight, x, y, reduced costs,
residuals, gap, objectives -- whatever the other members do.  Without the feature every test here fails at set_halpern_device_major."""
import math

import numpy as np
import pytest

from cuopt_amd import capi, synthetic
from test_halpern_device_major_gpu import CASES, EV, bits, head
from test_halpern_gpu import AFIRO, V50, golden
from test_halpern_resident_gpu import lp_only, v50_with_tighter_bounds
from test_halpern_small_batch_gpu import ON, V50_FACTORS, V50_OBJECTIVES, check, halpern_family, solve_alone
from test_small_batch_gpu import LIMIT, perturbed, same

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
REST = 2 ** 31 - 1


@pytest.fixture(scope="module")
def sixty_four(golden_problems):
    """the family of 64 (test_halpern_small_batch_gpu's) and every member's own P = 0 solve, computed once and never modified"""
    problems = halpern_family(golden_problems, 64)
    return problems, [solve_alone(p, tol=1e-6, iteration_limit=LIMIT, **ON) for p in problems]


def batch_of(problems, P, kws=None, **kw):
    solvers = [capi.Solver(p, **(kws[l] if kws else kw), **ON) for l, p in enumerate(problems)]
    for s in solvers:
        assert s.device.layout()["resident"]
    batch = capi.SmallBatch(solvers)
    batch.set_halpern_device_major(P)
    assert batch.halpern_device_major() == P
    return batch, solvers


def close_all(batch, solvers):
    batch.close()
    for s in solvers:
        s.close()


# ---- 1. each member equals its own P = 0 solve ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,P", [(2, 1), (2, 16), (7, 4), (7, 16), (64, 4)])
def test_each_member_equals_its_own_solve_bit_for_bit(sixty_four, K, P):
    problems, want = sixty_four[0][:K], sixty_four[1][:K]
    batch, solvers = batch_of(problems, P, tol=1e-6, iteration_limit=LIMIT)
    assert batch.stats()["tiers"] == (2 if K == 2 else 3)
    got = batch.advance()
    print(K, P, batch.stats(), batch.burst_stats())
    assert len({r["steps_taken"] for r in got}) > 1  # the members finish at different step counts and rest
    assert max(r["num_restarts"] for r in got) >= 1
    assert batch.burst_stats()["bursts"] >= 1
    for l, s in enumerate(solvers):
        check(want[l], got[l], s)
    close_all(batch, solvers)


# ---- 2. one synchronisation per burst --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 4, 16])
def test_one_synchronisation_per_burst(sixty_four, P):
    K = 7
    problems, want = sixty_four[0][:K], sixty_four[1][:K]
    batch, solvers = batch_of(problems, P, tol=1e-6, iteration_limit=LIMIT)  # every member at iteration 0
    before = batch.stats()
    got = batch.advance()
    after, burst = batch.stats(), batch.burst_stats()
    majors = [r["num_major_iterations"] for r in got]
    print(P, "major iterations", majors, before, after, burst)
    assert majors == [w[0]["num_major_iterations"] for w in want]
    assert after["syncs"] - before["syncs"] == math.ceil(max(majors) / P) == burst["bursts"]
    assert after["restart_rounds"] == before["restart_rounds"] and after["periods"] == before["periods"]  # no host-decided round ran
    assert burst["periods"] == P * burst["bursts"] and burst["records"] == sum(majors)
    assert burst["empty_periods"] == sum(P * math.ceil(m / P) - m for m in majors)
    # per period: one evaluation launch, and one loop launch per tier that still has an unfinished member when the burst starts
    tiers = [capi.lib.pdlpdev_resident_tier(s.m, s.n, len(p["values"])) for s, p in zip(solvers, problems)]
    assert sorted(set(tiers)) == [0, 1, 2]
    loops = sum(P * len({t for t, m in zip(tiers, majors) if m > i * P}) for i in range(burst["bursts"]))
    assert after["loop_launches"] - before["loop_launches"] == loops
    assert after["eval_launches"] - before["eval_launches"] == burst["periods"]
    close_all(batch, solvers)


# ---- 3. a member that stops early rests while the others go on -------------------------------------------------------------------------
def test_an_early_member_rests_while_the_others_go_on(golden_problems):
    problems = halpern_family(golden_problems, 4)
    kws = [dict(tol=1e-8, iteration_limit=LIMIT), dict(tol=1e-2, iteration_limit=LIMIT), dict(tol=1e-8, iteration_limit=LIMIT),
           dict(tol=1e-8, iteration_limit=LIMIT)]
    want = [solve_alone(p, **kw, **ON) for p, kw in zip(problems, kws)]
    majors = [w[0]["num_major_iterations"] for w in want]
    assert want[1][0]["status_name"] == "Optimal" and majors[1] == min(majors) and majors[1] < max(majors)  # the early member is early
    batch, solvers = batch_of(problems, 16, kws=kws)
    got = batch.advance()
    burst = batch.burst_stats()
    print(majors, burst, [r["status_name"] for r in got])
    for l, s in enumerate(solvers):  # the early member's result and solution are its own solve's, and so are the others'
        check(want[l], got[l], s)
    # every burst ran 16 periods: a member that stopped at major iteration m of its last burst left the rest of that burst empty
    assert burst["periods"] == 16 * burst["bursts"] and burst["records"] == sum(majors)
    assert burst["empty_periods"] == sum(16 * math.ceil(m / 16) - m for m in majors)
    assert burst["empty_periods"] >= 16 * math.ceil(majors[1] / 16) - majors[1] > 0
    close_all(batch, solvers)


# ---- 4. budgets: burst rounds and host-decided rounds mixed ----------------------------------------------------------------------------
@pytest.mark.parametrize("K,chunks", [(9, (90, 90, 120, REST)), (3, (80, 40, REST))], ids=["inside-periods", "on-periods"])
def test_budgets_resume_where_the_single_solvers_do(golden_problems, K, chunks):
    problems = halpern_family(golden_problems, K)
    want = [solve_alone(p, chunks=chunks, tol=1e-6, iteration_limit=LIMIT, **ON) for p in problems]
    batch, solvers = batch_of(problems, 4, tol=1e-6, iteration_limit=LIMIT)
    for c in chunks:
        got = batch.advance(c)
    st, burst = batch.stats(), batch.burst_stats()
    print(K, chunks, st, burst)
    for l, s in enumerate(solvers):
        check(want[l], got[l], s)
    assert burst["bursts"] >= 1
    if chunks[0] % 40:
        assert st["periods"] >= 1  # (a budget that ends inside a period goes the host-decided way: both kinds of round ran)
    close_all(batch, solvers)


# ---- 5. mixed settings and verdicts ------------------------------------------------------------------------------------------------------
def test_mixed_settings_and_verdicts(golden_problems):
    """the six members of test_halpern_small_batch_gpu.test_mixed_settings_and_verdicts at P = 4"""
    rng = np.random.default_rng(3)
    base = lp_only(golden(V50))
    probe = capi.Solver(base, **ON)
    start = probe.advance(0)  # the step size of the power iteration and the computed weight
    probe.close()
    members = [(base, dict(tol=1e-6, iteration_limit=LIMIT)),
               (perturbed(base, rng), dict(tol=1e-9, iteration_limit=170)),
               (perturbed(base, rng), dict(tol=1e-5, per_constraint_residual=1, iteration_limit=LIMIT)),
               (base, dict(tol=1e-6, iteration_limit=LIMIT, initial_step_size=0.9 * start["initial_step_size"],
                           initial_primal_weight=2.0 * start["initial_primal_weight"])),
               (synthetic.generate(200, 500, 6, seed=6), dict(tol=1e-6, iteration_limit=LIMIT)),
               (lp_only(golden(AFIRO)), dict(tol=1e-8))]
    want = [solve_alone(p, **kw, **ON) for p, kw in members]
    assert want[1][0]["status_name"] == "IterationLimit" and 170 <= want[1][0]["steps_taken"] < 170 + 40  # (inside a burst of four periods)
    assert want[0][0]["status_name"] == "Optimal" and want[5][0]["status_name"] == "Optimal"
    assert want[3][0]["steps_taken"] != want[0][0]["steps_taken"]  # (the given step and weight are what ran)
    batch, solvers = batch_of([p for p, _ in members], 4, kws=[kw for _, kw in members])
    got = batch.advance()
    print(batch.stats(), batch.burst_stats(), [(r["status_name"], r["steps_taken"]) for r in got])
    for l, s in enumerate(solvers):
        check(want[l], got[l], s)
    assert batch.burst_stats()["bursts"] >= 1
    close_all(batch, solvers)


# ---- 6. a step error -----------------------------------------------------------------------------------------------------------------------
def test_a_step_error_ends_one_member_and_leaves_the_others(golden_problems):
    problems = halpern_family(golden_problems, 3)
    kws = [dict(tol=1e-6, iteration_limit=LIMIT), dict(tol=1e-6, iteration_limit=LIMIT, initial_step_size=1e200), dict(tol=1e-6, iteration_limit=LIMIT)]
    want = [solve_alone(p, **kw, **ON) for p, kw in zip(problems, kws)]
    assert want[1][0]["status_name"] == "NumericalError"
    batch, solvers = batch_of(problems, 4, kws=kws)
    got = batch.advance()
    print(batch.stats(), batch.burst_stats(), [(r["status_name"], r["steps_taken"], r["num_major_iterations"]) for r in got])
    assert got[1]["status_name"] == "NumericalError"
    assert (got[1]["steps_taken"], got[1]["num_major_iterations"]) == (want[1][0]["steps_taken"], want[1][0]["num_major_iterations"])
    for l in (0, 2):  # the other members are untouched
        check(want[l], got[l], solvers[l])
    assert batch.burst_stats()["bursts"] >= 1
    close_all(batch, solvers)


# ---- 7. reset and branch rounds -------------------------------------------------------------------------------------------------------------
def test_reset_and_branch_rounds():
    """the three rounds of test_halpern_small_batch_gpu.test_reset_and_branch_rounds at P = 4 against single solvers with the option at 0"""
    variants = [lp_only(v50_with_tighter_bounds(f)) for f in V50_FACTORS]
    K, kw = 4, dict(tol=1e-5, iteration_limit=20000)
    ones = [capi.Solver(variants[l], **kw, **ON) for l in range(K)]
    many = [capi.Solver(variants[l], **kw, **ON) for l in range(K)]
    batch = capi.SmallBatch(many)
    batch.set_halpern_device_major(4)

    def compare(want, got, known):
        sols = batch.solutions()
        for l in range(K):
            same(dict(want[l][0], setup_seconds=0), dict(got[l], setup_seconds=0))  # (steps, restarts, verdict, residuals, objectives)
            assert got[l]["status_name"] == "Optimal"
            for u, v, w in zip(want[l][1], sols[l], many[l].solution()):
                np.testing.assert_array_equal(u, v)
                np.testing.assert_array_equal(u, w)
            assert abs(got[l]["primal_objective"] - known[l]) <= 2e-4 * (1.0 + abs(known[l])), (l, got[l]["primal_objective"], known[l])
        return sols

    prev = None
    for r in range(3):
        which = [(l + r) % K for l in range(K)]  # member l takes variant l + r
        lbs = [np.array(variants[v]["lb"], float) for v in which]
        ubs = [np.array(variants[v]["ub"], float) for v in which]
        want = []
        for l, s in enumerate(ones):
            s.reset(lb=lbs[l], ub=ubs[l], init_x=None if prev is None else prev[l][0], init_y=None if prev is None else prev[l][1])
            want.append((s.advance(), s.solution()))
        batch.reset(lb=lbs, ub=ubs, init_x=None if prev is None else [v[0] for v in prev], init_y=None if prev is None else [v[1] for v in prev])
        bursts = batch.burst_stats()["bursts"]
        sols = compare(want, batch.advance(), [V50_OBJECTIVES[v] for v in which])
        assert batch.halpern_device_major() == 4 and batch.burst_stats()["bursts"] > bursts  # (a reset keeps the option)
        # a branch that keeps the optimum: the upper bound of the variable that sits farthest inside its range moves half way towards
        # the point (members 0 .. 2); member 3 is re-solved as it is
        var, lo, hi = np.full(K, -1, np.int32), np.zeros(K), np.zeros(K)
        for l in range(K - 1):
            x = sols[l][0]
            room = np.where(np.isfinite(lbs[l]) & np.isfinite(ubs[l]), np.minimum(x - lbs[l], ubs[l] - x), -1.0)
            j = int(np.argmax(room))
            assert room[j] > 1e-3
            ubs[l][j] = 0.5 * (x[j] + ubs[l][j])
            var[l], lo[l], hi[l] = j, lbs[l][j], ubs[l][j]
        want2 = []
        for l, s in enumerate(ones):
            s.reset(lb=lbs[l], ub=ubs[l], init_x=want[l][1][0], init_y=want[l][1][1])  # (from the single solver's own returned point)
            want2.append((s.advance(), s.solution()))
        batch.branch(var, lo, hi)
        bursts = batch.burst_stats()["bursts"]
        prev = compare(want2, batch.advance(), [V50_OBJECTIVES[v] for v in which])
        assert batch.burst_stats()["bursts"] > bursts
    st = batch.stats()
    assert st["resets"] == 6 and st["restart_rounds"] == 0  # (every restart was the device's)
    close_all(batch, ones + many)


# ---- 8. the decision kernel: N cases as the N members of one launch ------------------------------------------------------------------------
def test_the_batched_decision_kernel_against_the_float64_restatement():
    """CASES of test_halpern_device_major_gpu.py, each as a member with state, parameters and sums of its own (workgroup w serves member
    N - 1 - w), against that file's restatement `head`: a member that read a neighbour's block would get the neighbour's verdict"""
    n = len(CASES)
    evs, ctls, hals, r_prevs, pars, targets, stops, records = [], [], [], [], [], [], [], []
    for i, (label, ev, steps, error, r, r_first, k, r_prev, P, target, stopped) in enumerate(CASES):
        ctl, hal = capi.Ctl(), capi.Halpern()
        ctl.steps_taken, ctl.attempts, ctl.error, ctl.primal_weight, ctl.step_size, ctl.target_steps = steps, steps, error, 1.75 + i, 0.01, target
        hal.r, hal.r_first, hal.k = r, r_first, k
        before = capi.HalpernMajorRecord()
        before.steps_taken, before.verdict, before.restart, before.r, before.new_weight = -7, 99, 5, 123.0 + i, 4.5  # (what a stopped member must keep)
        evs.append(list(ev)), ctls.append(ctl), hals.append(hal), r_prevs.append(r_prev), pars.append(P), targets.append(target)
        stops.append(stopped), records.append(before)
    recs, r_prev_out, stopped_out, restart_out = capi.debug_halpern_major_decide_batch(evs, ctls, hals, r_prevs, pars, targets, stops, records)
    verdicts = set()
    for i, (label, ev, steps, error, r, r_first, k, r_prev, P, target, stopped) in enumerate(CASES):
        rec = recs[i]
        ev_seen = list(ev)
        if not P.want_linf:
            ev_seen[EV["LINF_P"]] = ev_seen[EV["LINF_D"]] = 0.0
        want = head(ev_seen, steps, error, r, r_first, k, r_prev, P, target, stopped)
        print(label, "verdict", rec.verdict, "restart", rec.restart, "r_prev", r_prev_out[i], "stopped", stopped_out[i], "want", want)
        if want is None:  # the member has stopped: nothing may change
            assert (rec.steps_taken, rec.verdict, rec.restart, rec.r, rec.new_weight) == (-7, 99, 5, 123.0 + i, 4.5), label
            assert bits(r_prev_out[i]) == bits(r_prev) and stopped_out[i] == 1 and restart_out[i] == 0, label
            continue
        verdict, restart, r_prev_want, stopped_want = want
        verdicts.add((verdict, restart))
        assert (rec.verdict, rec.restart, stopped_out[i], restart_out[i]) == (verdict, restart, stopped_want, restart), label
        assert bits(r_prev_out[i]) == bits(r_prev_want), label
        assert (rec.steps_taken, rec.k) == (steps, k) and bits(rec.r) == bits(r) and bits(rec.r_first) == bits(r_first), label
        assert rec.primal_weight == 1.75 + i and list(rec.dist) == [0.0, 0.0] and rec.new_weight == 0.0, label  # (its OWN control block)
        if verdict in (capi.MAJOR_STEP_ERROR, capi.MAJOR_FELL_SHORT):
            assert list(rec.ev) == [0.0] * 8, label
        else:
            np.testing.assert_array_equal(bits(list(rec.ev)), bits(ev_seen))
    assert len(verdicts) >= 5 and n >= 40  # (go on with and without a restart, optimal, the limit, step error / fell short)


# ---- 9. refusals and the way back --------------------------------------------------------------------------------------------------------------
def refused(batch, P, code):
    with pytest.raises(capi.CuOptError) as e:
        batch.set_halpern_device_major(P)
    assert e.value.code == code and "halpern_device_major" in str(e.value), str(e.value)
    return str(e.value)


def test_other_batches_are_refused_by_name(monkeypatch):
    small = lp_only(golden(AFIRO))
    averaging = [capi.Solver(small) for _ in range(2)]
    batch = capi.SmallBatch(averaging)  # an averaging small-LP batch
    refused(batch, 4, -7)
    assert batch.halpern_device_major() == 0
    assert [r["status_name"] for r in batch.advance()] == ["Optimal"] * 2
    close_all(batch, averaging)
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    q = synthetic.generate(3000, 3000, 6)
    for kw in (dict(), dict(mode=4, halpern_lockstep=1)):  # either lockstep batch
        parent = capi.Solver(q, tol=0.0, **kw)
        child = parent.clone()
        batch = capi.SharedMatrixBatch([parent, child])
        refused(batch, 4, -7)
        refused(batch, 17, -1)
        assert batch.halpern_device_major() == 0
        assert [r["steps_taken"] for r in batch.advance(40)] == [40, 40]  # ... and the batch advances as before
        close_all(batch, [child, parent])


def test_out_of_range_and_refused_members_leave_the_batch_as_it_was(golden_problems):
    problems = halpern_family(golden_problems, 2)
    want = [solve_alone(p, tol=1e-6, iteration_limit=LIMIT, **ON) for p in problems]
    batch, solvers = batch_of(problems, 4, tol=1e-6, iteration_limit=LIMIT)
    for bad in (-1, 17):
        refused(batch, bad, -1)
        assert batch.halpern_device_major() == 4  # the getter still returns the old P
    got = batch.advance()  # ... and the batch solves, in bursts
    for l, s in enumerate(solvers):
        check(want[l], got[l], s)
    assert batch.burst_stats()["bursts"] >= 1
    close_all(batch, solvers)
    for kw in (dict(halpern_infeasibility=1), dict(accept_enabled=1)):
        kws = [dict(tol=1e-6, iteration_limit=LIMIT), dict(tol=1e-6, iteration_limit=LIMIT, **kw)]
        solvers = [capi.Solver(p, **k, **ON) for p, k in zip(problems, kws)]
        batch = capi.SmallBatch(solvers)
        assert ("halpern_infeasibility" if "halpern_infeasibility" in kw else "accept") in refused(batch, 4, -7)
        assert batch.halpern_device_major() == 0
        alone = [solve_alone(p, **k, **ON) for p, k in zip(problems, kws)]
        got = batch.advance()  # the refused call left the batch as it was: the host-decided round
        for l, s in enumerate(solvers):
            check(alone[l], got[l], s)
        assert batch.burst_stats()["bursts"] == 0
        close_all(batch, solvers)


def test_zero_restores_the_host_decided_round(golden_problems):
    problems = halpern_family(golden_problems, 3)
    stats = []
    for touch in (False, True):
        solvers = [capi.Solver(p, tol=1e-6, iteration_limit=LIMIT, **ON) for p in problems]
        batch = capi.SmallBatch(solvers)
        if touch:
            batch.set_halpern_device_major(8)
            batch.set_halpern_device_major(0)
        assert batch.halpern_device_major() == 0
        got = batch.advance()
        stats.append((batch.stats(), batch.burst_stats(), [(r["status"], r["steps_taken"], r["num_restarts"]) for r in got]))
        close_all(batch, solvers)
    print(stats)
    assert stats[0][0]["syncs"] == stats[1][0]["syncs"] and stats[0][0] == stats[1][0]  # the same synchronisations as a batch that never set it
    assert stats[1][1]["bursts"] == 0 and stats[0][2] == stats[1][2]
