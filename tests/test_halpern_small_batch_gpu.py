"""GPU: K LPs in reflected Halpern mode (solver mode 4, halpern_resident) in K workgroups of one launch -- cuoptamd_settings::halpern_batch,
pdlpdev_small_batch_create_halpern, k_pdhg_resident_halpern_batch / k_major_small_halpern_batch / k_halpern_restart_finish_batch.  The
contract is the averaging batch's (test_small_batch_gpu.py): every member gets, BIT FOR BIT, what its own
Solver(mode=4, halpern_resident=1).advance gives it -- results, iterates, verdicts, restart counts -- whatever the other members do."""
import ctypes as C
import time

import numpy as np
import pytest

from cuopt_amd import capi, synthetic
from cuopt_amd import linear_programming as lp
from test_halpern_gpu import AFIRO, COD, V50, golden
from test_halpern_resident_gpu import SUDOKU, lp_only, v50_with_tighter_bounds
from test_small_batch_gpu import LIMIT, family, perturbed, same

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ON = dict(mode=4, halpern_resident=1, halpern_batch=1)
# HiGHS on the host (test_halpern_resident_gpu.v50_with_tighter_bounds): the optimal objectives of 50v-10 at these factors
V50_FACTORS = (0.008, 0.006, 0.005, 0.004)
V50_OBJECTIVES = (2914.46, 2956.71, 3047.79, 3253.94)


def halpern_family(golden_problems, count, seed=1):
    """test_small_batch_gpu.family's four matrices and three tiers plus sudoku (tier 1), 2048 x 2048 x 2 (the edge of the largest tier)
    and 40 x 30 x 5, then perturbed copies.  One seed: the families of 2 and 7 are the first members of the family of 64."""
    rng = np.random.default_rng(seed)
    base = family(golden_problems, 6) + [lp_only(golden(SUDOKU)), synthetic.generate(2048, 2048, 2, seed=7), synthetic.generate(40, 30, 5, seed=8)]
    return [base[i % len(base)] if i < len(base) else perturbed(base[i % len(base)], rng) for i in range(count)]


def solve_alone(p, chunks=(2 ** 31 - 1,), **kw):
    s = capi.Solver(p, **kw)
    assert s.device.layout()["resident"], s.device.layout()
    r = None
    for c in chunks:
        r = s.advance(c)
    out = (r, s.solution())
    s.close()
    return out


def check(want, got, solver):
    same(want[0], got)
    for u, v in zip(want[1], solver.solution()):  # x, y, reduced costs
        np.testing.assert_array_equal(u, v)


@pytest.fixture(scope="module")
def sixty_four(golden_problems):
    """the family of 64 and every member's own solve, computed once for the three batch sizes"""
    problems = halpern_family(golden_problems, 64)
    return problems, [solve_alone(p, tol=1e-6, iteration_limit=LIMIT, **ON) for p in problems]


# ---- 1. each member gets its own solve --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 7, 64])
def test_each_member_gets_its_own_solve_bit_for_bit(sixty_four, K):
    problems, want = sixty_four[0][:K], sixty_four[1][:K]
    solvers = [capi.Solver(p, tol=1e-6, iteration_limit=LIMIT, **ON) for p in problems]
    for s in solvers:
        assert s.device.layout()["resident"]
    batch = capi.SmallBatch(solvers)
    assert batch.stats()["halpern"] == 1 and batch.stats()["tiers"] == (2 if K == 2 else 3)
    got = batch.advance()
    assert len({r["steps_taken"] for r in got}) > 1  # the members finish at different step counts and rest
    assert max(r["num_restarts"] for r in got) >= 1
    for l, s in enumerate(solvers):
        check(want[l], got[l], s)
    batch.close()
    for s in solvers:
        s.close()


# ---- 2. budgets ---------------------------------------------------------------------------------------------------------------------------
def test_budgets_resume_where_they_stopped(golden_problems):
    """pieces of (90, 90, 120, rest), test_small_batch_gpu's: budgets end inside periods, some right after a restart; every piece ends
    where the single solver's does"""
    problems = halpern_family(golden_problems, 9)
    chunks = (90, 90, 120, 2 ** 31 - 1)
    want = [solve_alone(p, chunks=chunks, tol=1e-6, iteration_limit=LIMIT, **ON) for p in problems]
    solvers = [capi.Solver(p, tol=1e-6, iteration_limit=LIMIT, **ON) for p in problems]
    batch = capi.SmallBatch(solvers)
    for c in chunks:
        got = batch.advance(c)
    for l, s in enumerate(solvers):
        check(want[l], got[l], s)
    batch.close()


def test_budgets_that_end_on_a_period(golden_problems):
    """pieces of 80 and 40 steps end exactly where a major iteration is due: the evaluation behind the steps is the one the next call uses"""
    problems = halpern_family(golden_problems, 3)
    chunks = (80, 40, 2 ** 31 - 1)
    want = [solve_alone(p, chunks=chunks, tol=1e-6, iteration_limit=LIMIT, **ON) for p in problems]
    solvers = [capi.Solver(p, tol=1e-6, iteration_limit=LIMIT, **ON) for p in problems]
    batch = capi.SmallBatch(solvers)
    for c in chunks:
        got = batch.advance(c)
    for l, s in enumerate(solvers):
        check(want[l], got[l], s)
    batch.close()


# ---- 3. mixed settings and verdicts ---------------------------------------------------------------------------------------------------------
def test_mixed_settings_and_verdicts(golden_problems):
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
    assert want[1][0]["status_name"] == "IterationLimit" and 170 <= want[1][0]["steps_taken"] < 170 + 40  # (the limit is looked at once a period)
    assert want[0][0]["status_name"] == "Optimal" and want[5][0]["status_name"] == "Optimal"
    assert want[3][0]["steps_taken"] != want[0][0]["steps_taken"]  # (the given step and weight are what ran)
    solvers = [capi.Solver(p, **kw, **ON) for p, kw in members]
    batch = capi.SmallBatch(solvers)
    got = batch.advance()
    for l, s in enumerate(solvers):
        check(want[l], got[l], s)
    batch.close()


# ---- 4. reset and branch rounds -------------------------------------------------------------------------------------------------------------
def test_reset_and_branch_rounds():
    """three rounds of batch.reset (other bounds, the previous primal / dual as the start) and batch.branch (one variable's bounds, the
    start from the member's own returned point, all on the device) against Solver.reset of single solvers"""
    variants = [lp_only(v50_with_tighter_bounds(f)) for f in V50_FACTORS]
    K, kw = 4, dict(tol=1e-5, iteration_limit=20000)
    ones = [capi.Solver(variants[l], **kw, **ON) for l in range(K)]
    many = [capi.Solver(variants[l], **kw, **ON) for l in range(K)]
    batch = capi.SmallBatch(many)

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
        sols = compare(want, batch.advance(), [V50_OBJECTIVES[v] for v in which])
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
        prev = compare(want2, batch.advance(), [V50_OBJECTIVES[v] for v in which])
    assert batch.stats()["resets"] == 6
    batch.close()


# ---- 5. one synchronisation per period ------------------------------------------------------------------------------------------------------
def test_one_synchronisation_per_period(golden_problems):
    problems = halpern_family(golden_problems, 8)
    solvers = [capi.Solver(p, tol=0.0, **ON) for p in problems]
    batch = capi.SmallBatch(solvers)
    batch.reset()  # (the anchors of the start: the "1 +" of the single solver's count)
    got = batch.advance(400)
    assert [r["steps_taken"] for r in got] == [400] * 8
    st = batch.stats()
    print(st)
    periods = 400 // 40
    assert st["halpern"] == 1 and st["tiers"] == 3 and st["periods"] == periods
    assert st["loop_launches"] == st["tiers"] * periods and st["eval_launches"] == periods
    assert max(r["num_restarts"] for r in got) <= st["restart_rounds"] <= periods  # (a round serves every member that restarts then)
    assert st["resets"] == 1 and st["syncs"] == 1 + st["restart_rounds"] + periods
    batch.close()


# ---- 6. what is refused, and what stays -------------------------------------------------------------------------------------------------------
def test_refusals():
    small = lp_only(golden(AFIRO))
    plain = [capi.Solver(small, mode=4, halpern_resident=1) for _ in range(2)]  # without the option
    with pytest.raises(capi.CuOptError) as e:
        capi.SharedMatrixBatch(plain)
    assert e.value.code == -7 and "Halpern" in str(e.value)
    opted = [capi.Solver(small, **ON) for _ in range(2)]
    averaging = capi.Solver(small)
    for mix in ([opted[0], averaging], [averaging, opted[0]], [opted[0], plain[0]]):
        with pytest.raises(capi.CuOptError) as e:
            capi.SmallBatch(mix)
        assert e.value.code == -7 and "Halpern" in str(e.value)
    for big in (golden(COD), synthetic.generate(3000, 3000, 6, seed=2)):  # not of resident size: the multi-launch kernels run the mode
        b = capi.Solver(lp_only(big), **ON)
        assert not b.device.layout()["resident"]
        with pytest.raises(capi.CuOptError) as e:
            capi.SmallBatch([opted[0], b])
        assert e.value.code == -7 and "resident" in str(e.value)
        b.close()
    ctx = (C.c_void_p * 2)(*[s.device.handle for s in opted])
    out = C.c_void_p()
    rc = capi.lib.pdlpdev_small_batch_create(C.byref(out), ctx, 2)  # the averaging batch's entry point refuses them with or without it
    assert rc == -7 and "Halpern" in capi.lib.pdlpdev_last_error().decode() and not out.value
    want = solve_alone(small, **ON)
    for s in plain + opted:  # every solver stays usable
        r = s.advance()
        same(want[0], r)
        s.close()
    assert averaging.advance()["status_name"] == "Optimal"
    averaging.close()


# ---- 7. the public paths ------------------------------------------------------------------------------------------------------------------------
def test_public_paths():
    variants = [lp_only(v50_with_tighter_bounds(f)) for f in V50_FACTORS]
    want = [solve_alone(q, **ON) for q in variants]
    assert [w[0]["status_name"] for w in want] == ["Optimal"] * 4
    res = capi.batch_solve(variants, **ON)
    assert capi.batch_solve_last_path() == "small_halpern"
    for r, w in zip(res, want):
        for k in ("status", "steps_taken", "num_restarts", "num_major_iterations", "primal_objective", "dual_objective"):
            assert r[k] == w[0][k], k
        for u, v in zip(w[1], (r["x"], r["y"], r["reduced_cost"])):
            np.testing.assert_array_equal(u, v)
    off = capi.batch_solve(variants, mode=4, halpern_resident=1)  # without the option: one resident loop after the other, as before
    assert capi.batch_solve_last_path() == "independent"
    for r, w in zip(off, want):
        assert r["steps_taken"] == w[0]["steps_taken"]
        np.testing.assert_array_equal(r["x"], w[1][0])
    capi.batch_solve(variants)  # (the averaging iteration's batch keeps its path)
    assert capi.batch_solve_last_path() == "small"
    settings = lp.SolverSettings()
    assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_BATCH) == 0
    settings.set_parameter(lp.CUOPT_PDLP_SOLVER_MODE, lp.PDLPSolverMode.Halpern1)
    settings.set_parameter(lp.CUOPT_AMD_HALPERN_RESIDENT, 1)
    settings.set_parameter(lp.CUOPT_AMD_HALPERN_BATCH, 1)
    assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_BATCH) == 1
    models = []
    for p in variants:
        dm = lp.DataModel()
        dm.set_csr_constraint_matrix(p["values"], p["indices"], p["offsets"])
        dm.set_objective_coefficients(p["c"])
        dm.set_constraint_lower_bounds(p["lo"])
        dm.set_constraint_upper_bounds(p["hi"])
        dm.set_variable_lower_bounds(p["lb"])
        dm.set_variable_upper_bounds(p["ub"])
        dm.set_maximize(p.get("maximize", False))
        dm.set_objective_offset(p.get("objective_offset", 0.0))
        models.append(dm)
    sols, _ = lp.BatchSolve(models, settings)
    assert capi.batch_solve_last_path() == "small_halpern"
    assert [s.get_termination_reason() for s in sols] == ["Optimal"] * 4
    assert [s.get_lp_stats()["nb_iterations"] for s in sols] == [w[0]["steps_taken"] for w in want]
    r = capi.solve(variants[0], method=1, pdlp_solver_mode=4, amd_halpern_resident=1, amd_halpern_batch=1)  # (a single solve is not changed by it)
    assert r["status"] == "Optimal" and r["steps_taken"] == want[0][0]["steps_taken"]


# ---- 8. speed -----------------------------------------------------------------------------------------------------------------------------------
def test_the_batch_is_faster_than_one_loop_after_the_other():
    """64 copies of 50v-10 at tol = 0, 4000 steps each after a warm-up: the batch's advance against the same 64 solvers advanced one after
    the other (what a caller of mode 4 got before the option).  At least 2.0x, or the batch defeats its purpose."""
    p = lp_only(golden(V50))
    K, steps = 64, 4000
    solvers = [capi.Solver(p, tol=0.0, **ON) for _ in range(K)]
    for s in solvers:
        s.advance(400)
    t0 = time.perf_counter()
    for s in solvers:
        s.advance(steps)
    alone = K * steps / (time.perf_counter() - t0)
    batch = capi.SmallBatch(solvers)
    batch.advance(400)
    t0 = time.perf_counter()
    got = batch.advance(steps)
    together = K * steps / (time.perf_counter() - t0)
    assert [r["steps_taken"] for r in got] == [400 + steps + 400 + steps] * K
    print("steps/s aggregate: batch %.0f, one after the other %.0f (%.2fx)" % (together, alone, together / alone))
    batch.close()
    assert together >= 2.0 * alone
