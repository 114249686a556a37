"""GPU: cuoptamd_solver_reset_objective / cuoptamd_batch_reset_objectives -- the persistent re-solve with a new OBJECTIVE vector, the
feasibility pump's call pattern (linear_project_onto_polytope, cpp/src/mip/local_search/feasibility_pump/feasibility_pump.cu:145-249:
per round a distance objective to the rounded point over the same constraints, warm-started).  D_r, D_c, the initial step and mode 4's
sigma_max depend on A only; the scaled objective, ||c|| and the initial primal weight are formed again by one kernel and one reduction
whose sums carry the bits of the reductions a fresh solver runs.  So the reference is exact: after the call the solver is, bit for bit,
a solver freshly created on the LP with that objective -- on every solver path, in every mode, single and in the K-workgroup batch."""
import functools
import os
import time

import numpy as np
import pytest
import scipy.sparse as sp

import resident_lps
from cuopt_amd import capi, synthetic

pytestmark = pytest.mark.gpu
LIMIT = 6000  # every solve is bounded: both solvers must then stop alike


def same_result(a, b, xa, xb):
    for k in ("status", "steps_taken", "attempted_steps", "num_restarts", "num_major_iterations"):
        assert a[k] == b[k], k
    for k in ("primal_objective", "dual_objective", "gap", "l2_primal_residual", "l2_dual_residual", "step_size",
              "primal_weight", "initial_step_size", "initial_primal_weight"):
        assert a[k] == b[k], k
    for u, v in zip(xa, xb):
        np.testing.assert_array_equal(u, v)


def same_as_fresh(s, a, q, **kw):
    """the persistent solver's result `a` against a solver freshly created on q"""
    fresh = capi.Solver(q, **kw)
    try:
        b = fresh.advance()
        same_result(a, b, s.solution(), fresh.solution())
        assert a["norm_c"] == b["norm_c"] and a["norm_b"] == b["norm_b"] and a["initial_primal_weight"] == b["initial_primal_weight"]
    finally:
        fresh.close()
    return b


def perturbed(c, rng):
    out = np.asarray(c, float) * (1.0 + 0.3 * rng.standard_normal(len(c)))
    out[rng.random(len(c)) < 0.1] = 0.0
    return out


@functools.lru_cache(maxsize=None)
def big_lp():
    return synthetic.generate(6000, 5000, 8, seed=5)


@functools.lru_cache(maxsize=None)
def small_lp():
    return synthetic.generate(700, 1000, 8, seed=5)


# ---- 1. equals a fresh solver ----------------------------------------------------------------------------------------------------------
MODES = [(1, {}), (0, {}), (2, {}), (4, {})]
CASES = [(case, mode, kw) for case in ("resident", "stream", "panel", "jag", "pb") for mode, kw in MODES] + [("resident", 4, dict(halpern_resident=1))]


@pytest.mark.parametrize("case,mode,extra", CASES, ids=["%s-mode%d%s" % (c, m, "-resident-loop" if kw else "") for c, m, kw in CASES])
def test_reset_objective_equals_fresh_solver(case, mode, extra, monkeypatch):
    if case not in ("resident",):
        monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", case)
    p = small_lp() if case == "resident" else big_lp()
    st = dict(tol=1e-4 if mode == 4 else 1e-6, iteration_limit=LIMIT, **extra)  # (a reset with settings replaces them all)
    kw = dict(st, mode=mode)
    rng = np.random.default_rng(17)
    s = capi.Solver(p, **kw)
    try:
        lay = s.device.layout()
        if case == "resident":
            assert lay["resident"] == (mode != 4 or bool(extra)), lay
        else:
            assert not lay["resident"] and case in (lay["A"]["layout"], lay["At"]["layout"]), lay
        s.advance()
        x0, y0, _ = s.solution()
        # a perturbed objective, from zero
        c1 = perturbed(p["c"], rng)
        s.reset_objective(c1, **st)
        a = s.advance()
        same_as_fresh(s, a, dict(p, c=c1, objective_offset=0.0), **kw)
        # another one with an offset and new variable bounds, from the previous solution
        x1, y1, _ = s.solution()
        c2 = perturbed(p["c"], rng)
        lb = np.where(np.isfinite(p["lb"]), p["lb"] - 0.25, p["lb"])
        ub = np.where(np.isfinite(p["ub"]), p["ub"] + 0.5, p["ub"])
        s.reset_objective(c2, objective_offset=3.25, lb=lb, ub=ub, init_x=x1, init_y=y1, **st)
        a = s.advance()
        same_as_fresh(s, a, dict(p, c=c2, objective_offset=3.25, lb=lb, ub=ub), init_x=x1, init_y=y1, **kw)
        # the original objective (and bounds) again, from zero
        s.reset_objective(p["c"], objective_offset=float(p.get("objective_offset", 0.0)), lb=p["lb"], ub=p["ub"], **st)
        a = s.advance()
        same_as_fresh(s, a, p, **kw)
    finally:
        s.close()


def test_a_maximise_solver_takes_the_maximise_sense_objective():
    p = small_lp()
    pmax = dict(p, c=-np.asarray(p["c"]), maximize=True)  # the same LP, stated as a maximisation
    kw = dict(tol=1e-6, iteration_limit=LIMIT)
    s = capi.Solver(pmax, **kw)
    try:
        s.advance()
        c1 = perturbed(pmax["c"], np.random.default_rng(3))
        s.reset_objective(c1, objective_offset=-1.5, **kw)
        a = s.advance()
        same_as_fresh(s, a, dict(pmax, c=c1, objective_offset=-1.5), **kw)
        # ... and is the minimisation of -c1 with the mirrored offset
        m = capi.Solver(dict(p, c=-c1, objective_offset=1.5), **kw)
        r = m.advance()
        assert r["primal_objective"] == -a["primal_objective"] and r["steps_taken"] == a["steps_taken"]
        m.close()
    finally:
        s.close()


# ---- 2. edges of the weight rule and of the reduction ------------------------------------------------------------------------------------
def edge_check(p, c, mode=1, iterations=120, hyper=None, **extra):
    st = dict(tol=0.0, iteration_limit=iterations, **extra)
    kw = dict(st, mode=mode, hyper=hyper)
    s = capi.Solver(p, **kw)
    try:
        s.advance()
        s.reset_objective(c, **st)
        a = s.advance()
        same_as_fresh(s, a, dict(p, c=c, objective_offset=0.0), **kw)
        return a
    finally:
        s.close()


def test_a_zero_objective_takes_the_primal_importance():
    p = small_lp()
    a = edge_check(p, np.zeros(p["n"]))
    assert a["norm_c"] == 0.0 and a["initial_primal_weight"] == capi.hyper_preset(1).primal_importance


def test_one_entry_in_the_last_column():
    for p in (small_lp(), big_lp()):
        c = np.zeros(p["n"])
        c[-1] = -2.5
        a = edge_check(p, c)
        assert a["norm_c"] == 2.5


@pytest.mark.parametrize("name", ["minimal-2x1", "rows-only"])
def test_fewer_columns_than_a_workgroup_has_threads(name):
    p = resident_lps.lp(name)[0]
    assert p["n"] in (1, 40)
    edge_check(p, perturbed(p["c"], np.random.default_rng(5)) + 0.125)


def test_the_first_n_past_the_cap_of_the_partials():
    """n = 256 * 1024 + 257: grid_for(n) is 1026 workgroups, the generic partials stop at 1024 -- the grid-stride loop takes a second trip"""
    n = 256 * 1024 + 257
    p = synthetic.generate(30000, n, 9, seed=8)  # (every column gets an entry: n <= 9 m)
    edge_check(p, perturbed(p["c"], np.random.default_rng(6)), iterations=40)


@pytest.mark.parametrize("before_scaling", [None, 0, 1], ids=["preset", "after-scaling", "before-scaling"])
def test_methodical1_with_the_weight_from_either_sum(before_scaling):
    """compute_initial_primal_weight_before_scaling as Methodical1's preset has it, and both of its values: the weight then comes from
    the sum of squares of the unscaled (1) or of the scaled (0) objective"""
    hyper = capi.hyper_preset(2)
    if before_scaling is not None:
        hyper.compute_initial_primal_weight_before_scaling = before_scaling
    for p in (small_lp(), big_lp()):
        edge_check(p, perturbed(p["c"], np.random.default_rng(7)), mode=2, hyper=hyper)


# ---- 3. graphs -----------------------------------------------------------------------------------------------------------------------------
def test_captured_attempt_graphs_see_the_new_objective(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    p = big_lp()
    kw = dict(tol=1e-6, iteration_limit=LIMIT, use_graph=1)
    s = capi.Solver(p, **kw)
    try:
        assert not s.device.layout()["resident"]
        s.advance(200)  # (the graphs exist now)
        c1 = perturbed(p["c"], np.random.default_rng(9))
        s.reset_objective(c1)  # settings unchanged: use_graph stays
        a = s.advance()
        same_as_fresh(s, a, dict(p, c=c1, objective_offset=0.0), **kw)
    finally:
        s.close()


# ---- 4. a reordered LP: c arrives in the caller's column order -------------------------------------------------------------------------
def test_a_reordered_lp_takes_the_objective_in_the_callers_order():
    p = synthetic.shuffled(synthetic.generate(131072, 131072, 10, seed=2, band=2000), seed=5)
    kw = dict(tol=0.0, iteration_limit=200)
    s = capi.Solver(p, **kw)
    try:
        assert s.reorder_info()["reordered"]
        s.advance(40)
        c1 = perturbed(p["c"], np.random.default_rng(10))
        s.reset_objective(c1, objective_offset=0.5, **kw)
        a = s.advance()
        same_as_fresh(s, a, dict(p, c=c1, objective_offset=0.5), **kw)
    finally:
        s.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def refused(s, c):
    with pytest.raises(capi.CuOptError) as e:
        s.reset_objective(c, objective_offset=7.0, tol=1e-2, iteration_limit=3)
    assert e.value.code == -7 and "cuoptamd_solver_reset_objective" in str(e.value), str(e.value)


def test_a_parent_with_a_live_clone_and_the_clone_are_refused():
    p = big_lp()
    kw = dict(tol=1e-6, iteration_limit=400)
    parent, twin = capi.Solver(p, **kw), capi.Solver(p, **kw)
    child = parent.clone()
    child_twin = twin.clone()
    try:
        for s in (parent, twin, child, child_twin):
            s.advance(80)
        c1 = perturbed(p["c"], np.random.default_rng(12))
        refused(parent, c1)
        refused(child, c1)
        same_result(parent.advance(), twin.advance(), parent.solution(), twin.solution())
        same_result(child.advance(), child_twin.advance(), child.solution(), child_twin.solution())
    finally:
        child.close(), child_twin.close(), parent.close(), twin.close()
    # once the clone is gone the objective is the solver's own again
    parent = capi.Solver(p, **kw)
    try:
        parent.clone().close()
        c1 = perturbed(p["c"], np.random.default_rng(12))
        parent.reset_objective(c1, **kw)
        same_as_fresh(parent, parent.advance(), dict(p, c=c1, objective_offset=0.0), **kw)
    finally:
        parent.close()


@pytest.mark.parametrize("kw", [dict(), dict(mode=4, halpern_lockstep=1)], ids=["averaging", "halpern_lockstep"])
def test_members_of_a_lockstep_batch_are_refused(kw, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    q = synthetic.generate(3000, 3000, 6)
    kw = dict(kw, tol=0.0, iteration_limit=120)
    parent, twin = capi.Solver(q, **kw), capi.Solver(q, **kw)
    child = parent.clone()
    batch = capi.SharedMatrixBatch([parent, child])
    try:
        batch.advance(40)
        twin.advance(40)
        c1 = perturbed(q["c"], np.random.default_rng(13))
        refused(parent, c1)
        refused(child, c1)
        with pytest.raises(capi.CuOptError) as e:
            batch.reset_objectives([c1, c1])
        assert e.value.code == -7 and "cuoptamd_batch_reset_objectives" in str(e.value), str(e.value)
        got = batch.advance()
        want = twin.advance()
        for r, s in zip(got, (parent, child)):
            same_result(r, want, s.solution(), twin.solution())
    finally:
        batch.close(), child.close(), parent.close(), twin.close()


def test_a_solver_behind_a_communicator_is_refused():
    p = big_lp()
    kw = dict(tol=1e-6, iteration_limit=400)
    s = capi.Solver(p, rank=0, world=1, comm_id=capi.softcomm_id(1), **kw)
    twin = capi.Solver(p, rank=0, world=1, comm_id=capi.softcomm_id(1), **kw)
    try:
        s.advance(80), twin.advance(80)
        refused(s, perturbed(p["c"], np.random.default_rng(14)))
        same_result(s.advance(), twin.advance(), s.solution(), twin.solution())
    finally:
        s.close(), twin.close()


# ---- 6. the K-workgroup batch ------------------------------------------------------------------------------------------------------------
MEMBERS = ("t0", "t1", "t2", "t1-full", "rows-only", "minimal-1x2")  # all three tiers, six matrices
BATCH_KW = {"averaging": dict(tol=1e-6, iteration_limit=400), "halpern_batch": dict(mode=4, tol=1e-6, iteration_limit=400, halpern_resident=1, halpern_batch=1)}


def open_batch(names, kw):
    solvers = [capi.Solver(resident_lps.lp(name)[0], **kw) for name in names]
    for s in solvers:
        assert s.device.layout()["resident"]
    return capi.SmallBatch(solvers), solvers


@pytest.mark.parametrize("flavour", list(BATCH_KW))
def test_batch_members_equal_their_single_solves(flavour):
    kw = BATCH_KW[flavour]
    lps = [resident_lps.lp(name)[0] for name in MEMBERS]
    rng = np.random.default_rng(21)
    batch, solvers = open_batch(MEMBERS, kw)
    singles = [capi.Solver(p, **kw) for p in lps]
    try:
        assert batch.stats()["halpern"] == (1 if flavour == "halpern_batch" else 0)
        batch.advance()
        for s in singles:
            s.advance()
        # round 1: new objectives from zero, member 2 keeps its own
        cs = [perturbed(p["c"], rng) for p in lps]
        cs[2] = None
        offs = [0.5 * l for l in range(len(lps))]
        views = batch.solution_views()
        batch.reset_objectives(cs, objective_offset=offs)
        assert batch.solution_views() is not views
        got = batch.advance()
        sols = batch.solutions()
        for l, (p, s) in enumerate(zip(lps, singles)):
            if cs[l] is None:
                s.reset()
                q = p
            else:
                s.reset_objective(cs[l], objective_offset=offs[l])
                q = dict(p, c=cs[l], objective_offset=offs[l])
            a = s.advance()
            same_result(got[l], a, sols[l], s.solution())
            assert got[l]["norm_c"] == a["norm_c"]
            same_as_fresh(s, a, q, **kw)
        # round 2: from the last returned point, on the device
        cs = [perturbed(p["c"], rng) for p in lps]
        cs[4] = None
        batch.reset_objectives(cs, warm_from_last=True)
        got = batch.advance()
        sols = batch.solutions()
        for l, (p, s) in enumerate(zip(lps, singles)):
            x, y, _ = s.solution()
            if cs[l] is None:
                s.reset(init_x=x, init_y=y)
            else:
                s.reset_objective(cs[l], init_x=x, init_y=y)
            a = s.advance()
            same_result(got[l], a, sols[l], s.solution())
            assert got[l]["norm_c"] == a["norm_c"]
        with pytest.raises(capi.CuOptError) as e:
            batch.reset_objectives(cs, init_x=[None] * len(lps), warm_from_last=True)
        assert e.value.code == -1 and "warm_from_last" in str(e.value)
    finally:
        batch.close()
        for s in solvers + singles:
            s.close()


@pytest.mark.parametrize("flavour", list(BATCH_KW))
def test_launches_do_not_depend_on_k_and_the_synchronisations_are_a_resets(flavour):
    kw = BATCH_KW[flavour]
    cost = {}
    for names in (MEMBERS[:2], MEMBERS):
        batch, solvers = open_batch(names, kw)
        try:
            batch.advance(40)
            s0 = batch.reset_stats()
            batch.reset()
            s1 = batch.reset_stats()
            batch.reset_objectives([np.asarray(resident_lps.lp(name)[0]["c"]) * 2.0 for name in names])
            s2 = batch.reset_stats()
            cost[len(names)] = (s2["launches"] - s1["launches"], s2["syncs"] - s1["syncs"], s1["launches"] - s0["launches"], s1["syncs"] - s0["syncs"])
        finally:
            batch.close()
            for s in solvers:
                s.close()
    assert cost[2] == cost[6], cost
    launches, syncs, reset_launches, reset_syncs = cost[6]
    assert syncs == reset_syncs == 1 and launches == reset_launches + 2, cost  # the objective kernel and its finish, nothing else


# ---- 7. the pump sequence on the 50v-10 relaxation -------------------------------------------------------------------------------------
V50 = "mip-50v-10-free-bound-relaxation"
PUMP_KW = dict(tol=1e-6, iteration_limit=50000)


def pump_objective(p, x, alpha):
    """linear_project_onto_polytope's distance objective to the rounding of x (feasibility_pump.cu:160-197) mixed with the original one by
    adjust_objective_with_original (:82-116) -> (c, offset).  NO auxiliary variables: an integer column whose rounded value sits on
    neither bound (7-8 general integers per round here) gets coefficient 0 instead of the reference's distance variable and its two rows,
    which would change A."""
    ints = np.asarray(p["var_types"]) == ord("I")
    lb, ub, c = p["lb"], p["ub"], np.asarray(p["c"], float)
    r = np.clip(np.round(x), lb, ub)
    at_ub = ints & (r == ub)
    at_lb = ints & ~at_ub & (r == lb)
    d = np.zeros(p["n"])
    d[at_ub], d[at_lb] = -1.0, 1.0
    offset = float(ub[at_ub].sum() - lb[at_lb].sum())
    return d * ((1.0 - alpha) / np.linalg.norm(d)) + (alpha / np.linalg.norm(c)) * c, offset, int((ints & ~at_ub & ~at_lb).sum())


def test_pump_sequence_through_one_persistent_solver(golden_problems):
    """Eight pump rounds on the 50v-10 relaxation (233 x 2013) through ONE solver: the reference's distance objective with alpha =
    0.9^round, warm-started from the previous point; integer columns whose rounded value sits on neither bound get coefficient 0 -- no
    auxiliary variables.  Every round ends Optimal within 2e-5 (1 + |f|) of HiGHS, the sequence is not slower than a solver per round,
    and the same eight objectives through a K = 8 batch equal their single solves."""
    from scipy.optimize import linprog
    full = dict(golden_problems[V50]["problem"])
    p = {k: v for k, v in full.items() if k != "var_types"}
    A = sp.csr_matrix((p["values"], p["indices"], p["offsets"]), shape=(p["m"], p["n"]))
    A_ub = sp.vstack([A[np.isfinite(p["hi"])], -A[np.isfinite(p["lo"])]])
    b_ub = np.concatenate([p["hi"][np.isfinite(p["hi"])], -p["lo"][np.isfinite(p["lo"])]])
    bounds = list(zip(p["lb"], p["ub"]))
    s = capi.Solver(p, **PUMP_KW)
    plan = []
    try:
        assert s.device.layout()["resident"]
        assert s.advance()["status_name"] == "Optimal"
        for k in range(1, 9):
            x, y, _ = s.solution()
            c, offset, interior = pump_objective(full, x, 0.9 ** k)
            ref = linprog(c, A_ub=A_ub, b_ub=b_ub, bounds=bounds, method="highs")
            assert ref.status == 0
            f = ref.fun + offset
            s.reset_objective(c, objective_offset=offset, init_x=x, init_y=y, **PUMP_KW)
            r = s.advance()
            print("pump round %d: %d interior integers, %d steps, objective %.9g (HiGHS %.9g)" % (k, interior, r["steps_taken"], r["primal_objective"], f))
            assert r["status_name"] == "Optimal"
            assert r["primal_objective"] == pytest.approx(f, abs=2e-5 * (1 + abs(f)))
            plan.append((c, offset, x.copy(), y.copy(), r, s.solution()))
        # the same eight rounds timed both ways (the same work in the loop: the results are bit-identical)
        t0 = time.perf_counter()
        for c, offset, ix, iy, _, _ in plan:
            s.reset_objective(c, objective_offset=offset, init_x=ix, init_y=iy, **PUMP_KW)
            s.advance()
        t_persistent = time.perf_counter() - t0
        t0 = time.perf_counter()
        for c, offset, ix, iy, r, sol in plan:
            f = capi.Solver(dict(p, c=c, objective_offset=offset), init_x=ix, init_y=iy, **PUMP_KW)
            f.advance()
            f.close()
        t_fresh = time.perf_counter() - t0
        print("pump sequence of %d rounds: persistent %.2f ms, solver per round %.2f ms" % (len(plan), 1e3 * t_persistent, 1e3 * t_fresh))
        c, offset, ix, iy, r, sol = plan[-1]
        f = capi.Solver(dict(p, c=c, objective_offset=offset), init_x=ix, init_y=iy, **PUMP_KW)
        same_result(r, f.advance(), sol, f.solution())
        f.close()
        if "PYTEST_XDIST_WORKER" not in os.environ:  # (a rate comparison: not under the contention soak, where four processes share the GPU)
            assert t_persistent < 1.1 * t_fresh
    finally:
        s.close()
    # eight copies, eight rounded points, one batch: each member against its single solve
    solvers = [capi.Solver(p, **PUMP_KW) for _ in plan]
    batch = capi.SmallBatch(solvers)
    try:
        batch.advance()
        batch.reset_objectives([e[0] for e in plan], objective_offset=[e[1] for e in plan], init_x=[e[2] for e in plan], init_y=[e[3] for e in plan])
        got = batch.advance()
        sols = batch.solutions()
        for l, (c, offset, ix, iy, r, sol) in enumerate(plan):
            same_result(got[l], r, sols[l], sol)
    finally:
        batch.close()
        for q in solvers:
            q.close()
