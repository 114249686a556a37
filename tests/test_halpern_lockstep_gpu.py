"""GPU: shared-matrix LOCKSTEP batches in reflected Halpern mode (solver mode 4 with cuoptamd_settings::halpern_lockstep;
kernels_batch_halpern.hip, docs/design/04d_halpern_mode.md "Lockstep batches").  The contract throughout: every member of a batch
gets, BIT FOR BIT, what its own freshly created Solver(mode=4) gives -- the result's integers and doubles, x, y, reduced costs and
the Halpern scalars (r, r_first, r2, r2_min, k) -- although the two products of a step serve all K LPs from one pass over the matrix
and every LP combines with the weights of its OWN k (restarts diverge between the members)."""
import os
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

import halpern_lockstep_case as case
from cuopt_amd import capi, synthetic
from halpern_lockstep_case import KEYS_F64, KEYS_INT, KW, LIMIT, close_all, layout_is, make_batch, same, state

pytestmark = pytest.mark.gpu

RESET_KW = dict(tol=1e-4, iteration_limit=LIMIT, halpern_lockstep=1)  # (a reset with settings replaces them all: the option again)


# ---- 1. trajectories -------------------------------------------------------------------------------------------------------------
# synthetic.generate(6000, 5000, 8, seed=33): several panels, several 512-row blocks per panel with a ragged last block.  The numpy
# restatement (tests/halpern_reference.py) gives the first four members 720 / 2840 / limit / 800 steps with 6 / 10 / 9 / 6 restarts and
# the sixteen six different outcomes: members rest at different times and restart at different steps.
@pytest.mark.parametrize("layout", ["panel", "stream"])
@pytest.mark.parametrize("k", [2, 4, 8, 16])
def test_trajectories_are_bit_identical_to_single_solves(k, layout, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    solvers, batch, _ = case.trajectories(k, layout)
    close_all(batch, solvers)


# ---- 2. tiny blocks: one partly filled row block; at K = 16 fewer entries than one staged chunk --------------------------------------
@pytest.mark.parametrize("k", [2, 16])
def test_tiny_blocks(k, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    p = synthetic.generate(600, 500, 6, seed=1)
    three = case.variants(p, 3)
    bounds = [three[l % 3] for l in range(k)]
    single = []
    for lb, ub in three:
        s = capi.Solver(dict(p, lb=lb, ub=ub), **KW)
        layout_is(s, "stream")
        single.append(state(s, s.advance()))
        s.close()
    solvers, batch = make_batch(p, bounds, **KW)
    got = batch.advance()
    for l in range(k):
        same(state(solvers[l], got[l]), single[l % 3], "LP %d" % l)  # (bit identity only: no condition on the verdicts)
    close_all(batch, solvers)


# ---- 3. second round: the clones reset to other bounds, the parent to its own, the batch re-created --------------------------------
def test_second_round_after_resets(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    k = 4
    solvers, batch, single = case.trajectories(k, "panel")
    batch.close()
    p, bounds = case.main_lp()
    src = [0] + [(l + 1) % k if (l + 1) % k else 1 for l in range(1, k)]
    for l in range(1, k):
        solvers[l].reset(lb=bounds[src[l]][0], ub=bounds[src[l]][1], **RESET_KW)
    solvers[0].reset(**RESET_KW)
    batch = capi.SharedMatrixBatch(solvers)  # (the table refresh; the anchor and the scalars after a reset)
    got = batch.advance()
    for l in range(k):
        same(state(solvers[l], got[l]), single[src[l]][1], "LP %d, second round" % l)
    close_all(batch, solvers)


# ---- 4. own row bounds: omega^0 differs per member ------------------------------------------------------------------------------
def test_own_row_bounds(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    p = synthetic.generate(9000, 7000, 8, seed=4)
    lo = np.where(np.isfinite(p["lo"]), p["lo"] - 0.5, p["lo"])
    hi = np.where(np.isfinite(p["hi"]), p["hi"] + 0.5, p["hi"])
    want = []
    for q in (p, dict(p, lo=lo, hi=hi)):
        s = capi.Solver(q, **KW)
        want.append(state(s, s.advance()))
        s.close()
    assert want[0][0]["initial_primal_weight"] != want[1][0]["initial_primal_weight"]
    parent = capi.Solver(p, **KW)
    child = parent.clone(lo=lo, hi=hi)
    batch = capi.SharedMatrixBatch([parent, child])
    got = batch.advance()
    same(state(parent, got[0]), want[0], "parent")
    same(state(child, got[1]), want[1], "clone with its own row bounds")
    close_all(batch, [parent, child])


# ---- 5. plain launches against graph replay ----------------------------------------------------------------------------------------
def test_plain_launches_give_the_bits_of_graph_replay(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    p, bounds = case.main_lp()
    single = case.main_singles("panel")
    solvers, batch = make_batch(p, bounds[:4], use_graph=0, **KW)
    got = batch.advance()
    for l in range(4):
        same(state(solvers[l], got[l]), single[l][1], "LP %d, use_graph=0" % l)
    close_all(batch, solvers)


# ---- 6. refusals and non-effects ---------------------------------------------------------------------------------------------------
def refused(solvers, code, *words):
    with pytest.raises(capi.CuOptError) as e:
        capi.SharedMatrixBatch(solvers)
    assert e.value.code == code, (e.value.code, str(e.value))
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    p, bounds = case.main_lp()
    plain = dict(tol=1e-4, iteration_limit=LIMIT)
    # no option
    parent = capi.Solver(p, mode=4, **plain)
    child = parent.clone(lb=bounds[1][0], ub=bounds[1][1])
    refused([parent, child], -7, "Halpern")
    child.close(), parent.close()
    # opted members next to members without the option; K = 3; the kernel timer
    parent = capi.Solver(p, **KW)
    unopted = parent.clone(lb=bounds[1][0], ub=bounds[1][1], **plain)
    refused([parent, unopted], -7, "halpern_lockstep")
    opted = [parent.clone(lb=lb, ub=ub) for lb, ub in bounds[1:3]]
    refused([parent] + opted, -1)
    batch = capi.SharedMatrixBatch([parent, opted[0]])
    with pytest.raises(capi.CuOptError) as e:
        batch.time_kernels(2)
    assert e.value.code == -7 and "Halpern" in str(e.value), str(e.value)
    batch.close()
    # Halpern next to averaging: two solvers over one matrix at the device layer (a clone shares its parent's iteration at the host layer)
    averaging = capi.Solver(p, halpern_lockstep=1, **plain)
    refused([parent, averaging], -7)
    twin = averaging.clone(lb=bounds[1][0], ub=bounds[1][1])
    twin.device.set_halpern(True)
    raw = lambda d: d.handle.value if hasattr(d.handle, "value") else int(d.handle)
    dev = capi.c_void_p()
    arr = (capi.c_void_p * 2)(raw(averaging.device), raw(twin.device))
    assert capi.lib.pdlpdev_batch_create(capi.C.byref(dev), arr, 2) == -7
    assert "mixes" in capi.lib.pdlpdev_last_error().decode()
    twin.close(), averaging.close()
    for s in [unopted] + opted:
        s.close()
    parent.close()


def test_a_jagged_parent_is_refused_by_name(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "jag")
    p = synthetic.generate(20000, 20000, 10, seed=2, band=500)
    parent = capi.Solver(p, batch_lanes=4, iteration_limit=200, mode=4, tol=1e-4, halpern_lockstep=1)
    lay = parent.device.layout()
    assert lay["A"]["layout"] == "jag" or lay["At"]["layout"] == "jag", lay
    child = parent.clone()
    refused([parent, child], -7, "jagged")
    child.close(), parent.close()


def test_the_averaging_modes_ignore_the_option(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    p, bounds = case.main_lp()
    out = []
    for extra in (dict(), dict(halpern_lockstep=1)):
        solvers, batch = make_batch(p, bounds[:2], tol=1e-4, iteration_limit=1500, **extra)
        got = batch.advance()
        out.append([(got[l], solvers[l].solution()) for l in range(2)])
        close_all(batch, solvers)
    for (a, sa), (b, sb) in zip(*out):
        for k in KEYS_INT + KEYS_F64:
            assert a[k] == b[k], (k, a[k], b[k])
        for u, v in zip(sa, sb):
            np.testing.assert_array_equal(u, v)


# ---- 7. routing through cuoptamd_batch_solve: 13 = 8 + 4 + 1 ------------------------------------------------------------------------
# Expected path "shared_matrix_halpern": the measured routing rule (docs/design/07_measurement.md, "Halpern mode": the lockstep median
# beats the sequential median by more than the two spreads combined at K = 4) keeps the routing on the panel layout, which this test uses.
def test_batch_solve_routes_through_the_halpern_lockstep_batch(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    p, bounds = case.main_lp()
    lps = [dict(p, lb=lb, ub=ub) for lb, ub in bounds[:13]]
    plain = dict(mode=4, tol=1e-4, iteration_limit=LIMIT)
    together = capi.batch_solve(lps, halpern_lockstep=1, **plain)
    assert capi.batch_solve_last_path() == "shared_matrix_halpern"
    without = capi.batch_solve(lps, **plain)
    assert capi.batch_solve_last_path() == "shared_matrix"  # (today's: one set-up, the clones one after the other)
    monkeypatch.setenv("CUOPT_AMD_TUNE", "shared_batch=0")
    apart = capi.batch_solve(lps, max_threads=2, **plain)
    assert capi.batch_solve_last_path() == "independent"
    single = case.main_singles("panel")
    for l in range(13):
        for k in KEYS_INT + KEYS_F64:
            assert together[l][k] == apart[l][k] == without[l][k], (l, k, together[l][k], apart[l][k], without[l][k])
            assert together[l][k] == single[l][1][0][k], (l, k)
        for name in ("x", "y", "reduced_cost"):
            np.testing.assert_array_equal(together[l][name], apart[l][name], err_msg="LP %d: %s" % (l, name))
            np.testing.assert_array_equal(without[l][name], apart[l][name], err_msg="LP %d: %s (without the option)" % (l, name))


# ---- 8. side by side: four processes share the GPU, each runs case 1 at K = 8 on the panels ----------------------------------------
def test_batches_repeat_themselves_next_to_other_processes():
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "halpern_lockstep_case.py")
    cmd = ["timeout", "-k", "10", "240", sys.executable, helper, "8", "panel"]  # (each child under a time limit of its own)
    logs = [tempfile.TemporaryFile(mode="w+") for _ in range(4)]  # (files, not pipes: nobody has to drain them while polling)
    procs = [subprocess.Popen(cmd, stdout=log, stderr=subprocess.STDOUT, text=True) for log in logs]
    def watch(q):  # one watcher per child, all four at once: the first child that fails ends the others
        if q.wait() != 0:
            for other in procs:
                if other is not q and other.poll() is None:
                    other.kill()

    watchers = [threading.Thread(target=watch, args=(q,)) for q in procs]
    for t in watchers:
        t.start()
    for t in watchers:
        t.join()
    outs = []
    for log in logs:
        log.seek(0)
        outs.append(log.read())
        log.close()
    for q, out in zip(procs, outs):
        assert q.returncode == 0, out[-2000:]
        assert "identical 8 panel" in out, out[-2000:]


# ---- interfaces --------------------------------------------------------------------------------------------------------------------
def test_the_option_travels_through_the_python_mirror(monkeypatch):
    from cuopt_amd import linear_programming as lp
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    settings = lp.SolverSettings()
    assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_LOCKSTEP) == 0
    settings.set_parameter(lp.CUOPT_PDLP_SOLVER_MODE, lp.PDLPSolverMode.Halpern1)
    settings.set_parameter(lp.CUOPT_AMD_HALPERN_LOCKSTEP, 1)
    settings.set_parameter(lp.CUOPT_ITERATION_LIMIT, LIMIT)
    p, bounds = case.main_lp()
    models = []
    for lb, ub in bounds[:4]:
        dm = lp.DataModel()
        dm.set_csr_constraint_matrix(p["values"], p["indices"], p["offsets"])
        dm.set_objective_coefficients(p["c"])
        dm.set_constraint_lower_bounds(p["lo"])
        dm.set_constraint_upper_bounds(p["hi"])
        dm.set_variable_lower_bounds(lb)
        dm.set_variable_upper_bounds(ub)
        models.append(dm)
    sols, _ = lp.BatchSolve(models, settings)
    assert capi.batch_solve_last_path() == "shared_matrix_halpern"
    single = case.main_singles("panel")
    assert [s.get_lp_stats()["nb_iterations"] for s in sols] == [single[l][1][0]["steps_taken"] for l in range(4)]
