"""GPU: lockstep batches of K LPs over one matrix in the JAGGED layout (kernels_batch.hip kbj_a_dual / kbj_at_step; the solvers are
created with cuoptamd_settings::batch_lanes >= K).  Pinned here: every LP of a batch takes, bit for bit, the trajectory of a solver
created on that LP with the same batch_lanes -- the batched products reproduce the single jagged kernels' row sums, epilogues and
per-block reduction trees -- and batch_lanes = 0 leaves the layouts exactly as they were."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import set_tune
from cuopt_amd import capi, synthetic
from test_shared_batch_gpu import KEYS_F64, KEYS_INT, LIMIT, same, variants

pytestmark = pytest.mark.gpu


def banded(m=30000, n=24000, seed=21, band=700):
    return synthetic.generate(m, n, 10, seed=seed, band=band)


def single_runs(p, bounds, steps=130, **kw):
    """per LP: (result after `steps` iterations, solution then, final result, final solution) of a fresh solver"""
    out = []
    for lb, ub in bounds:
        s = capi.Solver(dict(p, lb=lb, ub=ub), **kw)
        a = s.advance(steps) if steps is not None else s.advance()
        sa = s.solution()
        b = s.advance() if steps is not None else None
        out.append((a, sa, b, s.solution() if steps is not None else None))
        s.close()
    return out


def lockstep(p, bounds, **kw):
    parent = capi.Solver(dict(p, lb=bounds[0][0], ub=bounds[0][1]), **kw)
    return parent, [parent] + [parent.clone(lb=lb, ub=ub) for lb, ub in bounds[1:]]


def close_all(solvers):
    for s in solvers[1:]:
        s.close()
    solvers[0].close()


@pytest.mark.parametrize("waves", [8, 16])
@pytest.mark.parametrize("k", [2, 4, 8, 16])
def test_jag_batch_trajectories_are_bit_identical_to_single_solves(k, waves, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "jag")
    set_tune(monkeypatch, jag_waves=waves)
    p = banded()
    bounds = variants(p, k)
    kw = dict(tol=1e-5, iteration_limit=LIMIT, batch_lanes=k)
    single = single_runs(p, bounds, **kw)
    parent, solvers = lockstep(p, bounds, **kw)
    lay = parent.device.layout()
    assert lay["A"]["layout"] == "jag" and lay["At"]["layout"] == "jag", lay
    batch = capi.SharedMatrixBatch(solvers)
    got = batch.advance(130)
    for l in range(k):
        same(got[l], single[l][0], solvers[l].solution(), single[l][1], "LP %d after 130 iterations" % l)
    got = batch.advance()
    for l in range(k):
        same(got[l], single[l][2], solvers[l].solution(), single[l][3], "LP %d at the end" % l)
    assert got[0]["status_name"] == "Optimal"
    assert len({g["steps_taken"] for g in got}) > 1  # (the LPs finish at different times)
    # a second round: the clones reset to other bounds, the batch re-created
    batch.close()
    for l in range(1, k):
        lb, ub = bounds[(l + 1) % k if (l + 1) % k else 1]
        solvers[l].reset(lb=lb, ub=ub, tol=1e-5, iteration_limit=LIMIT)
    parent.reset(tol=1e-5, iteration_limit=LIMIT)
    batch = capi.SharedMatrixBatch(solvers)
    got = batch.advance()
    same(got[0], single[0][2], parent.solution(), single[0][3], "parent, second round")
    for l in range(1, k):
        src = (l + 1) % k if (l + 1) % k else 1
        same(got[l], single[src][2], solvers[l].solution(), single[src][3], "LP %d, second round" % l)
    batch.close()
    close_all(solvers)


@pytest.mark.parametrize("k", [8, 16])
def test_full_size_blocks(k, monkeypatch):
    """786 432 rows: the geometry of 256 rows per wave, blocks capped at 16384 / batch_lanes rows (2048 / 1024: the strips of K LPs
    fill the LDS); 130 iterations of every LP against its single solve"""
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "jag")
    m = 786432
    p = synthetic.generate(m, m, 8, seed=3, band=1000)
    bounds = variants(p, k)
    kw = dict(tol=1e-5, iteration_limit=LIMIT, batch_lanes=k)
    single = single_runs(p, bounds, steps=130, **kw)
    parent, solvers = lockstep(p, bounds, **kw)
    lay = parent.device.layout()
    assert lay["A"]["layout"] == "jag" and lay["At"]["layout"] == "jag", lay
    assert lay["A"]["workgroups"] >= m // (16384 // k), lay
    batch = capi.SharedMatrixBatch(solvers)
    got = batch.advance(130)
    for l in range(k):
        same(got[l], single[l][0], solvers[l].solution(), single[l][1], "LP %d after 130 iterations" % l)
    batch.close()
    close_all(solvers)


def test_mixed_pair_jagged_a_and_csr_walk_on_at(monkeypatch):
    """A (196 608 rows, banded) in the jagged layout, A^T (98 304 rows: below the jagged layout's size) on the panels or the CSR
    stream: each side keeps its own batched kernels"""
    monkeypatch.delenv("CUOPT_AMD_SPMV_LAYOUT", raising=False)
    p = synthetic.generate(196608, 98304, 8, seed=5, band=400)
    k = 4
    bounds = variants(p, k, seed=2)
    kw = dict(tol=1e-4, iteration_limit=1500, batch_lanes=k)
    single = single_runs(p, bounds, steps=130, **kw)
    parent, solvers = lockstep(p, bounds, **kw)
    lay = parent.device.layout()
    assert lay["A"]["layout"] == "jag" and lay["At"]["layout"] in ("panel", "stream"), lay
    batch = capi.SharedMatrixBatch(solvers)
    got = batch.advance(130)
    for l in range(k):
        same(got[l], single[l][0], solvers[l].solution(), single[l][1], "mixed pair, LP %d after 130" % l)
    got = batch.advance()
    for l in range(k):
        same(got[l], single[l][2], solvers[l].solution(), single[l][3], "mixed pair, LP %d at the end" % l)
    batch.close()
    close_all(solvers)


@pytest.mark.parametrize("mode", [0, 2, 3])  # Stable1, Methodical1, Fast1
def test_jag_batch_under_the_other_presets(mode, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "jag")
    p = synthetic.generate(8000, 7000, 8, seed=33, band=300)
    bounds = variants(p, 4, seed=7)
    kw = dict(mode=mode, tol=1e-4, iteration_limit=1500, batch_lanes=4)
    single = single_runs(p, bounds, steps=None, **kw)
    parent, solvers = lockstep(p, bounds, **kw)
    batch = capi.SharedMatrixBatch(solvers)
    got = batch.advance()
    for l in range(4):
        same(got[l], single[l][0], solvers[l].solution(), single[l][1], "mode %d, LP %d" % (mode, l))
    batch.close()
    close_all(solvers)


def test_an_infeasible_member_gets_its_own_verdict(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "jag")
    p = synthetic.generate(4000, 3500, 6, seed=12, band=200)
    lb_bad, ub_bad = np.array(p["lb"], float), np.array(p["ub"], float)
    ub_bad[np.argsort(-p["x_star"])[:50]] = 0.0
    sets = [(np.array(p["lb"], float), np.array(p["ub"], float)), (lb_bad, ub_bad)] + variants(p, 3, seed=2)[1:]
    kw = dict(tol=1e-4, iteration_limit=LIMIT, detect_infeasibility=1, batch_lanes=4)
    single = single_runs(p, sets, steps=None, **kw)
    parent, solvers = lockstep(p, sets, **kw)
    batch = capi.SharedMatrixBatch(solvers)
    got = batch.advance()
    for l in range(4):
        same(got[l], single[l][0], solvers[l].solution(), single[l][1], "LP %d" % l)
    assert got[0]["status_name"] == "Optimal"
    assert got[1]["status_name"] == single[1][0]["status_name"] != "Optimal"
    batch.close()
    close_all(solvers)


def test_jag_batches_repeat_themselves_next_to_other_processes():
    probe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scripts", "jag_contention_probe.py")
    procs = [subprocess.Popen([sys.executable, probe, "4", "2"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for _ in range(4)]
    outs = [q.communicate(timeout=600)[0] for q in procs]
    for q, out in zip(procs, outs):
        assert q.returncode == 0, out[-2000:]
        rounds = [ln for ln in out.splitlines() if " round " in ln]
        assert len(rounds) == 2, out[-2000:]
        for ln in rounds:
            assert "False" not in ln, ln


def test_batch_solve_keeps_a_banded_group_one_after_the_other(monkeypatch):
    """cuoptamd_batch_solve of 29 LPs over one banded matrix: the jagged lockstep batch is measured slower than one LP after the other
    at every K (profiles/r07_jag_batch.txt), so the group goes through one set-up and one solver, LP after LP -- bit for bit the
    independent solves created with the same settings, batch_lanes or not; and solves created with batch_lanes = 16 (other block
    boundaries, other partial-sum trees) agree with default ones in status and to the last bits of the objective"""
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "jag")
    p = synthetic.generate(12000, 10000, 8, seed=9, band=400)
    lps = [dict(p, lb=lb, ub=ub) for lb, ub in variants(p, 29, seed=5)]
    kw = dict(tol=1e-4, iteration_limit=LIMIT)
    runs = {lanes: capi.batch_solve(lps, batch_lanes=lanes, **kw) for lanes in (0, 16)}
    set_tune(monkeypatch, shared_batch=0)
    for lanes, together in runs.items():
        apart = capi.batch_solve(lps, max_threads=2, batch_lanes=lanes, **kw)
        assert len(together) == len(apart) == 29
        for l, (a, b) in enumerate(zip(together, apart)):
            for key in KEYS_INT + KEYS_F64:
                assert a[key] == b[key], (lanes, l, key, a[key], b[key])
            for name in ("x", "y", "reduced_cost"):
                np.testing.assert_array_equal(a[name], b[name], err_msg="lanes %d, LP %d: %s" % (lanes, l, name))
    for l, (a, d) in enumerate(zip(runs[16], runs[0])):
        assert a["status_name"] == d["status_name"], l
        assert abs(a["primal_objective"] - d["primal_objective"]) <= 2 * np.finfo(float).eps * abs(d["primal_objective"]), (l, a["primal_objective"], d["primal_objective"])
    assert runs[0][0]["status_name"] == "Optimal"


def test_batch_lanes_zero_keeps_the_layouts(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "jag")
    p = synthetic.generate(262144, 262144, 10, seed=2, band=2000)
    a = capi.Solver(p, tol=1e-4, iteration_limit=10)
    b = capi.Solver(p, tol=1e-4, iteration_limit=10, batch_lanes=0)
    np.testing.assert_array_equal(a.device.layout_checksums(), b.device.layout_checksums())
    assert a.device.layout() == b.device.layout()
    a.close(), b.close()


@pytest.mark.parametrize("lanes", [8, 16])
def test_host_and_device_constructions_agree_under_batch_lanes(lanes, monkeypatch):
    """the capped blocks of build_jag (CUOPT_AMD_TUNE=jag_device=0) and of the device construction, array for array"""
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "jag")
    p = synthetic.generate(786432, 786432, 6, seed=2, band=1500)
    set_tune(monkeypatch, jag_device=0)
    host = capi.Solver(p, tol=1e-4, iteration_limit=10, batch_lanes=lanes)
    set_tune(monkeypatch, jag_device=None)
    dev = capi.Solver(p, tol=1e-4, iteration_limit=10, batch_lanes=lanes)
    plain = capi.Solver(p, tol=1e-4, iteration_limit=10)
    a, b = host.device.layout_checksums(), dev.device.layout_checksums()
    np.testing.assert_array_equal(a, b)
    assert host.device.layout() == dev.device.layout()
    if 16384 // lanes < 2048:  # (8 waves of 256 rows: the cap bites from 16 lanes on)
        assert dev.device.layout()["A"]["workgroups"] > plain.device.layout()["A"]["workgroups"]
    host.close(), dev.close(), plain.close()


def test_not_eligible_jagged_parents_are_refused(monkeypatch):
    """-7 for: a jagged parent created without batch_lanes (or with fewer lanes than the batch), a jagged side with rows longer than
    kLongRow (block-angular linking rows), a parent with dense row segments"""
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "jag")
    p = synthetic.generate(20000, 20000, 10, seed=2, band=500)
    for lanes, k in ((0, 2), (4, 8)):
        parent = capi.Solver(p, tol=1e-4, iteration_limit=200, batch_lanes=lanes)
        clones = [parent.clone() for _ in range(k - 1)]
        with pytest.raises(capi.CuOptError) as e:
            capi.SharedMatrixBatch([parent] + clones)
        assert e.value.code == -7 and "batch_lanes" in str(e.value), str(e.value)
        for c in clones:
            c.close()
        parent.close()
    q = synthetic.generate_structured("block_angular", m=200000, n=200000, k=8, seed=7)
    parent = capi.Solver(q, tol=1e-4, iteration_limit=200, batch_lanes=4)
    assert "jag" in (parent.device.layout()["A"]["layout"], parent.device.layout()["At"]["layout"])
    clone = parent.clone()
    with pytest.raises(capi.CuOptError) as e:
        capi.SharedMatrixBatch([parent, clone])
    assert e.value.code == -7
    clone.close(), parent.close()
    monkeypatch.delenv("CUOPT_AMD_SPMV_LAYOUT")
    d = synthetic.generate_structured("dense_rows", m=200000, n=200000, k=10, seed=7)
    parent = capi.Solver(d, tol=1e-4, iteration_limit=200, batch_lanes=4)
    with pytest.raises(capi.CuOptError) as e:
        parent.clone()  # (dense-segment contexts have no clones, hence no batch)
    assert e.value.code == -7
    parent.close()
