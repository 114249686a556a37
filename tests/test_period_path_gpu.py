"""GPU: what a major-iteration period does outside its PDHG attempts.

(1) The evaluation of the CURRENT iterate reads its dual side from the loop's A^T y buffer instead of running the product again
    (k_panel_eval_dual_from_aty; CUOPT_AMD_TUNE=eval_reuse_aty=0 switches it off): same scalars, same vectors, bit for bit, on the
    panel layout in both variants, with a dense segment, with columns longer than 128 and with a column that owns a workgroup.
(2) The host tracks when that buffer is valid (pdlpdev_loop_stats): reuse on a plain solve, none in the first evaluation after
    set_initial, a warm start, a reset and a restart to the average.
(3) The fused period path (pdlpdev_run_period; CUOPT_AMD_TUNE=period_path=0 switches it off): one synchronisation per period where
    nothing is rejected and nothing restarts, and the same solve bit for bit."""
import numpy as np
import pytest
from conftest import set_tune

from cuopt_amd import capi, synthetic
from eval_lps import with_long_column as _with_long_column

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def multi_launch_kernels(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")  # these LPs are small: keep them off the resident one-workgroup path


def _case(name):
    if name == "dense-segment":
        return synthetic.generate_structured("dense_rows", m=70000, n=70000, k=8, seed=11)
    if name == "long-columns":
        p = _with_long_column(synthetic.generate(3000, 2600, 9, seed=12), 17, 400)
        return _with_long_column(p, 1900, 129, seed=4)
    if name == "column-with-its-own-workgroup":
        return _with_long_column(synthetic.generate(6000, 5000, 9, seed=13), 250, 4500)
    return synthetic.generate(3000, 2600, 9, seed=12)


CASES = [("plain", 0, 4096), ("plain", 0, 1 << 20), ("plain", 1, 32 * 1024), ("long-columns", 0, 4096), ("long-columns", 1, 32 * 1024),
         ("column-with-its-own-workgroup", 0, 64 * 1024), ("dense-segment", 0, 64 * 1024), ("dense-segment", 1, 64 * 1024)]


def _evaluations(p, reuse, seg, slab, monkeypatch):
    """the major evaluation at iteration 40, right after a restart to the average, and 40 iterations later"""
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    set_tune(monkeypatch, eval_reuse_aty=reuse, panel_seg=seg, slab_bytes=slab, dense=1)
    s = capi.Solver(p, mode=1, tol=0.0)
    s.advance(0)  # set-up, scaling, step size; the evaluation of iteration 0
    dev = s.device
    lay = dev.layout()
    assert lay["A"]["layout"] == lay["At"]["layout"] == "panel"
    out, stats = [], []

    def evaluate(mode):
        before = dev.loop_stats()
        cur, avg = dev.major_eval(mode)
        after = dev.loop_stats()
        out.append(dict(cur=cur, avg=avg, aty_u=dev.download("ATY_U_CURRENT", p["n"]), aty_u_avg=dev.download("ATY_U_AVERAGE", p["n"]),
                        rc=dev.download("RC_CURRENT", p["n"]), rc_avg=dev.download("RC_AVERAGE", p["n"])))
        stats.append((after["eval_reused_aty"] - before["eval_reused_aty"], after["eval_product"] - before["eval_product"]))

    ctl = dev.run(40)
    assert ctl.error == 0 and ctl.steps_taken == 40
    evaluate(2)
    dist = np.zeros(2)
    dev.call("restart", capi.AVERAGE, 0, capi._ptr(dist))
    evaluate(1)
    dev.call("compute_aty")
    ctl = dev.run(80)
    assert ctl.error == 0 and ctl.steps_taken == 80
    evaluate(2)
    info = dev.dense_info()
    s.close()
    return out, stats, info


@pytest.mark.parametrize("case,seg,slab", CASES, ids=["%s-%s-%dB" % (c, "longtail" if g else "rows", b) for c, g, b in CASES])
def test_evaluation_from_the_loops_aty_is_bit_equal(case, seg, slab, monkeypatch):
    p = _case(case)
    if case == "long-columns":
        assert np.sort(np.bincount(p["indices"], minlength=p["n"]))[-2] > 128
    if case == "column-with-its-own-workgroup":
        assert np.bincount(p["indices"], minlength=p["n"]).max() > 4096
    on, stats_on, info = _evaluations(p, 1, seg, slab, monkeypatch)
    off, stats_off, _ = _evaluations(p, 0, seg, slab, monkeypatch)
    if case == "dense-segment":
        assert info["on"] and info["segments"] >= 2
    # the twin ran at iteration 40 and 40 iterations behind the restart, the product right after the restart to the average
    assert stats_on == [(1, 0), (0, 1), (1, 0)], stats_on
    assert stats_off == [(0, 1), (0, 1), (0, 1)], stats_off
    for a, b in zip(on, off):
        for k in a:
            assert np.isfinite(a[k]).all(), k
            assert np.array_equal(a[k], b[k]), (k, np.abs(a[k] - b[k]).max())


def test_reuse_is_tracked_on_the_host(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    set_tune(monkeypatch, slab_bytes=64 * 1024)
    p = synthetic.generate(3000, 3000, 10, seed=4)
    s = capi.Solver(p, mode=1, tol=0.0)
    s.advance(0)
    st = s.device.loop_stats()
    assert st["eval_reused_aty"] == 0 and st["eval_product"] == 1  # the evaluation at iteration 0
    s.advance(400)
    st = s.device.loop_stats()
    # every period's evaluation behind accepted attempts reuses; the product runs only where a restart came in between
    assert st["eval_reused_aty"] >= 8, st
    assert st["eval_reused_aty"] + st["eval_product"] >= 10
    ws = s.get_warm_start()
    x, y, _ = s.solution()

    def first_evaluation(solver):
        before = solver.device.loop_stats()
        solver.advance(0)
        after = solver.device.loop_stats()
        return after["eval_reused_aty"] - before["eval_reused_aty"], after["eval_product"] - before["eval_product"]

    # a reset: the solver is a fresh one
    s.reset()
    assert first_evaluation(s) == (0, 1)
    s.close()
    # an initial solution (pdlpdev_set_initial)
    s = capi.Solver(p, mode=1, tol=0.0, init_x=x, init_y=y)
    assert first_evaluation(s) == (0, 1)
    s.close()
    # a warm start at iteration 400: a major iteration is due at once
    s = capi.Solver(p, mode=1, tol=0.0, warm_start=ws)
    assert first_evaluation(s) == (0, 1)
    s.close()


def test_one_synchronisation_per_period(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    set_tune(monkeypatch, slab_bytes=64 * 1024)
    p = synthetic.generate(3000, 3000, 10, seed=4)
    s = capi.Solver(p, mode=1, tol=0.0)
    period = int(s.hyper.major_iteration)
    window = 5 * period
    prev = s.advance(2 * window)
    clean_before = False
    for _ in range(40):
        st0 = s.device.loop_stats()
        r = s.advance(window)
        st1 = s.device.loop_stats()
        clean = (r["attempted_steps"] - prev["attempted_steps"] == r["steps_taken"] - prev["steps_taken"] == window
                 and r["num_restarts"] == prev["num_restarts"])
        if clean and clean_before:  # (the window before left neither a restart's control-block writes nor spare attempts behind)
            assert st1["loop_syncs"] - st0["loop_syncs"] == window // period, (st0, st1)
            assert st1["empty_attempts"] == st0["empty_attempts"]
            assert st1["eval_reused_aty"] - st0["eval_reused_aty"] == window // period
            s.close()
            return
        clean_before, prev = clean, r
    pytest.fail("no two windows in a row without a rejected attempt and without a restart")


@pytest.mark.parametrize("seg", [0, 1], ids=["rows", "longtail"])
def test_same_solve_with_the_fused_period_path_on_and_off(seg, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    p = synthetic.generate(5000, 4000, 8, seed=11)
    got = []
    for fused, reuse in ((1, 1), (0, 1), (0, 0)):
        set_tune(monkeypatch, period_path=fused, eval_reuse_aty=reuse, panel_seg=seg, slab_bytes=64 * 1024)
        s = capi.Solver(p, mode=1, tol=1e-6)
        r = s.advance()
        x, y, z = s.solution()
        st = s.device.loop_stats()
        s.close()
        assert r["status_name"] == "Optimal", r["status_name"]
        got.append((r, x, y, z, st))
    (r1, x1, y1, z1, st1) = got[0]
    assert st1["loop_syncs"] < got[1][4]["loop_syncs"]  # the fused path was taken
    assert st1["eval_reused_aty"] > 0 and got[2][4]["eval_reused_aty"] == 0
    for r0, x0, y0, z0, _ in got[1:]:
        assert (r1["steps_taken"], r1["attempted_steps"], r1["num_restarts"]) == (r0["steps_taken"], r0["attempted_steps"], r0["num_restarts"])
        assert np.array_equal(x1, x0) and np.array_equal(y1, y0) and np.array_equal(z1, z0)
        for k in ("primal_objective", "dual_objective", "l2_primal_residual", "l2_dual_residual", "step_size", "primal_weight"):
            assert r1[k] == r0[k], k
