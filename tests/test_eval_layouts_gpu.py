"""GPU: the convergence evaluation in EVERY SpMV layout against the extended-precision reference (tests/eval_reference.py).

The eval_primal / eval_dual products of the stream, panel (rows per lane and long-tail), jagged and gather-free layouts, the
product-free twin k_panel_eval_dual_from_aty and k_finalize_eval, at cur = 0 and cur = 1, for CURRENT, AVERAGE and LAST_RESTART, with
and without the l-infinity vectors, with and without dense segments.  The vectors the epilogues store (A x, A^T y, the reduced costs)
are compared per element against bounds the reference DERIVES (no tolerance is guessed), the eight scalars at the tolerances of
test_kernels_gpu.test_convergence_information_matches_oracle, the infeasibility information against the oracle.  Everything is taken
against the reference at the iterate the device holds (downloaded, unscaled as the epilogues unscale it), never against another layout.

The gather-free layout takes the LP with a column of 2400 nonzeros (the length test_kernels_gpu.ragged_problem proves it holds); every
other layout the one with 4500, a column with a workgroup of its own.

The gather-free layout's WIDE geometry cannot hold the 6000 x 6000 LP at all, whatever the long column (build_pb_wide: its 76 000
nonzeros are one (bin, panel) chunk of more than 65535 entries; and with fewer than seven 8192-column panels more than a tenth of
the nonzeros sit in rows with more than 7 entries inside one step of their bin) and quietly takes the other geometry.  Its id
therefore evaluates the same LP with 60000 columns -- same rows, long rows, long and empty columns, kinds and iterates; the
narrowest width tried that both sides accept (57500 and 60000 do, 50000 does not) -- where A is one bin over eight panels and A^T
eight bins, with serial rows on both sides."""
import numpy as np
import pytest
from conftest import set_tune

import eval_reference as er
from cuopt_amd import capi
from eval_lps import N, SEEDS, WIDE_N, edge_lp
from oracle import orcbind

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def multi_launch_kernels(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")  # these LPs are small: keep them off the resident one-workgroup path


# id -> (layout, knobs of CUOPT_AMD_TUNE, length of the long column, dense segments[, columns])
VARIANTS = {
    "stream": ("stream", dict(), 4500, False),
    "panel-rows-4KiB": ("panel", dict(panel_seg=0, slab_bytes=4096), 4500, False),
    "panel-rows-1slab": ("panel", dict(panel_seg=0, slab_bytes=1 << 20), 4500, False),
    "panel-longtail": ("panel", dict(panel_seg=1, slab_bytes=32768, panel_nnz=2048), 4500, False),
    "jag-8": ("jag", dict(jag_waves=8), 4500, False),
    "jag-16": ("jag", dict(jag_waves=16), 4500, False),
    "pb": ("pb", dict(), 2400, False),
    "pb-wide": ("pb", dict(pb_wide=1), 2400, False, WIDE_N),
    "dense-stream": ("stream", dict(), 4500, True),
    "dense-panel-rows": ("panel", dict(panel_seg=0, slab_bytes=4096), 4500, True),
    "dense-panel-longtail": ("panel", dict(panel_seg=1, slab_bytes=32768, panel_nnz=2048), 4500, True),
    "dense-jag-8": ("jag", dict(jag_waves=8), 4500, True),
    "dense-pb": ("pb", dict(), 2400, True),
}

_lps = {}


def _lp(long_col, dense, n=N):
    key = (long_col, dense, n)
    if key not in _lps:
        p, x, y = edge_lp(long_col, dense, SEEDS[1] if dense else SEEDS[0], n=n)
        for a in list(p.values()) + [x, y]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)  # shared among the ids: nobody changes it
        _lps[key] = (p, x, y, np.diff(p["offsets"]) == 0, np.bincount(p["indices"], minlength=p["n"]) == 0)
    return _lps[key]


def _check_scalars(ev, ref, want_linf, tag):
    """the tolerances of test_convergence_information_matches_oracle"""
    if not isinstance(ev, dict):
        ev = {k: ev[i] for k, i in capi.EV.items()}
    print("SCALARS %s " % tag + " ".join("%s=%.3e" % (k, abs(ev[k] - ref[k]) / max(abs(ref[k]), 1e-300)) for k in er.SCALARS if ref[k] != 0.0))
    assert ev["CX"] == pytest.approx(ref["CX"], rel=1e-11), tag
    assert ev["DUAL_SUM"] == pytest.approx(ref["DUAL_SUM"], rel=1e-10), tag
    assert np.sqrt(ev["PRES2"]) == pytest.approx(np.sqrt(ref["PRES2"]), rel=1e-11, abs=1e-12), tag
    assert np.sqrt(ev["DRES2"]) == pytest.approx(np.sqrt(ref["DRES2"]), rel=1e-11, abs=1e-12), tag
    assert np.sqrt(ev["X2"]) == pytest.approx(np.sqrt(ref["X2"]), rel=1e-12), tag
    assert np.sqrt(ev["Y2"]) == pytest.approx(np.sqrt(ref["Y2"]), rel=1e-12), tag
    if want_linf:
        assert ref["LINF_PRES_REL"] > 0.0 and ref["LINF_DRES_REL"] > 0.0, tag
        assert ev["LINF_PRES_REL"] == pytest.approx(ref["LINF_PRES_REL"], rel=1e-10, abs=1e-11), tag
        assert ev["LINF_DRES_REL"] == pytest.approx(ref["LINF_DRES_REL"], rel=1e-10, abs=1e-11), tag
    else:
        assert ev["LINF_PRES_REL"] == 0.0 and ev["LINF_DRES_REL"] == 0.0, tag


def _check_vectors(dev, slot, ref, empty_rows, empty_cols, tag):
    """A x per row, A^T y and the reduced costs per column, each within the reference's bound"""
    m, n = len(empty_rows), len(empty_cols)
    ax, aty, rc = dev.download("AX_U_" + slot, m), dev.download("ATY_U_" + slot, n), dev.download("RC_" + slot, n)
    keep = ~ref["near_tie"]
    ratios = dict(ax=er.worst_ratio(er.abs_err(ref, "ax", ax), ref["bound_ax"]),
                  aty=er.worst_ratio(er.abs_err(ref, "aty", aty), ref["bound_aty_prod"]),
                  rc=er.worst_ratio(er.abs_err(ref, "rc", rc), ref["bound_aty"], keep))
    print("RATIOS %s ax=%.3f aty=%.3f rc=%.3f ties=%d" % (tag, ratios["ax"], ratios["aty"], ratios["rc"], ref["near_tie"].sum()))
    assert np.isfinite(ax).all() and np.isfinite(aty).all() and np.isfinite(rc).all(), tag
    assert ratios["ax"] <= 1.0, (tag, ratios)
    assert ratios["aty"] <= 1.0, (tag, ratios)
    assert ref["near_tie"].mean() <= 0.005, tag
    assert ratios["rc"] <= 1.0, (tag, ratios)
    assert (ax[empty_rows] == 0.0).all() and (aty[empty_cols] == 0.0).all(), tag
    assert (rc[ref["g_is_zero"]] == 0.0).all() and ref["g_is_zero"].any(), tag
    return ratios


def _iterate(dev, xname, yname, dr, dc):
    """the unscaled iterate as the epilogues form it"""
    return dev.download(xname, len(dc)) * dc, dev.download(yname, len(dr)) * dr


def variant_lp(name):
    """(p, x0, y0, empty rows, empty columns) of id `name`: shared among the ids and the test files, read-only"""
    return _lp(VARIANTS[name][2], VARIANTS[name][3], *VARIANTS[name][4:])


def open_variant(name, p, monkeypatch, **tune):
    """a context for LP p in the layout and geometry of id `name` (further CUOPT_AMD_TUNE keys in `tune`), and the assertions that
    it IS that layout, that geometry and, where the id says so, the dense-segment prologue"""
    layout, knobs, long_col, dense = VARIANTS[name][:4]
    m, n = p["m"], p["n"]
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    set_tune(monkeypatch, dense=1 if dense else 0, **knobs, **tune)
    dev = capi.Device(p)
    lay = dev.layout()
    print("LAYOUT %s %s" % (name, lay))
    assert lay["A"]["layout"] == lay["At"]["layout"] == layout, lay
    if layout == "panel":
        sums = "by_nonzero" if knobs["panel_seg"] else "by_row"
        assert lay["A"]["row_sums"] == lay["At"]["row_sums"] == sums, lay
        assert (lay["A"]["slabs"] == lay["At"]["slabs"] == 1) == (knobs["slab_bytes"] >= 8 * n), lay
        assert knobs.get("panel_nnz") is None or min(lay["A"]["workgroups"], lay["At"]["workgroups"]) >= 20, lay  # many panels
    if layout == "pb":  # the wide geometry: bins of 8192 rows; the other one: of at most 1024
        wide = (lay["A"]["workgroups"], lay["At"]["workgroups"]) == (-(-m // 8192), -(-n // 8192))
        assert wide == bool(knobs.get("pb_wide")) and (wide or min(lay["A"]["workgroups"], lay["At"]["workgroups"]) >= -(-min(m, n) // 1024)), lay
    info = dev.dense_info()
    assert info["on"] == dense and (not dense or (info["segments"] >= 2 and info["entries"] > 4096 + 256)), info
    return dev


def _evaluations(name, reuse, monkeypatch):
    layout, knobs, long_col, dense = VARIANTS[name][:4]
    p, x0, y0, empty_rows, empty_cols = variant_lp(name)
    m, n = p["m"], p["n"]
    dev = open_variant(name, p, monkeypatch, eval_reuse_aty=reuse)
    worst = {}

    def vectors(slot, ref, phase):
        for k, v in _check_vectors(dev, slot, ref, empty_rows, empty_cols, "%s %s %s" % (name, phase, slot)).items():
            worst[k] = max(worst.get(k, 0.0), v)

    # (a) start
    dev.call("scaling_compute", 1, 10, 1, 1.0)
    dev.call("scale_problem")
    dev.call("set_initial", capi._ptr(x0), capi._ptr(y0))
    dr, dc = dev.download("DROW", m), dev.download("DCOL", n)
    # (b) the first evaluations: cur = 0, the products (the loop's A^T y is not there yet)
    assert dev.ctl().cur == 0
    x, y = _iterate(dev, "X", "Y", dr, dc)
    np.testing.assert_allclose(x, x0, rtol=4e-16, atol=0)
    np.testing.assert_allclose(y, y0, rtol=4e-16, atol=0)
    for rule in (True, False):
        ref = er.evaluate(p, x, y, rule_finite=rule, eps_p=1e-4, eps_d=1e-4)
        for eps in (1e-4, -1.0):  # (-1: no l-infinity vectors, one finalize launch for both sides)
            before = dev.loop_stats()
            ev = dev.eval(capi.CURRENT, rule_finite=rule, eps_p=eps, eps_d=eps)
            after = dev.loop_stats()
            assert (after["eval_reused_aty"] - before["eval_reused_aty"], after["eval_product"] - before["eval_product"]) == (0, 1)
            phase = "first rule=%d eps=%g" % (rule, eps)
            _check_scalars(ev, ref, eps >= 0, "%s %s" % (name, phase))
            vectors("CURRENT", ref, phase)
    # (c) after an odd number of steps: cur = 1, the average differs from the current iterate
    mx = dev.init_norms()[0]
    dev.call("set_step", 1.0 / mx, 1.0)
    dev.call("compute_aty")
    ctl = dev.run(3)
    assert ctl.error == 0 and ctl.steps_taken == 3 and ctl.cur == 1, (ctl.error, ctl.steps_taken, ctl.cur)
    before = dev.loop_stats()
    cur, avg = dev.major_eval(2, rule_finite=True)
    after = dev.loop_stats()
    twin = layout == "panel" and reuse == 1
    assert (after["eval_reused_aty"] - before["eval_reused_aty"], after["eval_product"] - before["eval_product"]) == ((1, 0) if twin else (0, 1))
    xc, yc = _iterate(dev, "X", "Y", dr, dc)
    xa, ya = _iterate(dev, "AVG_X", "AVG_Y", dr, dc)
    assert np.abs(xc - xa).max() > 1e-3 and np.abs(yc - ya).max() > 1e-3 and np.abs(xc - x).max() > 1e-3
    for slot, ev, (xs, ys) in (("CURRENT", cur, (xc, yc)), ("AVERAGE", avg, (xa, ya))):
        ref = er.evaluate(p, xs, ys, rule_finite=True, eps_p=-1.0, eps_d=-1.0)
        _check_scalars(ev, ref, False, "%s steps %s" % (name, slot))
        vectors(slot, ref, "steps twin" if twin and slot == "CURRENT" else "steps")
    # (e) infeasibility information of the two iterates just evaluated
    for which, (xs, ys) in ((capi.CURRENT, (xc, yc)), (capi.AVERAGE, (xa, ya))):
        got = dev.eval_infeasibility(which, rule_finite=True)
        orc = orcbind.evaluate_infeasibility(p, xs, ys, finite_bounds_rule=True)
        for k in orc:
            assert got[k] == pytest.approx(orc[k], rel=1e-10, abs=1e-12), (name, which, k)
    # (d) the last restart point: restart to the average, two more steps, so that the anchor is neither the current iterate nor
    #     the average; the other rule, so that a reduced cost landing in the wrong slot shows
    dist = np.zeros(2)
    dev.call("restart", capi.AVERAGE, 0, capi._ptr(dist))
    dev.call("compute_aty")
    ctl = dev.run(5)
    assert ctl.error == 0 and ctl.steps_taken == 5, (ctl.error, ctl.steps_taken)
    cur, avg = dev.major_eval(2, rule_finite=True)
    xl, yl = _iterate(dev, "LAST_RESTART_X", "LAST_RESTART_Y", dr, dc)
    np.testing.assert_array_equal(xl, xa)
    xc, yc = _iterate(dev, "X", "Y", dr, dc)
    xa, ya = _iterate(dev, "AVG_X", "AVG_Y", dr, dc)
    assert min(np.abs(xl - xa).max(), np.abs(xl - xc).max(), np.abs(yl - ya).max(), np.abs(yl - yc).max()) > 1e-4
    kept = {k: dev.download(k, m if k.startswith("AX") else n) for k in ("RC_CURRENT", "RC_AVERAGE", "AX_U_CURRENT", "AX_U_AVERAGE", "ATY_U_CURRENT", "ATY_U_AVERAGE")}
    for eps in (1e-4, -1.0):
        ev = dev.eval(capi.LAST_RESTART, rule_finite=False, eps_p=eps, eps_d=eps)
        _check_scalars(ev, er.evaluate(p, xl, yl, rule_finite=False, eps_p=eps, eps_d=eps), eps >= 0, "%s last-restart eps=%g" % (name, eps))
    for k, v in kept.items():  # (its vectors go to slots of their own, the reduced costs to scratch)
        np.testing.assert_array_equal(dev.download(k, len(v)), v, err_msg=k)
    # ... and the slots of the other two still hold what the evaluation in front wrote (cur is 1 again: the product or its twin)
    for slot, ev, (xs, ys) in (("CURRENT", cur, (xc, yc)), ("AVERAGE", avg, (xa, ya))):
        ref = er.evaluate(p, xs, ys, rule_finite=True, eps_p=-1.0, eps_d=-1.0)
        _check_scalars(ev, ref, False, "%s restarted %s" % (name, slot))
        vectors(slot, ref, "restarted")
    dev.close()
    print("WORST %s reuse=%d ax=%.3f aty=%.3f rc=%.3f" % (name, reuse, worst["ax"], worst["aty"], worst["rc"]))


@pytest.mark.parametrize("name", list(VARIANTS))
def test_evaluation_against_the_reference(name, monkeypatch):
    _evaluations(name, 1, monkeypatch)
    if VARIANTS[name][0] == "panel":  # once more with the product where the twin ran
        _evaluations(name, 0, monkeypatch)
