"""GPU: dense row segments at their segment, chunk, tile and fusion boundaries (cuopt_amd/csrc/kernels_dense.hip: find_dense_segments,
k_dense_rows / k_dense_rows_finish / k_dense_cols; spmv_panel.hpp: the own-row workgroups and the column epilogue that add the
segments themselves; pdlp_create.hip: own_segments, column_segments, the candidate-row scan of the device-side set-up).

The LPs, the plain Python model of the segment rule, the longdouble reference and the bound are tests/dense_cases.py's (checked on the
host by tests/test_dense_cases.py).  Every product is compared PER ELEMENT with
    |got - ref| <= (gamma_L + L * 2^-64) * sum|a_k||v_k|,    gamma_L = L u / (1 - L u), u = 2^-53, L = the row's / column's entries
which holds for any order of the L products' additions, with or without fused multiply-adds (dense_cases' docstring): no tolerance
is guessed.  On top of that
  * empty rows and empty columns are exactly 0;
  * where no segment reaches, the products equal the oracle's left-to-right sums (orcbind.spmv) bit for bit -- on the rows and columns
    each layout sums left to right (exact_lengths, from the id's layout and knobs alone): of any length in the gather-free layout,
    of at most 128 entries (kLongRow) in the stream, row-sum panel and jagged layouts, whose longer rows are summed by a fixed tree
    (the rounding contract at the head of pdlp_kernels.hpp), none in the long-tail panels, which deal EVERY row by nonzero
    (spmv_panel.hpp).  That is all the existing dense test could see, whose untouched rows are all short.  Row 4 of boundary_lp (a
    run of 255, left sparse) outside the gather-free id, and everything in the long-tail id, are held to the bound instead;
  * the layout is asserted on both sides, dense_info() against the model, and for the panels bits 8 and 9 of layout_checksums()[15]:
    "A's own-row workgroups add the segments" and "the A^T epilogue adds them" (clear: k_dense_cols runs in front).

Worst ratios are printed per case (WORST ...)."""
import time

import numpy as np
import pytest
from conftest import set_tune

import dense_cases as dc
from cuopt_amd import capi
from oracle import orcbind
from test_eval_layouts_gpu import VARIANTS

pytestmark = pytest.mark.gpu

LAYOUT_IDS = ["dense-stream", "dense-panel-rows", "dense-panel-longtail", "dense-jag-8", "dense-pb"]
SHORT = 128  # kLongRow: rows up to here are summed left to right, bit-identical to the oracle


@pytest.fixture(autouse=True)
def multi_launch_kernels(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")  # (a context with dense segments is never resident; the threshold LP without them would be)


_cases = {}


def case(name):
    """(p, model, [(x, y, reference, oracle's A x, oracle's A^T y)] for the two vector pairs): built once, shared, read-only"""
    if name not in _cases:
        kind, _, arg = name.partition("-")
        p = dict(boundary=dc.boundary_lp, abut=dc.abut_lp)[kind]() if not arg else dict(stack=dc.stack_lp, threshold=dc.threshold_lp)[kind](int(arg))
        _cases[name] = (p, dc.model(p), _references(p, p["values"]))
        for a in p.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _cases[name]


def _references(p, values, at_values=None):
    """(at_values: what A^T holds of each entry, in p's order, where that is not `values` itself)"""
    to, ti, tv = orcbind.transpose(p["m"], p["n"], p["offsets"], p["indices"], values if at_values is None else at_values)
    return [(x, y, dc.reference_products(p, x, y, values, at_values), orcbind.spmv(p["offsets"], p["indices"], values, x), orcbind.spmv(to, ti, tv, y))
            for x, y in dc.vectors(p, 7)]


def open_layout(name, p, monkeypatch, dense=1, **tune):
    """a context in the layout and with the knobs of test_eval_layouts_gpu's id `name`; the layout asserted on both sides"""
    layout, knobs = VARIANTS[name][:2]
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    set_tune(monkeypatch, dense=dense, **knobs, **tune)
    dev = capi.Device(p)
    assert_layout(name, dev)
    return dev


def assert_layout(name, dev):
    layout, knobs = VARIANTS[name][:2]
    lay = dev.layout()
    print("LAYOUT %s %s" % (name, lay))
    assert lay["A"]["layout"] == lay["At"]["layout"] == layout, lay
    if layout == "panel":
        assert lay["A"]["row_sums"] == lay["At"]["row_sums"] == ("by_nonzero" if knobs["panel_seg"] else "by_row"), lay


def flags(dev):
    f = int(dev.layout_checksums()[15])
    return dict(own_rows_add=bool(f >> 8 & 1), epilogue_adds=bool(f >> 9 & 1))


def exact_lengths(name):
    """the longest row id `name`'s layout sums left to right, bit-identical to the oracle (from VARIANTS alone, not from the context)"""
    layout, knobs = VARIANTS[name][:2]
    return 0 if layout == "panel" and knobs["panel_seg"] else 2 ** 31 if layout == "pb" else SHORT


def check(dev, name, p, mod, refs, tag):
    """both products for both vector pairs, in id `name`'s layout -> the worst ratios"""
    worst, longest = {}, exact_lengths(name)
    for k, (x, y, ref, orc_ax, orc_aty) in enumerate(refs):
        ax, aty = dev.spmv(x, False, p["m"]), dev.spmv(y, True, p["n"])
        exact_ax = (~mod["rows_touched"] & (ref["len_ax"] <= longest), orc_ax)
        exact_aty = (~mod["cols_touched"] & (ref["len_aty"] <= longest), orc_aty)
        try:
            got = dc.check_products(p, mod, ref, ax, aty, exact_ax, exact_aty)
        except AssertionError as e:
            raise AssertionError("%s, vectors %d: %s" % (tag, k, e)) from None
        for key, v in got.items():
            worst[key] = max(worst.get(key, 0.0), v)
    print("WORST %s %s" % (tag, " ".join("%s=%.3f" % kv for kv in worst.items())))
    return worst


# ---- a. the boundary LP in five layouts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAYOUT_IDS)
def test_boundary_lp_in_every_layout(name, monkeypatch):
    p, mod, refs = case("boundary")
    dev = open_layout(name, p, monkeypatch)
    assert dev.dense_info() == dict(on=True, segments=mod["segments"], entries=mod["entries"])
    if VARIANTS[name][0] == "panel":  # 17 segments <= 32 in any panel, no column with a workgroup of its own
        assert flags(dev) == dict(own_rows_add=True, epilogue_adds=True)
    check(dev, name, p, mod, refs, "boundary " + name)
    dev.close()


# ---- b. the scaled matrix ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense-stream", "dense-panel-rows"])
def test_scaled_boundary_lp(name, monkeypatch):
    """sync_panel_values after scale_problem: the segment values and both hot CSRs re-permuted from the scaled full matrices.  The
    reference is diag(DROW) A diag(DCOL) as scale_problem rounds it: fl(fl(a D_r) D_c) in A, fl(fl(a D_c) D_r) in A^T -- the two may
    differ in the last bit (tests/frame_reference.py), and a bound of one rounding per product has no room for a second matrix: every
    entry is taken with the rounding of the copy the product reads.  This pins where the segments' values come from: they are
    stored once, permuted from A's scaled values, so with segments on A^T y is NOT the product with AT_VALUES bit for bit.  Should
    the column side ever read segment values in A^T's rounding, nothing would be wrong and this reference has to follow"""
    p, mod, _ = case("boundary")
    dev = open_layout(name, p, monkeypatch)
    h, H = orcbind.hyper_preset(1), orcbind.H
    dev.call("scaling_compute", int(h[H["ORC_H_DO_RUIZ"]]), int(h[H["ORC_H_RUIZ_ITERATIONS"]]), int(h[H["ORC_H_DO_POCK_CHAMBOLLE"]]),
             float(h[H["ORC_H_ALPHA_POCK_CHAMBOLLE"]]))
    dev.call("scale_problem")
    dr, dcol = dev.download("DROW", p["m"]), dev.download("DCOL", p["n"])
    assert np.abs(dr - 1.0).max() > 1e-3 and np.abs(dcol - 1.0).max() > 1e-3 and (dr > 0).all() and (dcol > 0).all()
    rows = np.repeat(np.arange(p["m"]), np.diff(p["offsets"]))
    scaled, scaled_t = (p["values"] * dr[rows]) * dcol[p["indices"]], (p["values"] * dcol[p["indices"]]) * dr[rows]
    np.testing.assert_array_equal(dev.download("A_VALUES", len(scaled)), scaled)
    np.testing.assert_array_equal(dev.download("AT_VALUES", len(scaled)), dc.transposed(p, scaled_t)[2])
    assert (scaled != scaled_t).any()
    # a segment's values are stored ONCE, taken from A's matrix (DenseHost::perm), and serve both products: in A^T's product the
    # segment entries carry A's rounding, the sparse remainder A^T's own
    check(dev, name, p, mod, _references(p, scaled, np.where(mod["in_segment"], scaled, scaled_t)), "scaled " + name)
    dev.close()


# ---- c. the 32 / 33 switch of the panel epilogue -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which,epilogue_adds", [("dense-panel-rows", "stack-32", True), ("dense-panel-rows", "stack-33", False),
                                                      ("dense-stream", "stack-33", None), ("dense-panel-rows", "abut", True)])
def test_segments_stacked_over_one_tile(name, which, epilogue_adds, monkeypatch):
    """K segments over the same columns: 32 are the epilogue's, 33 k_dense_cols'; and (abut) 32 that begin where a panel begins, next to
    one that ends there, are still the epilogue's"""
    p, mod, refs = case(which)
    dev = open_layout(name, p, monkeypatch)
    assert dev.dense_info() == dict(on=True, segments=mod["segments"], entries=mod["entries"])
    if epilogue_adds is not None:
        got = flags(dev)
        print("FLAGS %s %s %s" % (which, name, got))
        if which == "abut":  # the cut dense_cases.abut_lp is built around
            w = dev.panel_words("At")
            assert w["panels"] == 2 and w["tile_ptr"][w["slabs"]] - w["tile_ptr"][0] == dc.PANEL_TARGET, (w["panels"], w["tile_ptr"])
        assert got == dict(own_rows_add=True, epilogue_adds=epilogue_adds)
    check(dev, name, p, mod, refs, "%s %s" % (which, name))
    dev.close()


# ---- d. the switch-on rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 1])
def test_the_path_switches_itself_on_at_two_percent(extra, monkeypatch):
    p, mod, refs = case("threshold-%d" % extra)
    monkeypatch.delenv("CUOPT_AMD_SPMV_LAYOUT", raising=False)
    set_tune(monkeypatch, dense=None)
    dev = capi.Device(p)
    info, lay = dev.dense_info(), dev.layout()
    print("THRESHOLD extra=%d %s %s" % (extra, info, lay))
    assert lay["A"]["layout"] == lay["At"]["layout"] == "stream", lay  # (what the unforced choice gives an LP of this size)
    assert mod["on_by_default"] == (extra == 0)
    assert info["on"] == (extra == 0), info
    assert extra or info == dict(on=True, segments=1, entries=256)
    check(dev, "dense-stream", p, mod, refs, "threshold extra=%d" % extra)
    dev.close()


# ---- e. the device-side set-up ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense-stream", "dense-panel-rows"])
@pytest.mark.parametrize("which", ["boundary", "stack-70"])
def test_device_side_setup_is_the_host_path(which, name, monkeypatch):
    """boundary: 14 candidate rows (up to 64: their indices alone come back for the first scan); stack-70: more, the whole index
    array.  That first scan only decides WHETHER there are segments: once it finds some, the set-up scans again on the whole index
    array (the constructions behind it read every row), so the tables compared here come from the full fetch in both cases"""
    p, mod, refs = case(which)
    candidates = int((np.diff(p["offsets"]) >= dc.MIN_RUN).sum())
    assert candidates == 14 if which == "boundary" else candidates > 64
    host = open_layout(name, p, monkeypatch)
    dev = capi.Device(p, analysis=capi.Analysis(p, reorder=False))
    assert_layout(name, dev)
    assert dev.dense_info() == host.dense_info() == dict(on=True, segments=mod["segments"], entries=mod["entries"])
    assert dev.layout() == host.layout()
    np.testing.assert_array_equal(dev.layout_checksums(), host.layout_checksums())
    for x, y, *_ in refs:
        np.testing.assert_array_equal(dev.spmv(x, False, p["m"]), host.spmv(x, False, p["m"]))
        np.testing.assert_array_equal(dev.spmv(y, True, p["n"]), host.spmv(y, True, p["n"]))
    check(dev, name, p, mod, refs, "device set-up %s %s" % (which, name))
    host.close(), dev.close()


# ---- f. a solve ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_solve_is_the_same_with_and_without_the_segments(monkeypatch):
    p, _, _ = case("boundary")
    monkeypatch.delenv("CUOPT_AMD_SPMV_LAYOUT", raising=False)
    got = {}
    for flag in ("0", "1"):
        set_tune(monkeypatch, dense=flag)
        t0 = time.perf_counter()
        r = capi.Solver(p, tol=0.0, iteration_limit=80).advance()
        got[flag] = (r["steps_taken"], r["attempted_steps"], r["num_restarts"], r["primal_objective"], r["step_size"])
        print("SOLVE dense=%s %s %.2f s" % (flag, got[flag], time.perf_counter() - t0))
    assert got["0"][:3] == got["1"][:3] and got["0"][0] > 0
    assert got["0"][3] == pytest.approx(got["1"][3], rel=1e-9) and got["0"][4] == pytest.approx(got["1"][4], rel=1e-9)
