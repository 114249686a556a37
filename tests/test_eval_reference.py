"""CPU: the extended-precision restatement of the convergence evaluation (tests/eval_reference.py) against numbers worked out by hand
and against the C oracle, on the LPs tests/test_eval_layouts_gpu.py evaluates on the device -- and the condition on those inputs that
keeps the GPU test from excluding its way past a failure (hardly any column may sit on a reduced-cost tie)."""
import numpy as np
import pytest

import eval_reference as er
from eval_lps import EMPTY_COLS, LONG_COLS, LONG_ROWS, SEEDS, WIDE_N, edge_lp
from oracle import orcbind

INF = np.inf
# (long_col, dense, seed[, columns]): what the GPU test builds
LPS = [(4500, False, SEEDS[0]), (2400, False, SEEDS[0]), (4500, True, SEEDS[1]), (2400, True, SEEDS[1]), (2400, False, SEEDS[0], WIDE_N)]
LP_IDS = ["col4500", "col2400", "dense-col4500", "dense-col2400", "col2400-60000-columns"]


@pytest.fixture(scope="module", params=LPS, ids=LP_IDS)
def lp(request):
    return request.param, edge_lp(*request.param)


def test_long_double_is_extended():
    """x86 and most others: a 64-bit significand; elsewhere the reference computes in exact rationals"""
    assert er.LONGDOUBLE_IS_EXTENDED == bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)


@pytest.mark.parametrize("exact", [False, True], ids=["longdouble", "fractions"])
def test_identity_lp_by_hand(exact):
    """the identity LP of test_per_constraint_residual_identity_lp: x = (0.02, 0.03, 0.1) against rhs 0, the largest residual is 0.1"""
    if not exact and not er.LONGDOUBLE_IS_EXTENDED:
        exact = True
    p = dict(m=3, n=3, offsets=[0, 1, 2, 3], indices=[0, 1, 2], values=[1.0, 1.0, 1.0], c=[0.0, 0.0, 0.0],
             lo=[0.0, 0.0, 0.0], hi=[0.0, 0.0, 0.0], lb=[0.02, 0.03, 0.1], ub=[0.02, 0.03, 0.1])
    x = np.array([0.02, 0.03, 0.1])
    r = er.evaluate(p, x, np.zeros(3), eps_p=0.0, eps_d=0.0, exact=exact)
    assert r["LINF_PRES_REL"] == 0.1 and r["LINF_DRES_REL"] == 0.0
    assert r["PRES2"] == pytest.approx(0.0113, rel=1e-15) and r["X2"] == pytest.approx(0.0113, rel=1e-15)
    assert r["CX"] == r["DUAL_SUM"] == r["DRES2"] == r["Y2"] == 0.0
    np.testing.assert_array_equal(r["ax"], x)
    np.testing.assert_array_equal(r["rc"], 0.0)
    assert r["g_is_zero"].all() and not r["near_tie"].any()
    np.testing.assert_array_equal(r["bound_ax"], 17 * 2.0 ** -53 * x)


@pytest.mark.parametrize("exact", [False, True], ids=["longdouble", "fractions"])
def test_two_by_three_lp_by_hand(exact):
    """A = [1 2 0; 0 -1 3], x = (1, 1/2, 1), y = (1/2, -1): every number is a dyadic rational, so the expected values are exact.
       A x = (2, 5/2) against (-inf, 3/2] and [3, 4]: violations 1/2 (above) and 1/2 (below)
       A^T y = (1/2, 2, -3), c = (1, 2, -1): g = (1/2, 0, 2); bounds [3, inf), [0, 5], (-inf, 3]
         column 0: g > 0 takes lb = 3: finite, so rc = g under the finite-bounds rule; |x - 3| = 2 > |x| = 1, so rc = 0 under the other
         column 1: g == 0
         column 2: g > 0 takes lb = -inf: rc = 0 under both rules, the dual residual is 2
       sum B(y) = 0 (y_0 > 0, lo = -inf) + (-1)(4) = -4;  sum B(rc) = (1/2)(3) under the finite-bounds rule, 0 under the other"""
    if not exact and not er.LONGDOUBLE_IS_EXTENDED:
        exact = True
    p = dict(m=2, n=3, offsets=[0, 2, 4], indices=[0, 1, 1, 2], values=[1.0, 2.0, -1.0, 3.0], c=[1.0, 2.0, -1.0],
             lo=[-INF, 3.0], hi=[1.5, 4.0], lb=[3.0, 0.0, -INF], ub=[INF, 5.0, 3.0])
    x, y = np.array([1.0, 0.5, 1.0]), np.array([0.5, -1.0])
    want = {True: dict(CX=1.0, X2=2.25, Y2=1.25, PRES2=0.5, DRES2=4.0, DUAL_SUM=-2.5, LINF_PRES_REL=0.125, LINF_DRES_REL=2.25),
            False: dict(CX=1.0, X2=2.25, Y2=1.25, PRES2=0.5, DRES2=4.25, DUAL_SUM=-4.0, LINF_PRES_REL=0.125, LINF_DRES_REL=2.25)}
    for rule in (True, False):
        r = er.evaluate(p, x, y, rule_finite=rule, eps_p=0.25, eps_d=0.25, exact=exact)
        assert {k: r[k] for k in er.SCALARS} == want[rule], rule
        np.testing.assert_array_equal(r["ax"], [2.0, 2.5])
        np.testing.assert_array_equal(r["aty"], [0.5, 2.0, -3.0])
        np.testing.assert_array_equal(r["absax"], [2.0, 3.5])
        np.testing.assert_array_equal(r["absaty"], [0.5, 2.0, 3.0])
        np.testing.assert_array_equal(r["rc"], [0.5 if rule else 0.0, 0.0, 0.0])
        np.testing.assert_array_equal(r["g_is_zero"], [False, True, False])
        assert not r["near_tie"].any()
        np.testing.assert_array_equal(r["bound_ax"], 18 * 2.0 ** -53 * np.array([2.0, 3.5]))
        np.testing.assert_array_equal(r["bound_aty_prod"], 2.0 ** -53 * np.array([17 * 0.5, 18 * 2.0, 17 * 3.0]))
        np.testing.assert_array_equal(r["bound_aty"], 2.0 ** -53 * np.array([17 * 1.5, 18 * 4.0, 17 * 4.0]))
        # without the l-infinity request (a negative eps) both are reported as 0
        assert er.evaluate(p, x, y, rule_finite=rule, eps_p=-1.0, eps_d=-1.0, exact=exact)["LINF_DRES_REL"] == 0.0
    # a tie: g = 2^-60 is below the column's bound, so its sign -- and with it the bound it picks -- is not determined
    q = dict(p, c=[0.5 + 2.0 ** -60, 2.0, -1.0])
    np.testing.assert_array_equal(er.evaluate(q, x, y, exact=exact)["near_tie"], [False, False, False])  # (0.5 + 2^-60 rounds to 0.5)
    q = dict(p, c=[0.5 + 2.0 ** -52, 2.0, -1.0])
    np.testing.assert_array_equal(er.evaluate(q, x, y, exact=exact)["near_tie"], [True, False, False])
    # ... and under the other rule |x - bv| against |x|: x = 3/2 (1 + 2^-52) against bv = 3 misses |x| by a few ulps, under 16 u |x|
    xt = np.array([1.5 * (1 + 2.0 ** -52), 0.5, 1.0])
    np.testing.assert_array_equal(er.evaluate(p, xt, y, rule_finite=False, exact=exact)["near_tie"], [True, False, False])
    np.testing.assert_array_equal(er.evaluate(p, xt, y, rule_finite=True, exact=exact)["near_tie"], [False, False, False])
    xt[0] = 1.5  # |x - bv| == |x| exactly: no tie, compared
    np.testing.assert_array_equal(er.evaluate(p, xt, y, rule_finite=False, exact=exact)["near_tie"], [False, False, False])


def test_edge_lp_holds_what_it_promises(lp):
    (long_col, dense), (p, x, y) = lp[0][:2], lp[1]
    m, n = p["m"], p["n"]
    rlen, clen = np.diff(p["offsets"]), np.bincount(p["indices"], minlength=n)
    assert (rlen[::97] == 0).all() and (rlen == 0).sum() >= 60
    for r, l in LONG_ROWS.items():
        assert l <= rlen[r] <= l + 3  # (a long column may add an entry)
    assert [int(clen[c]) for c in LONG_COLS] == [400, long_col, 129]  # (over 128: cooperative; 4500 is over 4096: a workgroup of its own)
    assert (clen[list(EMPTY_COLS)] == 0).all() and len(EMPTY_COLS) >= 20
    assert (p["c"][list(EMPTY_COLS[::2])] == 0).all() and (p["c"][list(EMPTY_COLS[1::2])] != 0).all()
    if dense:
        runs = [np.diff(p["indices"][p["offsets"][r]:p["offsets"][r + 1]]) for r in (10, 3500)]
        assert [len(d) + 1 for d in runs] == [300, 5000] and all((d == 1).all() for d in runs)
    lo, hi, lb, ub = (p[k] for k in ("lo", "hi", "lb", "ub"))
    row_kinds = [np.isinf(lo) & np.isfinite(hi), np.isfinite(lo) & np.isinf(hi), lo == hi, np.isinf(lo) & np.isinf(hi),
                 np.isfinite(lo) & np.isfinite(hi) & (lo < hi)]
    col_kinds = [np.isinf(lb) & np.isinf(ub), np.isinf(lb) & (ub == 5.0), (lb == 0.0) & np.isinf(ub), (lb == 1.5) & (ub == 1.5),
                 (lb == 0.0) & (ub == 5.0)]
    assert [int(k.sum()) for k in row_kinds] == [m // 5] * 5 and [int(k.sum()) for k in col_kinds] == [n // 5] * 5
    assert (x[col_kinds[3]] == 1.5).all() and 0.2 < (x == 0).mean() < 0.3
    assert (y[row_kinds[0]] > 0).any() and (y[row_kinds[1]] < 0).any() and (y[row_kinds[3]] != 0).all()  # wrong-signed duals stay


@pytest.mark.parametrize("rule", [True, False], ids=["finite-bounds-rule", "reduced-cost-rule"])
def test_reference_against_the_oracle(lp, rule):
    """the oracle is double precision and sums left to right: scalars at rel 1e-12, reduced costs within the derived bound"""
    _, (p, x, y) = lp
    ref = er.evaluate(p, x, y, rule_finite=rule, eps_p=1e-4, eps_d=1e-4)
    orc = orcbind.evaluate(p, x, y, finite_bounds_rule=rule, rel_primal_tol=1e-4, rel_dual_tol=1e-4)
    assert ref["CX"] == pytest.approx(orc["primal_objective"], rel=1e-12)
    assert ref["DUAL_SUM"] == pytest.approx(orc["dual_objective"], rel=1e-12)
    assert np.sqrt(ref["PRES2"]) == pytest.approx(orc["l2_primal_residual"], rel=1e-12)
    assert np.sqrt(ref["DRES2"]) == pytest.approx(orc["l2_dual_residual"], rel=1e-12)
    assert np.sqrt(ref["X2"]) == pytest.approx(orc["l2_x"], rel=1e-12)
    assert np.sqrt(ref["Y2"]) == pytest.approx(orc["l2_y"], rel=1e-12)
    assert ref["LINF_PRES_REL"] == pytest.approx(orc["linf_rel_primal_residual"], rel=1e-12)
    assert ref["LINF_DRES_REL"] == pytest.approx(orc["linf_rel_dual_residual"], rel=1e-12)
    assert min(ref["PRES2"], ref["DRES2"], ref["LINF_PRES_REL"], ref["LINF_DRES_REL"]) > 0.0
    # a condition on the inputs, not a measurement: the GPU test compares every column outside near_tie
    assert ref["near_tie"].mean() <= 0.005
    keep = ~ref["near_tie"]
    err = er.abs_err(ref, "rc", orc["reduced_cost"])
    assert er.worst_ratio(err, ref["bound_aty"], keep) <= 1.0
    assert (orc["reduced_cost"][ref["g_is_zero"]] == 0.0).all() and ref["g_is_zero"].sum() >= len(EMPTY_COLS) // 2
    # the oracle's own products against the bounds (its sums are one of the trees the bound covers)
    to, ti, tv = orcbind.transpose(p["m"], p["n"], p["offsets"], p["indices"], p["values"])
    assert er.worst_ratio(er.abs_err(ref, "ax", orcbind.spmv(p["offsets"], p["indices"], p["values"], x)), ref["bound_ax"]) <= 1.0
    assert er.worst_ratio(er.abs_err(ref, "aty", orcbind.spmv(to, ti, tv, y)), ref["bound_aty_prod"]) <= 1.0
    # both decisions of each rule occur, on columns that are compared
    assert (ref["rc"][keep] != 0).sum() > 500 and ((ref["rc"] == 0) & ~ref["g_is_zero"] & keep).sum() > 500


def test_wide_gather_free_bins_hold_the_wider_lp_only():
    """why the GPU test's pb-wide id has 60000 columns: the host construction of the wide bins (build_pb_wide through its CPU walk,
    pdlpdev_debug_pb_wide_host) refuses both sides of the 6000 x 6000 LP and holds both sides of the 6000 x 60000 one, serial rows
    included, with products equal to the left-to-right sums"""
    import ctypes as C
    from cuopt_amd import capi
    walk = capi.lib.pdlpdev_debug_pb_wide_host
    walk.restype = C.c_int

    def side(rows, cols, off, idx, val, vec):
        out, info = np.zeros(rows), np.zeros(8, np.int64)
        rc = walk(C.c_int32(rows), C.c_int32(cols), capi._ptr(off), capi._ptr(idx), capi._ptr(val), capi._ptr(vec), capi._ptr(out), info.ctypes.data_as(C.c_void_p))
        return rc, out, info

    for n, held in ((6000, False), (WIDE_N, True)):
        p, x, y = edge_lp(2400, False, SEEDS[0], n=n)
        off, idx, val = capi._i32(p["offsets"]), capi._i32(p["indices"]), capi._f64(p["values"])
        to, ti, tv = orcbind.transpose(p["m"], n, off, idx, val)
        for rows, cols, o, i, v, vec in ((p["m"], n, off, idx, val, x), (n, p["m"], to, ti, tv, y)):
            rc, out, info = side(rows, cols, o, i, v, np.ascontiguousarray(vec))
            assert (rc == 0) == held, (n, rows, rc)
            if held:
                assert info[1] == -(-rows // 8192) and info[4] >= 1  # bins of 8192 rows; rows summed by single lanes
                np.testing.assert_array_equal(out, orcbind.spmv(o, i, v, vec))
