"""CPU: tests/frame_reference.py and tests/frame_cases.py proven without a GPU -- the hand LP in exact rationals, the scaling restatement
against the C oracle bit for bit, the derived bounds against float64 sums in four orders, the branches the cases reach, and that every
check of tests/test_frame_gpu.py can fail."""
import math
from fractions import Fraction as F

import numpy as np
import pytest

import frame_cases as fc
import frame_reference as fr
from attempt_reference import Structure, bits_equal
from eval_lps import LONG_ROWS
from eval_reference import U
from oracle import orcbind

INF = np.inf


def _struct(p):
    return Structure(p["m"], p["n"], p["offsets"], p["indices"])


# ---- the hand LP -----------------------------------------------------------------------------------------------------------------------
def _close(got, exact, roundings):
    """a float64 against an exact rational: within `roundings` relative roundings of u (first order, doubled for the second)"""
    return abs(F(float(got)) - exact) <= 2 * roundings * F(U) * abs(exact)


def test_hand_lp_in_exact_rationals():
    """A = [[4, 0], [0, 16], [2, 16]].  Ruiz pass 1: row maxima (4, 16, 16), column maxima (4, 16), all exact squares, so
    D_r = (1/2, 1/4, 1/4), D_c = (1/2, 1/4) EXACTLY and D_r A D_c = [[1, 0], [0, 1], [1/4, 1]]; its row and column maxima are 1: every
    further Ruiz pass divides by sqrt(1).  Pock-Chambolle: row sums (1, 1, 5/4), column sums (1 + 1/4, 1 + 1) = (5/4, 2), so
    D_r^2 = (1/4, 1/16, 1/16 / (5/4)) = (1/4, 1/16, 1/20) and D_c^2 = (1/4 / (5/4), 1/16 / 2) = (1/5, 1/32).
    Squares of everything behind it are rational: a_ij^2 D_r,i^2 D_c,j^2, c_j^2 D_c,j^2, b_i^2 D_r,i^2."""
    p, x0, y0 = fc.hand()
    S = _struct(p)
    ones_m, ones_n, vals = np.ones(3), np.ones(2), p["values"]
    dr1, dc1 = fr.scaling_pass(S, vals, ones_m, ones_n, False)
    assert dr1.tolist() == [0.5, 0.25, 0.25] and dc1.tolist() == [0.5, 0.25]
    assert ((vals * dr1[S.rows]) * dc1[S.idx]).tolist() == [1.0, 1.0, 0.25, 1.0]
    dr2, dc2 = fr.scaling_pass(S, vals, dr1, dc1, False)
    assert bits_equal(dr2, dr1) and bits_equal(dc2, dc1)
    for iterations in (1, 5, 10):
        dr, dc = fr.scaling(p, iterations, False)
        assert bits_equal(dr, dr1) and bits_equal(dc, dc1)
    # Pock-Chambolle behind it: d / sqrt(sum), a square root and a division
    dr2_exact, dc2_exact = [F(1, 4), F(1, 16), F(1, 20)], [F(1, 5), F(1, 32)]
    for iterations in (5, 10):
        dr, dc = fr.scaling(p, iterations, True)
        assert dr[0] == 0.5 and dr[1] == 0.25  # (sums of 1: nothing is rounded)
        assert all(_close(F(float(v)) ** 2, e, 4) for v, e in zip(dr, dr2_exact)), dr
        assert all(_close(F(float(v)) ** 2, e, 4) for v, e in zip(dc, dc2_exact)), dc
    prob = fr.scaled_problem(p, dr, dc, S)
    # the scaled values (CSR order: (0,0), (1,1), (2,0), (2,1)) and A^T's (column 0: rows 0, 2; column 1: rows 1, 2)
    a2 = [F(16) * F(1, 4) * F(1, 5), F(256) * F(1, 16) * F(1, 32), F(4) * F(1, 20) * F(1, 5), F(256) * F(1, 20) * F(1, 32)]
    assert a2 == [F(4, 5), F(1, 2), F(1, 25), F(2, 5)]
    assert all(_close(F(float(v)) ** 2, e, 12) for v, e in zip(prob["A_VALUES"], a2))
    assert all(_close(F(float(v)) ** 2, e, 12) for v, e in zip(prob["AT_VALUES"], [a2[0], a2[2], a2[1], a2[3]]))
    assert np.isneginf(prob["LO"][0]) and np.isposinf(prob["HI"][1]) and np.isneginf(prob["LB"][1]) and np.isposinf(prob["UB"][1])
    assert prob["LB"][0] == 0.0 and _close(F(float(prob["UB"][0])) ** 2, F(25) / F(1, 5), 8)
    # the norms: max|A|^2 = 4/5; sum c^2 D_c^2 = 9/5 + 64/32 = 19/5; b = (6, 2, 4): 36/4 + 4/16 + 16/20 = 201/20
    mx, c2, b2 = fr.init_norms(prob)
    assert _close(F(mx) ** 2, F(4, 5), 12)
    assert _close(F(float(c2[0])), F(19, 5), 12) and _close(F(float(b2[0])), F(201, 20), 12)
    assert fr.combine_bounds(p["lo"], p["hi"]).tolist() == [6.0, 2.0, 4.0]
    # ... of the caller's problem: sum c^2 = 73, sum b^2 = 56, exactly
    assert float(fr.sum_squares(p["c"])[0]) == 73.0 and float(fr.sum_squares(fr.combine_bounds(p["lo"], p["hi"]))[0]) == 56.0
    nc, nb = fr.problem_norms(p["c"], p["lo"], p["hi"])
    assert _close(F(float(nc[0])) ** 2, F(73), 4) and _close(F(float(nb[0])) ** 2, F(56), 4)
    # the start, the clamp and the way back
    x, y = fr.to_scaled_start(x0, y0, dr, dc)
    assert _close(F(float(x[0])) ** 2, F(49) * 5, 8) and _close(F(float(y[2])) ** 2, F(4) * 20, 8) and y[0] == 1.0 and y[1] == -4.0
    xc = fr.clamp(x, prob["LB"], prob["UB"])
    assert xc[0] == prob["UB"][0] and xc[1] == x[1]
    ux, uy = fr.unscaled(x, y, dr, dc)
    np.testing.assert_allclose(ux, x0, rtol=4 * U, atol=0)
    np.testing.assert_allclose(uy, y0, rtol=4 * U, atol=0)


# ---- two independent statements of the scaling -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", list(fc.PRESETS))
@pytest.mark.parametrize("case", list(fc.CPU_CASES))
def test_scaling_restatement_equals_the_oracle(case, preset):
    p = fc.CPU_CASES[case]()[0]
    h = orcbind.hyper_preset({"ruiz10-pc": 1, "ruiz5-pc": 2}[preset])
    H = orcbind.H
    assert (h[H["ORC_H_DO_RUIZ"]], h[H["ORC_H_RUIZ_ITERATIONS"]], h[H["ORC_H_DO_POCK_CHAMBOLLE"]], h[H["ORC_H_ALPHA_POCK_CHAMBOLLE"]]) == (1, fc.PRESETS[preset], 1, 1.0)
    dr, dc = fr.scaling(p, fc.PRESETS[preset], True)
    odr, odc = orcbind.compute_scaling(p["m"], p["n"], p["offsets"], p["indices"], p["values"], h)
    assert bits_equal(dr, odr), int(np.argmax(dr != odr))
    assert bits_equal(dc, odc), int(np.argmax(dc != odc))
    S = _struct(p)
    assert (dr[S.len_r == 0] == 1.0).all() and (dc[S.len_c == 0] == 1.0).all()
    # A^T is the stable transposition: what the oracle (and the device) is handed
    to, ti, tv = orcbind.transpose(p["m"], p["n"], p["offsets"], p["indices"], p["values"])
    assert np.array_equal(to, S.t_off) and np.array_equal(ti, S.t_rows) and bits_equal(tv, np.asarray(p["values"])[S.order])


def test_left_to_right_sums_are_left_to_right():
    rng = np.random.default_rng(3)
    lens = np.array([0, 1, 5, 0, 300, 2, 129, 0])
    off = np.concatenate([[0], np.cumsum(lens)])
    v = np.abs(rng.standard_normal(off[-1])) * 10.0 ** rng.integers(-8, 8, size=off[-1])
    got = fr.rows_left_to_right(v, off)
    for r, l in enumerate(lens):
        acc = 0.0
        for k in range(off[r], off[r + 1]):
            acc = acc + v[k]
        assert got[r] == acc
    assert fr.rows_max(v, off)[[0, 3, 7]].tolist() == [0.0, 0.0, 0.0] and fr.rows_max(v, off)[4] == v[off[4]:off[5]].max()


# ---- the bounds hold for float64 sums in any order --------------------------------------------------------------------------------------
def _left_to_right(t):
    acc = 0.0
    for v in t.tolist():
        acc = acc + v
    return acc


def _pairwise(t):
    t = t.copy()
    while len(t) > 1:
        if len(t) % 2:
            t = np.concatenate([t, [0.0]])
        t = t[0::2] + t[1::2]
    return float(t[0]) if len(t) else 0.0


def _strided(t):
    """1024 workgroups of 256 lanes, grid-stride: a lane's terms left to right, the lanes pairwise, the workgroups pairwise"""
    lanes = 1024 * 256
    pad = np.concatenate([t, np.zeros(-len(t) % lanes)]).reshape(-1, lanes)
    acc = np.zeros(lanes)
    for row in pad:
        acc = acc + row
    acc = acc.reshape(1024, 256)
    while acc.shape[1] > 1:
        acc = acc[:, 0::2] + acc[:, 1::2]
    return _pairwise(acc[:, 0])


ORDERS = {"left-to-right": _left_to_right, "reversed": lambda t: _left_to_right(t[::-1]), "pairwise": _pairwise, "strided": _strided}


def _vectors():
    """(name, terms' factors): the sums the GPU test bounds, on the scaled edge LP and on the wrap LP"""
    p, x0, y0 = fc.edge("stream")
    dr, dc = fr.scaling(p, 10, True)
    prob = fr.scaled_problem(p, dr, dc)
    pw, xw, yw = fc.wrap()
    yield "edge c2", prob["C"], prob["C"]
    b = fr.combine_bounds(prob["LO"], prob["HI"])
    yield "edge b2", b, b
    x, y = fr.to_scaled_start(fc.start(p, x0), y0, dr, dc)
    yield "edge x2", x, x
    yield "edge x.c", x, prob["C"]
    yield "wrap c2", pw["c"], pw["c"]
    yield "wrap x.c", xw, pw["c"]
    bw = fr.combine_bounds(pw["lo"], pw["hi"])
    yield "wrap b2", bw, bw
    yield "1x1", np.array([0.75]), np.array([0.75])


def test_bounds_hold_for_float64_sums_in_four_orders():
    worst = 0.0
    for name, a, b in _vectors():
        entry = fr.sum_squares(a) if a is b else fr.dot(a, b)
        terms = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
        for order, f in ORDERS.items():
            r = fr.ratio(entry, f(terms))
            print("RATIO %s %s %.4f" % (name, order, r))
            worst = max(worst, r)
            assert r <= 1.0, (name, order, r)
        if a is b:  # the norm behind it
            r = fr.ratio(fr.norm_of(entry, len(terms)), math.sqrt(_strided(terms)))
            worst = max(worst, r)
            assert r <= 1.0, (name, "norm", r)
    print("WORST reference-alone %.4f" % worst)
    assert 0.0 < worst <= 1.0


# ---- the cases reach their branches -----------------------------------------------------------------------------------------------------
def _finiteness(lo, hi):
    return {(bool(a), bool(b)) for a, b in zip(np.isfinite(lo), np.isfinite(hi))}


@pytest.mark.parametrize("name", ["stream", "dense-stream", "pb"])
def test_edge_lp_reaches_the_scaling_branches(name):
    p, x0, y0 = fc.edge(name)
    S = _struct(p)
    long_col = 2400 if name == "pb" else 4500
    if name != "dense-stream":  # (the long columns add up to three entries to a long row; the dense twin rebuilds two rows)
        assert all(l <= S.len_r[r] <= l + 3 for r, l in LONG_ROWS.items()), S.len_r[list(LONG_ROWS)]
    assert all((S.len_c == w).any() for w in (129, 400, long_col)), name
    for lens in (S.len_r, S.len_c):
        assert (lens == 0).sum() >= 20 and ((lens > 0) & (lens <= fc.K_LONG_ROW)).any()
        assert ((lens > fc.K_LONG_ROW) & (lens < 140)).any()  # just past kLongRow
        assert ((lens > fc.K_LONG_ROW) & (lens <= fc.K_NNZ_BLOCK)).any() and (lens > fc.K_NNZ_BLOCK).any()  # both sides of kNnzBlock
    assert _finiteness(p["lo"], p["hi"]) == {(False, True), (True, False), (True, True), (False, False)}
    assert (p["lo"] == p["hi"]).any() and ((p["lo"] < p["hi"]) & np.isfinite(p["lo"]) & np.isfinite(p["hi"])).any()
    assert _finiteness(p["lb"], p["ub"]) == {(False, False), (False, True), (True, False), (True, True)} and (p["lb"] == p["ub"]).any()
    # combine_bounds picks either side somewhere
    both = np.isfinite(p["lo"]) & np.isfinite(p["hi"])
    assert (np.abs(p["lo"][both]) > np.abs(p["hi"][both])).any() and (np.abs(p["lo"][both]) < np.abs(p["hi"][both])).any()
    # the start: every column kind above its upper and below its lower bound, fixed columns off their value
    x = fc.start(p, x0)
    kinds = {(bool(a), bool(b)) for a, b in zip(np.isfinite(p["lb"]), np.isfinite(p["ub"]))}
    for kind in kinds:
        sel = (np.isfinite(p["lb"]) == kind[0]) & (np.isfinite(p["ub"]) == kind[1])
        assert not kind[1] or (x[sel] > p["ub"][sel]).any(), kind
        assert not kind[0] or (x[sel] < p["lb"][sel]).any(), kind
        assert ((x[sel] >= p["lb"][sel]) & (x[sel] <= p["ub"][sel])).any(), kind
    fixed = p["lb"] == p["ub"]
    assert (x[fixed] > p["ub"][fixed]).any() and (x[fixed] < p["lb"][fixed]).any()


def test_wrap_lp_is_beyond_both_wrap_points():
    p, x0, y0 = fc.wrap()
    S = _struct(p)
    nnz = len(p["values"])
    assert p["n"] > fc.ELEMENTWISE_WRAP and nnz > fc.REDUCE_WRAP and p["n"] % 256 != 0 and nnz % 256 != 0
    assert p["n"] - fc.ELEMENTWISE_WRAP < 2048 * 256 and 2000 <= p["m"] <= 5000 and nnz < p["n"]
    assert (S.len_r == 0).sum() == 10 and (S.len_c == 0).sum() == p["n"] // 10 and S.len_c.max() == 1
    assert ((S.len_r > 0) & (S.len_r <= fc.K_LONG_ROW)).any() and (S.len_r > fc.K_LONG_ROW).any()
    assert _finiteness(p["lo"], p["hi"]) == {(False, True), (True, False), (True, True), (False, False)}
    assert _finiteness(p["lb"], p["ub"]) == {(False, False), (False, True), (True, False), (True, True)}
    # ... beyond the wrap point too: the second trip of the element-wise kernels sees every column kind
    tail = slice(fc.ELEMENTWISE_WRAP, None)
    assert _finiteness(p["lb"][tail], p["ub"][tail]) == {(False, False), (False, True), (True, False), (True, True)}
    x = fc.start(p, x0)
    assert (x[tail] > p["ub"][tail]).any() and (x[tail] < p["lb"][tail]).any()


def test_small_cases():
    p, x0, y0 = fc.zero_c()
    assert fr.sum_squares(p["c"]) == (0.0, 0.0) and fr.sum_squares(fr.combine_bounds(p["lo"], p["hi"]))[0] > 0
    p, x0, y0 = fc.free_rows()
    assert float(fr.sum_squares(fr.combine_bounds(p["lo"], p["hi"]))[0]) == 0.0 and float(fr.sum_squares(p["c"])[0]) > 0
    p, x0, y0 = fc.one_by_one()
    assert (p["m"], p["n"], len(p["values"])) == (1, 1, 1) and x0[0] > p["ub"][0]
    from cuopt_amd import capi
    p, x0, y0 = fc.resident()
    assert capi.resident_tier(p["m"], p["n"], len(p["values"])) >= 0


# ---- the checks can fail ----------------------------------------------------------------------------------------------------------------
def test_corrupted_outputs_are_rejected():
    p, x0, y0 = fc.edge("stream")
    S = _struct(p)
    dr, dc = fr.scaling(p, 10, True, S)
    prob = fr.scaled_problem(p, dr, dc, S)
    # one long column's Pock-Chambolle sum added in reverse
    j = int(np.argmax(S.len_c))
    assert S.len_c[j] == 4500
    bad_dr, bad_dc = fr.scaling(p, 10, True, S, corrupt=("reverse_column", j))
    assert bits_equal(bad_dr, dr) and not bits_equal(bad_dc, dc) and (bad_dc != dc).sum() == 1 and bad_dc[j] != dc[j]
    # AT_VALUES multiplied in A's order
    bad = fr.scaled_problem(p, dr, dc, S, corrupt="at_in_a_order")
    assert not bits_equal(bad["AT_VALUES"], prob["AT_VALUES"]) and bits_equal(bad["AT_VALUES"], prob["A_VALUES"][S.order])
    np.testing.assert_allclose(bad["AT_VALUES"], prob["AT_VALUES"], rtol=5 * U, atol=0)  # (two roundings each: nothing coarser than the bits would see it)
    # b2 from lo alone; hi ignored where lo is finite
    mx, c2, b2 = fr.init_norms(prob)
    for corrupt in ("b2_from_lo", "hi_ignored"):
        wrong = float(fr.init_norms(prob, corrupt=corrupt)[2][0])
        assert fr.ratio(b2, wrong) > 1e6, corrupt
    # y unscaled with D_c
    x, y = fr.to_scaled_start(x0, y0, dr, dc)
    good, bad = fr.unscaled(x, y, dr, dc), fr.unscaled(x, y, dr, dc, corrupt="y_with_dc")
    assert bits_equal(good[0], bad[0]) and not bits_equal(good[1], bad[1])
    # the average left unclamped
    xs = fr.to_scaled_start(fc.start(p, x0), y0, dr, dc)[0]
    assert not bits_equal(fr.clamp(xs, prob["LB"], prob["UB"]), xs)
    free = np.isinf(p["lb"]) & np.isinf(p["ub"])
    assert bits_equal(fr.clamp(xs, prob["LB"], prob["UB"])[free], xs[free])
    # a sum off by a relative 1e-9 (the suite's own tolerance for whole solves) is far outside the bound
    assert fr.ratio(c2, float(c2[0]) * (1.0 + 1e-9)) > 1e3
