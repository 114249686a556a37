"""CPU: the LPs, the model of the segment rule, the reference products and the bound of tests/test_dense_boundaries_gpu.py
(tests/dense_cases.py) on the host: the LPs are what their generators promise, the model -- a plain Python restatement of the rule's
description -- counts the figures the GPU test compares dense_info() with, the longdouble reference is exact to its own error term
on rows summed in rationals, one float64 numpy.dot per row stays inside the bound, and three deliberately wrong products (a segment's
last chunk, a segment's last tile, a whole segment left out) each FAIL the check, so it bites without a kernel being touched."""
from fractions import Fraction

import numpy as np
import pytest

import dense_cases as dc


@pytest.fixture(scope="module")
def boundary():
    p = dc.boundary_lp()
    return p, dc.model(p)


def _from_table():
    """the segments as BOUNDARY_ROWS itself lists them (no run of the table touches another run or a stray of its row)"""
    return [(r, c0, length) for r, (runs, _) in sorted(dc.BOUNDARY_ROWS.items()) for c0, length in runs if length >= dc.MIN_RUN]


def test_the_boundary_lp_is_what_its_generator_promises(boundary):
    p, mod = boundary
    m, n, off, idx = p["m"], p["n"], np.asarray(p["offsets"], np.int64), np.asarray(p["indices"], np.int64)
    assert (m, n) == (1200, 9001) and n == 35 * 256 + 41
    lens, ordinary = np.diff(off), 0
    for r in range(m):
        cols = idx[off[r]:off[r + 1]]
        assert (np.diff(cols) > 0).all(), "columns strictly increasing in every row"
        if r in dc.BOUNDARY_ROWS:
            runs, strays = dc.BOUNDARY_ROWS[r]
            want = sorted([c for c0, length in runs for c in range(c0, c0 + length)] + list(strays))
            assert cols.tolist() == want, r
        else:
            ordinary += 1
            assert len(cols) <= 12 and (len(cols) == 0 or (cols[0] >= 2 and cols[-1] <= 8599)), r
            assert ordinary % 97 != 0 or len(cols) == 0, r
    assert ordinary == m - 15 and (lens == 0).sum() >= ordinary // 97
    assert set(lens[[r for r in range(m) if r not in dc.BOUNDARY_ROWS]]) == set(range(13)), "every length 0 .. 12 among the ordinary rows"
    assert (p["lb"] == 0).all() and (p["ub"] == 3).all() and (p["hi"] == 50).all() and np.isneginf(p["lo"]).all()
    assert (p["values"] != 0).all()
    # the rule's model on it
    assert mod["segs"] == _from_table()
    got = {k: mod[k] for k in dc.BOUNDARY_FIGURES}
    print("FIGURES boundary_lp", got, "nnz", len(idx))
    assert got == dc.BOUNDARY_FIGURES
    assert mod["on_by_default"]
    assert not mod["rows_touched"][4] and lens[4] == 255, "the run of 255 stays sparse"
    assert mod["cols_touched"][0] and mod["cols_touched"][n - 1] and not mod["cols_touched"][8194:8744].any()
    assert (np.bincount(idx, minlength=n) == 0).any(), "an empty column"
    # the edges the issue names, as the model sees them
    seg_lens = sorted(length for _, _, length in mod["segs"])
    assert {256, 257, 4095, 4096, 4097, 8192, 8193} <= set(seg_lens)
    assert min(c0 for _, c0, _ in mod["segs"]) == 0 and max(c0 + length for _, c0, length in mod["segs"]) == n
    assert (lens >= dc.MIN_RUN).sum() == 14, "the candidate rows of the set-up's scan: up to 64 of them come over on their own"


@pytest.mark.parametrize("K", [32, 33, 70])
def test_the_stack_lp(K):
    p = dc.stack_lp(K)
    mod = dc.model(p)
    assert (p["m"], p["n"]) == (400, 2048)
    assert mod["segs"] == [(r, 512, 256) for r in range(10, 10 + K)]
    assert (mod["tiles_touched"], mod["max_segments_per_tile"], mod["rows_without_remainder"]) == (1, K, K)
    assert np.diff(p["offsets"]).max() == 256 and (np.diff(p["offsets"]) >= dc.MIN_RUN).sum() == K
    assert mod["sparse_per_col"].sum() <= dc.PANEL_TARGET + 400, "A^T's sparse remainder: one or two panels, the tile inside one"


def test_the_abutting_lp_cuts_a_panel_where_one_segment_ends_and_32_begin():
    p = dc.abut_lp()
    mod = dc.model(p)
    assert mod["segs"] == [(5, 256, 256)] + [(r, 512, 256) for r in range(10, 42)]
    t_off = np.concatenate([[0], np.cumsum(mod["sparse_per_col"])])
    assert t_off[512] == dc.PANEL_TARGET and t_off[513] == dc.PANEL_TARGET + 1, "the greedy cut ends the first panel in front of column 512"
    assert t_off[-1] - t_off[512] <= dc.PANEL_TARGET, "... and the second panel takes the rest"
    assert mod["max_segments_per_tile"] == dc.PANEL_SEGS
    assert np.diff(p["offsets"]).max() == 256, "no column or row with a workgroup of its own"


@pytest.mark.parametrize("extra", [0, 1])
def test_the_threshold_lp(extra):
    p = dc.threshold_lp(extra)
    mod = dc.model(p)
    assert len(p["indices"]) == 12800 + extra and mod["segs"] == [(7, 300, 256)]
    assert mod["entries"] * 50 == 12800 and mod["on_by_default"] == (extra == 0)


def test_a_row_that_is_not_strictly_increasing_stays_sparse():
    p = dc.stack_lp(2)
    off, idx = p["offsets"], p["indices"].copy()
    idx[off[10]:off[10] + 2] = idx[off[10]:off[10] + 2][::-1]  # 513, 512, 514, ...
    assert dc.segments(dict(p, indices=idx)) == [(11, 512, 256)]


def _exact_row(values, v, idx):
    return sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(values, v[idx])), Fraction(0))


def test_the_reference_is_exact_to_its_own_error_term(boundary):
    p, _ = boundary
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "numpy.longdouble is no wider than float64 here"
    (x, y), _ = dc.vectors(p, 7)
    ref = dc.reference_products(p, x, y)
    off, idx, values = p["offsets"], p["indices"], p["values"]
    t_off, t_rows, t_values = dc.transposed(p)
    for r in (3, 401, 601, 10):  # a run of 256, the longest row, two segments with strays, an ordinary row
        exact = _exact_row(values[off[r]:off[r + 1]], x, idx[off[r]:off[r + 1]])
        L, mag = int(ref["len_ax"][r]), Fraction(float(ref["mag_ax"][r]))
        assert L == off[r + 1] - off[r]
        # (the longdouble itself is read exactly: 64 significant bits split in two float64 halves)
        hi = float(ref["ax"][r])
        lo = float(ref["ax"][r] - np.longdouble(hi))
        assert abs(Fraction(hi) + Fraction(lo) - exact) <= L * Fraction(1, 2 ** 64) * mag * Fraction(1001, 1000), r
    for c in (0, 300, 9000):
        exact = _exact_row(t_values[t_off[c]:t_off[c + 1]], y, t_rows[t_off[c]:t_off[c + 1]])
        L, mag = int(ref["len_aty"][c]), Fraction(float(ref["mag_aty"][c]))
        hi = float(ref["aty"][c])
        lo = float(ref["aty"][c] - np.longdouble(hi))
        assert abs(Fraction(hi) + Fraction(lo) - exact) <= L * Fraction(1, 2 ** 64) * mag * Fraction(1001, 1000), c
    assert (ref["ax"][ref["len_ax"] == 0] == 0).all() and (ref["aty"][ref["len_aty"] == 0] == 0).all()


@pytest.mark.parametrize("case", ["boundary", "stack-33", "abut", "threshold-1"])
def test_one_float64_dot_per_row_stays_inside_the_bound(case, boundary):
    p = boundary[0] if case == "boundary" else dc.stack_lp(33) if case == "stack-33" else dc.abut_lp() if case == "abut" else dc.threshold_lp(1)
    mod = boundary[1] if case == "boundary" else dc.model(p)
    for k, (x, y) in enumerate(dc.vectors(p, 7)):
        ref = dc.reference_products(p, x, y)
        ax, aty = dc.sequential_f64(p, x, y)
        worst = dc.check_products(p, mod, ref, ax, aty, exact_ax=(~mod["rows_touched"], ax), exact_aty=(~mod["cols_touched"], aty))
        at = int(np.argmax(np.abs(ax.astype(np.longdouble) - ref["ax"]) / np.maximum(dc.bound(ref["len_ax"], ref["mag_ax"]), np.longdouble(1e-300))))
        print("RATIOS %s vectors %d %s (A x: the worst row has L = %d)" % (case, k, " ".join("%s=%.3f" % kv for kv in worst.items()), ref["len_ax"][at]))
        if k == 1:
            assert (x == 0).mean() > 0.6 and (y == 0).mean() > 0.6, "exact-zero products"


def _without(p, mod, x, y, what):
    """both products with part of the segments' share left out: what a table that is one entry short makes of them"""
    off, idx, values = np.asarray(p["offsets"], np.int64), np.asarray(p["indices"], np.int64), p["values"].copy()
    for r, c0, length in mod["segs"]:
        k = off[r] + int(np.searchsorted(idx[off[r]:off[r + 1]], c0))
        if what == "last chunk" and length > dc.CHUNK:
            values[k + (length - 1) // dc.CHUNK * dc.CHUNK:k + length] = 0.0
        if what == "last tile" and (c0 + length - 1) // dc.TILE > c0 // dc.TILE:
            values[k + (c0 + length - 1) // dc.TILE * dc.TILE - c0:k + length] = 0.0
        if what == "one segment" and (r, c0) == (801, 4257):
            values[k:k + length] = 0.0
    return dc.sequential_f64(p, x, y, values)


@pytest.mark.parametrize("what", ["last chunk", "last tile", "one segment"])
def test_a_product_that_misses_part_of_a_segment_fails_the_check(what, boundary):
    p, mod = boundary
    for x, y in dc.vectors(p, 7):
        ref = dc.reference_products(p, x, y)
        good_ax, good_aty = dc.sequential_f64(p, x, y)
        ax, aty = _without(p, mod, x, y, what)
        for pair in ((ax, good_aty), (good_ax, aty)):  # either product alone gives it away
            with pytest.raises(AssertionError):
                dc.check_products(p, mod, ref, *pair)


def test_a_product_that_moves_where_no_segment_reaches_fails_the_exact_comparison(boundary):
    p, mod = boundary
    x, y = dc.vectors(p, 7)[0]
    ref = dc.reference_products(p, x, y)
    ax, aty = dc.sequential_f64(p, x, y)
    moved = ax.copy()
    moved[10] = np.nextafter(moved[10], np.inf)  # inside the bound of a row of several products, not the same bits
    assert len(p["indices"][p["offsets"][10]:p["offsets"][11]]) > 2 and not mod["rows_touched"][10]
    dc.check_products(p, mod, ref, moved, aty)
    with pytest.raises(AssertionError):
        dc.check_products(p, mod, ref, moved, aty, exact_ax=(~mod["rows_touched"], ax))
