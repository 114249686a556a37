"""TEST UTILITY: the LPs, the model of the segment rule, the reference products and the bound of tests/test_dense_boundaries_gpu.py
(dense row segments, cuopt_amd/csrc/kernels_dense.hip, spmv_panel.hpp, pdlp_create.hip).  tests/test_dense_cases.py runs all of it
on the host.  numpy only.

THE RULE (segments): a row takes part only when its columns are strictly increasing; inside such a row every MAXIMAL run of columns
that step by +1 is a segment when it holds at least 256 entries (MIN_RUN).  A segment's entries are stored index-free; a row's
segments are cut into chunks of 4096 entries (CHUNK) for the A product, and taken per 256-column tile (TILE) for the A^T product.
The path switches itself on when the segments hold at least 2 % of the nonzeros (entries * 50 >= nnz).  model() restates this from
the description above, in plain Python, and counts what the GPU test relies on.

THE LPs
    boundary_lp   1200 x 9001 (9001 = 35 * 256 + 41: the last tile is partial).  BOUNDARY_ROWS lists the designed rows as (first
                  column, length) runs plus stray columns: runs of exactly 256, 4096 and 4097 entries and one entry short of / beyond
                  them, a run from column 0, a run that ends in column n - 1, a run of 255 (stays sparse), rows with two segments
                  (one column apart) and with a sparse run between two segments, nine segments over one tile, rows whose sparse
                  remainder is empty and rows that keep strays in front of, between and behind their segments.  Every other row is
                  ORDINARY: 0 .. 12 entries in columns 2 .. 8599 (so columns 0, 1 and 8744 .. 9000 are touched by segments alone, and
                  tile 33 by none), every 97th of them empty.
    stack_lp(K)   400 x 2048: rows 10 .. 10 + K - 1 hold the run (512, 256) and nothing else -- K segments over ONE tile (columns
                  512 .. 767) and over the panels those columns fall in; the columns' sparse remainder is the ordinary rows' alone.
    abut_lp       400 x 2048: 32 such rows next to one run (256, 256), and A^T's forced panels cut between columns 511 and 512 (its
                  docstring): the overlap test that lists a panel's segments, at both of its edges.
    threshold_lp  600 x 1500, one run of 256 entries and nnz = 12800 + extra: 256 * 50 = 12800, the switch-on rule's edge.
All are bounded and feasible (0 <= x <= 3, rows <= 50: x = 0 is feasible), so a solve runs on them.

THE BOUND (bound): for a sum of L products in float64, in ANY order and with or without fused multiply-adds, every product passes
through one rounding of its own and at most L - 1 additions (with FMAs: L roundings at most), so |got - exact| <= gamma_L * sum|a_k||v_k|
with gamma_L = L u / (1 - L u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2; argued at
length in tests/attempt_reference.py).  The reference itself is summed in numpy.longdouble (u' = 2^-64 on x86), so its own error
L * 2^-64 * sum|a_k||v_k| is added.  No tolerance is guessed: L is the number of stored entries of the row / column."""
import numpy as np

INF = np.inf
MIN_RUN, CHUNK, TILE, PANEL_SEGS = 256, 4096, 256, 32
U = 2.0 ** -53
M_B, N_B = 1200, 9001
ORDINARY_COLS = (2, 8600)  # ordinary entries of boundary_lp: columns 2 .. 8599
# row -> ([(first column, length)], [stray columns])
BOUNDARY_ROWS = {
    3: ([(0, 256)], []),
    4: ([(255, 255)], []),  # stays sparse
    64: ([(256, 257)], []),
    65: ([(1, 4095)], []),
    200: ([(300, 4096)], []),
    201: ([(511, 4097)], []),
    400: ([(2, 8192)], []),
    401: ([(1, 8193)], []),
    600: ([(8744, 257)], []),  # ends at column n - 1
    601: ([(100, 300), (401, 300)], [5, 50, 8000]),
    800: ([(1000, 256), (1300, 255), (2000, 600)], [1280, 8900]),
    801: ([(4000, 256), (4257, 256)], []),
    900: ([(2500, 256)], [7]),
    901: ([(2600, 256)], []),
    902: ([(2700, 300)], [8599]),
}
# what model(boundary_lp(BOUNDARY_SEED)) must give (tests/test_dense_cases.py)
# (everything but the last figure follows from BOUNDARY_ROWS; how many columns the ordinary rows leave to the segments alone depends on
#  the draw: 3600 .. 3700 over the seeds tried, 3662 at this one)
BOUNDARY_SEED = 16
BOUNDARY_FIGURES = dict(segments=17, rows=14, entries=32223, chunks=21, tiles=36, tiles_touched=35, max_segments_per_tile=9,
                        rows_without_remainder=10, segment_only_columns=3662)


# ---- the LPs -----------------------------------------------------------------------------------------------------------------------------
def _assemble(m, n, rows, rng):
    """rows: per row a sorted array of columns -> the LP dict"""
    lens = np.array([len(c) for c in rows], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = (np.concatenate(rows) if lens.sum() else np.zeros(0)).astype(np.int32)
    values = rng.standard_normal(len(idx))
    values[values == 0.0] = 1.0
    return dict(m=m, n=n, offsets=off, indices=idx, values=values, c=rng.standard_normal(n), lo=np.full(m, -INF), hi=np.full(m, 50.0),
                lb=np.zeros(n), ub=np.full(n, 3.0), maximize=False, objective_offset=0.0)


def _ordinary(rng, m, special, c0, c1, longest=12):
    """m rows of 0 .. `longest` entries in columns c0 .. c1 - 1, every 97th ORDINARY row empty; rows in `special` are left out (None)"""
    rows, count = [], 0
    for r in range(m):
        if r in special:
            rows.append(None)
            continue
        count += 1
        size = 0 if count % 97 == 0 else int(rng.integers(0, longest + 1))
        rows.append(np.sort(rng.choice(np.arange(c0, c1), size=size, replace=False)))
    return rows


def _designed(runs, strays):
    cols = np.concatenate([np.arange(c0, c0 + length) for c0, length in runs] + [np.array(strays, np.int64)])
    assert len(np.unique(cols)) == len(cols)
    return np.sort(cols)


def boundary_lp(seed=BOUNDARY_SEED):
    rng = np.random.default_rng(seed)
    rows = _ordinary(rng, M_B, BOUNDARY_ROWS, *ORDINARY_COLS)
    for r, (runs, strays) in BOUNDARY_ROWS.items():
        rows[r] = _designed(runs, strays)
    return _assemble(M_B, N_B, rows, rng)


def stack_lp(K, seed=1):
    m, n = 400, 2048
    assert 1 <= K <= m - 20
    rng = np.random.default_rng(seed)
    special = set(range(10, 10 + K))
    rows = _ordinary(rng, m, special, 0, n)
    for r in special:
        rows[r] = np.arange(512, 512 + 256)
    return _assemble(m, n, rows, rng)


def threshold_lp(extra, seed=2):
    """one run of 256 entries (row 7, from column 300) and 12544 + extra ordinary entries in the other 599 rows (20 or 21 or 22 each)"""
    m, n, run_row = 600, 1500, 7
    rng = np.random.default_rng(seed)
    want = 50 * MIN_RUN - MIN_RUN + extra
    lens = np.full(m - 1, want // (m - 1), np.int64)
    lens[:want - int(lens.sum())] += 1
    assert lens.sum() == want and lens.max() < MIN_RUN
    rows = [np.sort(rng.choice(n, size=int(l), replace=False)) for l in lens]
    rows.insert(run_row, np.arange(300, 300 + MIN_RUN))
    p = _assemble(m, n, rows, rng)
    assert len(p["indices"]) == 50 * MIN_RUN + extra
    return p


def abut_lp(seed=3):
    """400 x 2048: row 5 holds the run (256, 256), rows 10 .. 41 the run (512, 256), and the forced panels of A^T are cut between
    columns 511 and 512: a panel takes columns while their entries (the sparse remainder's) stay within PANEL_TARGET = 2048, columns
    0 .. 511 hold exactly 4 sparse entries each (rows 50 .. 65: every fourth column), column 512 holds one (row 70).  So one segment ENDS
    where the second panel begins and 32 -- as many as the panel epilogue takes -- BEGIN there: an overlap test that is off by one on
    either side hands a panel 33."""
    m, n = 400, 2048
    rng = np.random.default_rng(seed)
    special = {5: np.arange(256, 512), 70: np.array([512, 1000])}
    special.update({r: np.arange(512, 768) for r in range(10, 42)})
    special.update({50 + j: np.arange(j % 4, 512, 4) for j in range(16)})
    rows = _ordinary(rng, m, special, 513, n)
    for r, cols in special.items():
        rows[r] = cols
    return _assemble(m, n, rows, rng)


PANEL_TARGET = 2048  # panel_plan's smallest target (cuopt_amd/csrc/kernels_panel.hip): what a matrix of a few thousand entries gets


# ---- the rule, restated --------------------------------------------------------------------------------------------------------------------
def segments(p):
    """[(row, first column, length)] in ascending row order, a row's segments in ascending column order"""
    off, idx, out = p["offsets"], p["indices"], []
    for r in range(p["m"]):
        cols = [int(c) for c in idx[off[r]:off[r + 1]]]
        if any(b <= a for a, b in zip(cols, cols[1:])):
            continue  # not strictly increasing: the whole row stays sparse
        start = 0
        for k in range(1, len(cols) + 1):
            if k == len(cols) or cols[k] != cols[k - 1] + 1:
                if k - start >= MIN_RUN:
                    out.append((r, cols[start], k - start))
                start = k
    return out


def model(p):
    """the figures the tests assert, and the masks of the rows / columns a segment touches"""
    m, n, off, idx = p["m"], p["n"], np.asarray(p["offsets"], np.int64), np.asarray(p["indices"], np.int64)
    segs = segments(p)
    rows_touched, cols_touched = np.zeros(m, bool), np.zeros(n, bool)
    in_segment = np.zeros(len(idx), bool)  # per stored entry
    per_tile = np.zeros(-(-n // TILE), np.int64)
    chunks = 0
    for r, c0, length in segs:
        rows_touched[r] = True
        cols_touched[c0:c0 + length] = True
        k = off[r] + int(np.searchsorted(idx[off[r]:off[r + 1]], c0))
        assert (idx[k:k + length] == np.arange(c0, c0 + length)).all()
        in_segment[k:k + length] = True
        per_tile[c0 // TILE:(c0 + length - 1) // TILE + 1] += 1
        chunks += -(-length // CHUNK)
    entries = int(in_segment.sum())
    row_of = np.repeat(np.arange(m), np.diff(off))
    sparse_per_row = np.bincount(row_of[~in_segment], minlength=m)
    sparse_per_col = np.bincount(idx[~in_segment], minlength=n)
    return dict(segs=segs, segments=len(segs), rows=int(rows_touched.sum()), entries=entries, chunks=chunks, tiles=len(per_tile),
                tiles_touched=int((per_tile > 0).sum()), max_segments_per_tile=int(per_tile.max()) if len(per_tile) else 0,
                rows_without_remainder=int((rows_touched & (sparse_per_row == 0)).sum()),
                segment_only_columns=int((cols_touched & (sparse_per_col == 0)).sum()),
                on_by_default=entries > 0 and entries * 50 >= len(idx), rows_touched=rows_touched, cols_touched=cols_touched,
                in_segment=in_segment, sparse_per_col=sparse_per_col)


# ---- the reference and the bound -----------------------------------------------------------------------------------------------------------
def transposed(p, values=None):
    """(offsets, rows, values) of A^T, a column's entries in ascending row order"""
    off, idx = np.asarray(p["offsets"], np.int64), np.asarray(p["indices"], np.int64)
    values = np.asarray(p["values"] if values is None else values, np.float64)
    row_of = np.repeat(np.arange(p["m"]), np.diff(off))
    order = np.argsort(idx, kind="stable")
    t_off = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=p["n"]))])
    return t_off, row_of[order], values[order]


def _row_sums(off, idx, values, v, dtype):
    lens = np.diff(off)
    prod = values.astype(dtype) * v[idx].astype(dtype)
    out, mag = np.zeros(len(lens), dtype), np.zeros(len(lens), dtype)
    some = lens > 0
    if some.any():
        out[some] = np.add.reduceat(prod, off[:-1][some])
        mag[some] = np.add.reduceat(np.abs(prod), off[:-1][some])
    return out, mag, lens


def reference_products(p, x, y, values=None, at_values=None):
    """A x and A^T y in numpy.longdouble from the full CSR, and per row / column sum |a_k| |v_k| and the number of stored entries L
    -> dict(ax, mag_ax, len_ax, aty, mag_aty, len_aty).  `values`: other values on p's pattern; `at_values`: the values A^T holds, in
    p's order, where they are not `values` bit for bit (the scaled matrices: each side is rounded in an order of its own)"""
    off, idx = np.asarray(p["offsets"], np.int64), np.asarray(p["indices"], np.int64)
    values = np.asarray(p["values"] if values is None else values, np.float64)
    ax, mag_ax, len_ax = _row_sums(off, idx, values, np.asarray(x, np.float64), np.longdouble)
    t_off, t_rows, t_values = transposed(p, values if at_values is None else at_values)
    aty, mag_aty, len_aty = _row_sums(t_off, t_rows, t_values, np.asarray(y, np.float64), np.longdouble)
    return dict(ax=ax, mag_ax=mag_ax, len_ax=len_ax, aty=aty, mag_aty=mag_aty, len_aty=len_aty)


def bound(L, mag):
    """gamma_L * sum|a_k||v_k| for the float64 sum under test, plus the longdouble reference's own L * 2^-64 * sum|a_k||v_k|"""
    L = np.asarray(L, np.longdouble)
    return (L * U / (1.0 - L * U) + L * np.longdouble(2.0) ** -64) * np.asarray(mag, np.longdouble)


def worst_ratio(got, ref, L, mag, where=None):
    """max over the elements (of `where`) of |got - ref| / bound; an element with a zero bound counts 0 when it is exact, inf when not"""
    err = np.abs(np.asarray(got, np.float64).astype(np.longdouble) - ref)
    b = bound(L, mag)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf)).astype(np.float64)
    ratio[~np.isfinite(np.asarray(got, np.float64))] = np.inf
    if where is not None:
        ratio = ratio[where]
    return float(ratio.max()) if len(ratio) else 0.0


def vectors(p, seed):
    """the two vector pairs of the GPU test: dense Gaussians, and Gaussians with 70 % exact zeros -> [(x, y), (x, y)]"""
    rng = np.random.default_rng(seed)
    n, m = p["n"], p["m"]
    dense = rng.standard_normal(n), rng.standard_normal(m)
    sparse = rng.standard_normal(n) * (rng.random(n) >= 0.7), rng.standard_normal(m) * (rng.random(m) >= 0.7)
    return [dense, sparse]


def sequential_f64(p, x, y, values=None):
    """both products by one float64 numpy.dot per row / column: the stand-in tests/test_dense_cases.py holds against the bound"""
    off, idx = np.asarray(p["offsets"], np.int64), np.asarray(p["indices"], np.int64)
    values = np.asarray(p["values"] if values is None else values, np.float64)
    t_off, t_rows, t_values = transposed(p, values)
    ax = np.array([np.dot(values[a:b], x[idx[a:b]]) for a, b in zip(off[:-1], off[1:])])
    aty = np.array([np.dot(t_values[a:b], y[t_rows[a:b]]) for a, b in zip(t_off[:-1], t_off[1:])])
    return ax, aty


def check_products(p, mod, ref, ax, aty, exact_ax=None, exact_aty=None):
    """What the GPU test asserts of one pair of products -> dict of the worst ratios.  ref: reference_products' dict; exact_ax /
    exact_aty: (mask, values) the rows / columns under the mask must equal bit for bit."""
    rows, cols = mod["rows_touched"], mod["cols_touched"]
    out = dict(ax_touched=worst_ratio(ax, ref["ax"], ref["len_ax"], ref["mag_ax"], rows),
               ax_rest=worst_ratio(ax, ref["ax"], ref["len_ax"], ref["mag_ax"], ~rows),
               aty_touched=worst_ratio(aty, ref["aty"], ref["len_aty"], ref["mag_aty"], cols),
               aty_rest=worst_ratio(aty, ref["aty"], ref["len_aty"], ref["mag_aty"], ~cols))
    assert np.isfinite(ax).all() and np.isfinite(aty).all()
    assert max(out.values()) <= 1.0, out
    assert (ax[ref["len_ax"] == 0] == 0.0).all(), "an empty row's A x is not 0"
    assert (aty[ref["len_aty"] == 0] == 0.0).all(), "an empty column's A^T y is not 0"
    for got, exact, what in ((ax, exact_ax, "A x"), (aty, exact_aty, "A^T y")):
        if exact is not None:
            mask, want = exact
            bad = np.nonzero(mask & (got != want))[0]  # (numpy.testing.assert_array_equal's equality, as the existing dense test's)
            assert len(bad) == 0, (what, "not bit-identical where no segment reaches", bad[:8], got[bad[:8]], want[bad[:8]])
    return out
