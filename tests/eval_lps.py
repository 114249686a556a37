"""TEST UTILITY: the LPs of the evaluation tests (tests/test_eval_reference.py on the CPU, tests/test_eval_layouts_gpu.py on the GPU) and
the long-column construction they share with tests/test_period_path_gpu.py.  numpy only."""
import numpy as np

INF = np.inf

M = N = 6000
LONG_ROWS = {5: 300, 700: 129, 1500: 2400, 2999: 2049}  # cooperative path, a row of its own workgroup, a row over many 4 KiB slabs
LONG_COLS = (17, 250, 5900)                             # 400, `long_col` and 129 nonzeros
EMPTY_COLS = tuple(range(5600, 5800, 10))               # 20 columns without an entry: c = 0 on every other one
DENSE_ROWS = {10: (1000, 300), 3500: (500, 5000)}       # row: (first column, length) of a run of consecutive columns
WIDE_N = 60000                                          # columns of the LP for the gather-free layout's wide bins (test_eval_layouts_gpu.py)
SEEDS = (5, 6)                                          # the seeds the GPU test builds its LPs with


def with_long_column(p, col, count, seed=3, avoid=None):
    """p with `count` nonzeros in column `col` (the rows of A^T are the columns of A: the twin kernel walks those); no entry goes
    into the rows of `avoid`"""
    rng = np.random.default_rng(seed)
    m, off, idx, val = p["m"], p["offsets"], p["indices"], p["values"]
    rows = np.repeat(np.arange(m), np.diff(off))
    keep = idx != col
    pool = m if avoid is None else np.setdiff1d(np.arange(m), avoid)
    add_rows = np.sort(rng.choice(pool, size=count, replace=False))
    r = np.concatenate([rows[keep], add_rows])
    c = np.concatenate([idx[keep], np.full(count, col)])
    v = np.concatenate([val[keep], 0.05 * rng.standard_normal(count)])
    order = np.lexsort((c, r))
    q = dict(p)
    q["offsets"] = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))]).astype(np.int32)
    q["indices"], q["values"] = c[order].astype(np.int32), v[order]
    return q


def edge_lp(long_col=4500, dense=False, seed=5, n=N):
    """6000 x 6000 (6000 x n), the smallest LP that reaches every path of the evaluation kernels.

    rows:    the lengths of test_kernels_gpu.ragged_problem (0 .. 23, every 97th row empty, rows of 129, 300, 2049 and 2400 nonzeros);
             dense: two rows are runs of 300 and of 5000 consecutive columns (over the 256 minimum; over kDenseChunk = 4096)
    columns: 129, 400 and `long_col` nonzeros in three of them (with_long_column), 20 empty ones, c = 0 on every other empty one
    kinds:   rows <=, >=, equality, free, ranged and columns free, upper bound only, lb = 0 only, fixed at 1.5, boxed [0, 5] in
             equal shares
    Returns (p, x, y): x = |N(0,1)| Bernoulli(0.7), exactly 1.5 on the fixed columns; y ~ N(0,1) with no sign repair."""
    rng = np.random.default_rng(seed)
    m = M
    lens = rng.integers(0, 24, size=m)
    lens[::97] = 0
    for r, l in LONG_ROWS.items():
        lens[r] = l
    empty_rows = np.nonzero(lens == 0)[0]
    allowed = np.setdiff1d(np.arange(n), np.concatenate([LONG_COLS, EMPTY_COLS]))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = np.concatenate([np.sort(rng.choice(allowed, size=l, replace=False)) for l in lens]).astype(np.int32)
    p = dict(m=m, n=n, offsets=off, indices=idx, values=rng.standard_normal(off[-1]))
    for col, count, s in zip(LONG_COLS, (400, long_col, 129), (3, 4, 7)):
        p = with_long_column(p, col, count, seed=seed + s, avoid=np.concatenate([empty_rows, list(DENSE_ROWS)]))
    if dense:
        rows = np.repeat(np.arange(m), np.diff(p["offsets"]))
        keep = ~np.isin(rows, list(DENSE_ROWS))
        r, c, v = [rows[keep]], [p["indices"][keep]], [p["values"][keep]]
        for row, (c0, length) in DENSE_ROWS.items():
            r.append(np.full(length, row)), c.append(np.arange(c0, c0 + length)), v.append(0.1 * rng.standard_normal(length))
        r, c, v = np.concatenate(r), np.concatenate(c), np.concatenate(v)
        order = np.lexsort((c, r))
        p["offsets"] = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))]).astype(np.int32)
        p["indices"], p["values"] = c[order].astype(np.int32), v[order]
    row_kind, col_kind = rng.permutation(np.arange(m) % 5), rng.permutation(np.arange(n) % 5)
    b, w = rng.standard_normal(m), np.abs(rng.standard_normal(m)) + 0.5
    # <= | >= | equality | free | ranged
    p["lo"] = np.choose(row_kind, [np.full(m, -INF), b - 1.0, b, np.full(m, -INF), b - 1.0])
    p["hi"] = np.choose(row_kind, [b + 3.0, np.full(m, INF), b, np.full(m, INF), b - 1.0 + w])
    # free | upper bound only | lb = 0 only | fixed | boxed
    p["lb"] = np.choose(col_kind, [-INF, -INF, 0.0, 1.5, 0.0]).astype(np.float64)
    p["ub"] = np.choose(col_kind, [INF, 5.0, INF, 1.5, 5.0]).astype(np.float64)
    p["c"] = rng.standard_normal(n)
    p["c"][list(EMPTY_COLS[::2])] = 0.0
    x = np.abs(rng.standard_normal(n)) * (rng.random(n) < 0.7)
    x[col_kind == 3] = 1.5
    y = rng.standard_normal(m)
    return p, x, y
