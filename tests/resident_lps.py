"""TEST UTILITY: the LPs of the resident small-LP tests (tests/test_resident_attempts_gpu.py on the GPU, tests/test_attempt_reference.py
on the float64 stand-in), in the style of tests/eval_lps.edge_lp.  numpy only.

Every LP: rows <=, >=, equality, free and ranged, columns free, upper bound only, lb = 0 only, fixed at 1.5 and boxed [0, 5] in equal
shares (to within one where the count is no multiple of five); x0 = |N(0,1)| Bernoulli(0.7), exactly 1.5 on the fixed columns;
y0 ~ N(0,1).

The scenario LPs, one per tier of the one-workgroup loop (T lanes, Q rows / columns and U nonzeros per lane):
    t0   300 x  500, 1 600 entries                             tier 0 (256, 2, 8)
    t1   700 x 1000, 6 000 (over 4096: not tier 2)              tier 1 (512, 2, 16)
    t2  1800 x 2000, 3 600                                      tier 2 (512, 4, 8)
each with rows of 0, 1, 7, 8, 9, 16 and 17 entries (lds_row_sum takes eight at a time), one row of 129 and one of 300, one column of 129,
at least 10 empty rows and 10 columns without an entry, c = 0 on every other one of those.

The edge LPs:
    t0-full    512 x  512, 2048 entries exactly   every lane, slot and LDS word of tier 0
    t1-full   1024 x 1024, 8192 exactly           every slot of tier 1; k_major_small at its 65 536 bytes of LDS
    t2-full   2048 x 2048, 4096 exactly           every slot of tier 2
    past-n     300 x  513, 2000                   tier 1 by one column
    past-nnz   400 x  500, 2049                   tier 1 by one nonzero
    rows-only 1025 x   40                         tier 2 by its rows: most lanes own rows and no column, n is less than a wave
    cols-only   40 x 1025                         the mirror image
    spanning    64 x   64                         row 20 holds all 64 columns, column 40 all 64 rows
    minimal-1x2, minimal-2x1                      one nonzero slot in use, almost every lane idle
The `full` ones keep 10 columns without an entry (c = 0 on all of them) and 10 empty rows inside their exact counts."""
import numpy as np

INF = np.inf
ROW_LENGTHS = (0, 1, 7, 8, 9, 16, 17)  # every scenario LP has rows of these lengths ...
LONG_ROWS = (129, 300)                 # ... and of these
LONG_COL = 129
EMPTY = 10                             # empty rows and columns without an entry, at least
# id -> (m, n, entries (None: what the lengths drawn come to), tier, mean row length, seed)
SCENARIO = {"t0": (300, 500, 1600, 0, 4, 21), "t1": (700, 1000, 6000, 1, 8, 22), "t2": (1800, 2000, 3600, 2, 2, 23)}
FULL = {"t0-full": (512, 512, 2048, 0, 4, 31), "t1-full": (1024, 1024, 8192, 1, 8, 32), "t2-full": (2048, 2048, 4096, 2, 2, 33)}
EDGE = {"past-n": (300, 513, 2000, 1, 4, 41), "past-nnz": (400, 500, 2049, 1, 5, 42), "rows-only": (1025, 40, None, 2, 2, 43),
        "cols-only": (40, 1025, None, 2, 50, 44), "spanning": (64, 64, None, 0, 4, 45), "minimal-1x2": (1, 2, None, 0, 2, 46),
        "minimal-2x1": (2, 1, None, 0, 1, 47)}
ALL = {**SCENARIO, **FULL, **EDGE}
SPANNING_ROW, SPANNING_COL = 20, 40


def _kinds(count, rng):
    return rng.permutation(np.arange(count) % 5)


def _finish(p, rng, zero_cost):
    """bounds, costs and the start: eval_lps.edge_lp's"""
    m, n = p["m"], p["n"]
    row_kind, col_kind = _kinds(m, rng), _kinds(n, rng)
    b, w = rng.standard_normal(m), np.abs(rng.standard_normal(m)) + 0.5
    p["lo"] = np.choose(row_kind, [np.full(m, -INF), b - 1.0, b, np.full(m, -INF), b - 1.0])       # <= | >= | equality | free | ranged
    p["hi"] = np.choose(row_kind, [b + 3.0, np.full(m, INF), b, np.full(m, INF), b - 1.0 + w])
    p["lb"] = np.choose(col_kind, [-INF, -INF, 0.0, 1.5, 0.0]).astype(np.float64)                # free | upper | lb = 0 | fixed | boxed
    p["ub"] = np.choose(col_kind, [INF, 5.0, INF, 1.5, 5.0]).astype(np.float64)
    p["c"] = rng.standard_normal(n)
    p["c"][list(zero_cost)] = 0.0
    x = np.abs(rng.standard_normal(n)) * (rng.random(n) < 0.7)
    x[col_kind == 3] = 1.5
    return p, x, rng.standard_normal(m)


def _csr(m, n, lens, allowed, rng, column=None, column_rows=()):
    """rows of `lens` entries in columns drawn from `allowed`, ascending; the rows of `column_rows` hold `column` as one of theirs"""
    holds = np.zeros(m, bool)
    holds[list(column_rows)] = True
    idx = []
    for r in range(m):
        cols = rng.choice(allowed, size=int(lens[r]) - int(holds[r]), replace=False)
        idx.append(np.sort(np.concatenate([cols, [column]]) if holds[r] else cols))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = np.concatenate(idx).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
    return dict(m=m, n=n, offsets=off, indices=idx, values=rng.standard_normal(int(off[-1])))


def rich_lp(name):
    """the scenario and the `full` LPs, past-n and past-nnz -> (p, x0, y0)"""
    m, n, entries, tier, mean, seed = ALL[name]
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 2 * mean, size=m)
    special = list(ROW_LENGTHS) + list(LONG_ROWS) + [0] * (EMPTY - 1)
    rows = rng.choice(m, size=len(special), replace=False)
    lens[rows] = special
    free = np.setdiff1d(np.arange(m), rows)  # rows whose length nothing above promises: they take the long column and the exact count
    col_rows = rng.choice(free, size=LONG_COL, replace=False)
    lens[col_rows] = np.maximum(lens[col_rows], 1)
    if entries is not None:  # the exact count: one entry at a time on and off rows nothing is promised of
        while lens.sum() != entries:
            r = rng.choice(free)
            if lens.sum() < entries and lens[r] < 4 * mean:
                lens[r] += 1
            elif lens.sum() > entries and lens[r] > 1:
                lens[r] -= 1
    empty_cols = rng.choice(n, size=EMPTY + 1, replace=False)
    long_col, empty_cols = int(empty_cols[0]), np.sort(empty_cols[1:])
    allowed = np.setdiff1d(np.arange(n), np.concatenate([[long_col], empty_cols]))
    p = _csr(m, n, lens, allowed, rng, long_col, col_rows)
    p["empty_cols"], p["long_col"] = empty_cols, long_col
    return _finish(p, rng, empty_cols if name in FULL else empty_cols[::2])


def thin_lp(name):
    """rows-only, cols-only, spanning and the two minimal LPs -> (p, x0, y0): every column (row) of the short side is in use"""
    m, n, entries, tier, mean, seed = ALL[name]
    rng = np.random.default_rng(seed)
    lens = np.minimum(rng.integers(1, 2 * mean + 1, size=m), n)
    if name == "rows-only":
        lens[rng.choice(m, size=EMPTY, replace=False)] = 0
    if name == "spanning":
        lens[SPANNING_ROW] = n
    if name.startswith("minimal"):
        lens[:] = n
    column = SPANNING_COL if name == "spanning" else None
    allowed = np.arange(n) if column is None else np.setdiff1d(np.arange(n), [column])
    if name == "spanning":
        p = _csr(m, n, lens, allowed, rng, column, np.arange(m))
    else:
        p = _csr(m, n, lens, allowed, rng)
    p["empty_cols"] = np.nonzero(np.bincount(p["indices"], minlength=n) == 0)[0]
    return _finish(p, rng, p["empty_cols"][::2])


_cache = {}


def lp(name):
    """(p, x0, y0) of id `name`, built once and read-only"""
    if name not in _cache:
        p, x, y = (rich_lp if name in SCENARIO or name in FULL or name in ("past-n", "past-nnz") else thin_lp)(name)
        for a in list(p.values()) + [x, y]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (p, x, y)
    return _cache[name]


def tier_of(name):
    return ALL[name][3]
