"""TEST UTILITY: the LPs and points of the restart-input tests (tests/test_restart_reference.py on the CPU, tests/test_restart_inputs_gpu.py
on the GPU).  numpy only.

An LP of kinds_lp has rows <=, >=, equality, free and ranged and columns free, upper bound only, lb = 0 only, fixed at 1.5 and boxed [0, 5]
in equal shares, a tenth of its rows empty and columns without an entry among which c = 0 on every other one (g = c - A^T y == 0 there).
A point is given in the space of tr_element's centers: x inside its bounds, two fifths of the columns with a finite bound sitting on
it; y sign-feasible as the dual projection leaves it (y <= 0 where lo is infinite, y >= 0 where hi is, 0 on free rows) and zero on a
quarter of the rows and on the first two rows of every kind.  Three seeds give the three different vectors of the three slots."""
import numpy as np

INF = np.inf
WRAP_M, WRAP_N = 262144 + 300, 262144 + 513  # every grid-stride loop (1024 workgroups of 256) takes a second trip that ends mid-workgroup
SLOTS = ("CURRENT", "AVERAGE", "LAST_RESTART")
# what a case with every kind of row and column must reach (restart_reference.elements / infeasibility count them)
RICH_TR = ("col_on_lb_g_pos", "col_on_ub_g_neg", "g_zero", "col_free", "col_fixed", "y_neg", "y_pos", "y0_free", "y0_lo_only", "y0_hi_only",
           "y0_both", "y0_both_below", "y0_both_above", "rows_equality", "blocked", "moving", "moving_forever")
RICH_INFEAS = ("g_zero", "rc_taken", "rc_dropped", "rows_lo_finite_violated", "rows_hi_finite_violated", "rows_free")
RAGGED_TR = tuple(k for k in RICH_TR if k not in ("g_zero", "col_fixed", "rows_equality"))  # (test_kernels_gpu.ragged_problem has none of these)
RAGGED_INFEAS = tuple(k for k in RICH_INFEAS if k != "g_zero")


def _bounds(p, rng):
    m, n = p["m"], p["n"]
    row_kind, col_kind = np.arange(m) % 5, np.arange(n) % 5
    if m >= 5:
        row_kind = rng.permutation(row_kind)
    if n >= 5:
        col_kind = rng.permutation(col_kind)
    b, w = rng.standard_normal(m), np.abs(rng.standard_normal(m)) + 0.5
    p["lo"] = np.choose(row_kind, [np.full(m, -INF), b - 1.0, b, np.full(m, -INF), b - 1.0])  # <= | >= | equality | free | ranged
    p["hi"] = np.choose(row_kind, [b + 3.0, np.full(m, INF), b, np.full(m, INF), b - 1.0 + w])
    p["lb"] = np.choose(col_kind, [-INF, -INF, 0.0, 1.5, 0.0]).astype(np.float64)           # free | upper | lb = 0 | fixed | boxed
    p["ub"] = np.choose(col_kind, [INF, 5.0, INF, 1.5, 5.0]).astype(np.float64)
    p["c"] = rng.standard_normal(n)
    empty = np.nonzero(np.bincount(p["indices"], minlength=n) == 0)[0]
    p["c"][empty[::2]] = 0.0
    p["row_kind"], p["col_kind"] = row_kind, col_kind
    return p


def kinds_lp(m, n, per_row, seed):
    """m x n, `per_row` entries in nine rows out of ten, drawn from the first nine tenths of the columns (the rest hold no entry)"""
    rng = np.random.default_rng(seed)
    lens = np.full(m, per_row)
    if m >= 10:
        lens[rng.choice(m, size=m // 10, replace=False)] = 0
    used = n if n < 10 else n - n // 10
    lens = np.minimum(lens, used)
    if per_row == 2 and used > 4:  # (the wrap LP, built directly: two distinct columns per row)
        a = rng.integers(0, used, size=m)
        b = (a + 1 + rng.integers(0, used - 1, size=m)) % used
        pair = np.sort(np.stack([a, b], axis=1), axis=1)
        idx = pair[lens > 0].reshape(-1)
    else:
        idx = np.concatenate([np.sort(rng.choice(used, size=l, replace=False)) for l in lens] + [np.zeros(0, np.int64)])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return _bounds(dict(m=m, n=n, offsets=off, indices=idx.astype(np.int32), values=rng.standard_normal(int(off[-1]))), rng)


def point(p, seed):
    """(x, y) in the space of the centers"""
    rng = np.random.default_rng(seed)
    m, n = p["m"], p["n"]
    lo, hi, lb, ub = (np.asarray(p[k], dtype=np.float64) for k in ("lo", "hi", "lb", "ub"))
    x = np.abs(rng.standard_normal(n)) * (rng.random(n) < 0.7)
    x = np.where(np.isinf(lb), rng.standard_normal(n), x)
    x = np.minimum(np.maximum(x, lb), ub)
    sit = rng.random(n)
    x = np.where(np.isfinite(lb) & (sit < 0.4), lb, x)
    x = np.where(np.isfinite(ub) & (sit > 0.6), ub, x)
    y = rng.standard_normal(m)
    y = np.where(np.isinf(lo), -np.abs(y), y)
    y = np.where(np.isinf(hi), np.abs(y), y)
    y = np.where(np.isinf(lo) & np.isinf(hi), 0.0, y)
    zero = rng.random(m) < 0.25
    kind = np.asarray(p.get("row_kind", np.zeros(m, np.int64)))
    for k in np.unique(kind):
        zero[np.nonzero(kind == k)[0][:2]] = True
    if m < 5:
        zero[:] = False
    return x, np.where(zero, 0.0, y)


def to_scaled(v, d):
    """vhat with fl(vhat d) == v wherever one of v / d and its two neighbours gives that (a point sitting on a bound keeps sitting on it)"""
    v, d = np.asarray(v, dtype=np.float64), np.asarray(d, dtype=np.float64)
    out = v / d
    for toward in (INF, -INF):
        bad = out * d != v
        cand = np.nextafter(out, toward)
        out = np.where(bad & (cand * d == v), cand, out)
    return out


def integer_lp(m=40, n=30, seed=77):
    """||objective|| == 0 exactly: small integers everywhere (every product and sum is exact in any order, the LP is evaluated unscaled),
    c = A^T y, a row with y > 0 has lo = (A x)_i, with y < 0 hi = (A x)_i, with y = 0 is ranged around (A x)_i -> (p, x, y)"""
    rng = np.random.default_rng(seed)
    dense = rng.integers(-2, 3, size=(m, n)) * (rng.random((m, n)) < 0.2)
    rows, cols = np.nonzero(dense)
    off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    x = rng.integers(0, 4, size=n).astype(np.float64)
    y = rng.integers(-3, 4, size=m).astype(np.float64)
    ax, aty = dense @ x, dense.T @ y
    p = dict(m=m, n=n, offsets=off, indices=cols.astype(np.int32), values=dense[rows, cols].astype(np.float64), c=aty.astype(np.float64),
             lo=np.where(y > 0, ax, np.where(y < 0, -INF, ax - 1.0)), hi=np.where(y < 0, ax, np.where(y > 0, INF, ax + 1.0)),
             lb=np.zeros(n), ub=np.full(n, 5.0))
    return p, x, y


def all_finite_lp(m=120, n=90, seed=78):
    """every moving element has a finite threshold: boxed columns, rows <= that the point satisfies strictly (a dual element moves
    towards its bound 0 or is blocked on it) -> (p, x, y)"""
    p = kinds_lp(m, n, 4, seed)
    rng = np.random.default_rng(seed + 1)
    p["lb"], p["ub"] = np.zeros(n), np.full(n, 5.0)
    x = rng.random(n) * 5.0 * (rng.random(n) < 0.8)
    dense = np.zeros((m, n))
    dense[np.repeat(np.arange(m), np.diff(p["offsets"])), p["indices"]] = p["values"]
    p["lo"], p["hi"] = np.full(m, -INF), dense @ x + 1.0
    y = -np.abs(rng.standard_normal(m)) * (rng.random(m) < 0.7)
    return p, x, y


_cache = {}


def _freeze(*things):
    for t in things:
        for a in (t.values() if isinstance(t, dict) else [t]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)


def shape_lp(name):
    """the LPs of the shapes: built once, read-only -> p"""
    if name not in _cache:
        if name == "1x1":
            p = dict(m=1, n=1, offsets=np.array([0, 1], np.int32), indices=np.array([0], np.int32), values=np.array([0.75]),
                     c=np.array([-0.6]), lo=np.array([-0.5]), hi=np.array([2.0]), lb=np.array([0.0]), ub=np.array([5.0]))
        elif name == "ragged":
            from test_kernels_gpu import ragged_problem
            p = ragged_problem()
        else:
            m, n, per_row, seed = {"37x53": (37, 53, 5, 61), "300x257": (300, 257, 6, 62), "wrap": (WRAP_M, WRAP_N, 2, 63)}[name]
            p = kinds_lp(m, n, per_row, seed)
        _freeze(p)
        _cache[name] = p
    return _cache[name]


def shape_points(name):
    """three different points for the three slots -> {slot: (x, y)}"""
    key = ("points", name)
    if key not in _cache:
        p = shape_lp(name)
        pts = {slot: point(p, 100 + 7 * i) for i, slot in enumerate(SLOTS)}
        if name == "1x1":  # (one column, one row: a point inside, one on the upper bound, one on the lower)
            pts = dict(CURRENT=(np.array([0.3]), np.array([0.4])), AVERAGE=(np.array([5.0]), np.array([-0.7])), LAST_RESTART=(np.array([0.0]), np.array([0.0])))
        for v in pts.values():
            _freeze(*v)
        _cache[key] = pts
    return _cache[key]


SHAPES = ("1x1", "37x53", "300x257", "ragged", "wrap")
SMALL_SHAPES = ("1x1", "37x53", "300x257")
# (wp, wd, pds, dds, primal_weight): tau = 0.5, sigma = 1 / 0.7 of a solve; a lopsided pair
WEIGHTS = ((2.0, 0.7, 0.5, 0.5, 1.5), (0.3, 5.0, 0.2, 0.8, 0.4))
RADII = (-1.0, 1e-30, 1e-3, 0.5, 10.0, 1e4, 1e7)  # own distance; inside the first breakpoint, across many, beyond all finite ones
WRAP_RADII = (-1.0, 1e-30, 0.5, 1e7)


def required(name):
    if name == "ragged":
        return RAGGED_TR, RAGGED_INFEAS
    if name == "1x1":
        return (), ()
    return RICH_TR, RICH_INFEAS
