"""TEST UTILITY: the LPs of the frame tests (tests/test_frame_reference.py on the CPU, tests/test_frame_gpu.py on the GPU), each the
smallest that reaches its path.  numpy only.

    edge        eval_lps.edge_lp as tests/test_eval_layouts_gpu.variant_lp serves it (6000 x 6000; rows of 129, 300, 2049 and 2400 entries,
                columns of 129, 400 and 4500 -- 2400 under the gather-free ids --, empty rows and columns, five row and five column kinds)
                and its twin with dense segments
    1x1         restart_cases.shape_lp("1x1")
    hand        3 x 2, written out: tests/test_frame_reference.py states its every scaling pass and norm in exact rationals
    zero-c      37 x 53 with c = 0        -> sum c^2 == 0.0 exactly
    free-rows   37 x 53 with every row free -> sum combine_bounds^2 == 0.0 exactly
    wrap        3000 x 525 000, one nonzero in nine columns out of ten: nnz and n are beyond 262 144 = kGenericBlocks * kBlock (the
                reductions' grid wraps) and beyond 524 288 = 2048 * kBlock (the element-wise kernels' grid wraps), the second trip ends
                mid-workgroup; rows on both sides of kLongRow; bounds of every kind
    resident    resident_lps.lp("t1") (700 x 1000), opened so that it takes the one-workgroup path

start(p, x0) moves a third of the columns above every finite upper bound and a third below every finite lower bound."""
import numpy as np

import resident_lps
import restart_cases as rc

INF = np.inf
K_LONG_ROW, K_NNZ_BLOCK = 128, 2044                      # kLongRow, kNnzBlock (cuopt_amd/csrc/pdlp_kernels.hpp)
REDUCE_WRAP, ELEMENTWISE_WRAP = 1024 * 256, 2048 * 256   # kGenericBlocks * kBlock; grid_for's cap * kBlock (pdlp_ctx.hpp)
WRAP_M, WRAP_N = 3000, 525000
EDGE_IDS = ("stream", "dense-stream", "panel-rows-4KiB", "jag-8", "pb")  # ids of test_eval_layouts_gpu.VARIANTS
PRESETS = {"ruiz10-pc": 10, "ruiz5-pc": 5}                # Ruiz iterations; Pock-Chambolle with alpha = 1 behind them

_cache = {}


def _frozen(key, make):
    if key not in _cache:
        out = make()
        for t in out if isinstance(out, tuple) else (out,):
            for a in (t.values() if isinstance(t, dict) else [t]):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def edge(name):
    """(p, x0, y0) of the edge LP under id `name`: the very arrays the evaluation tests use"""
    from test_eval_layouts_gpu import variant_lp
    return variant_lp(name)[:3]


def hand():
    """3 x 2.  A = [[4, 0], [0, 16], [2, 16]]: one Ruiz pass gives D_r = (1/2, 1/4, 1/4), D_c = (1/2, 1/4) exactly, and
    D_r A D_c = [[1, 0], [0, 1], [1/4, 1]] has every row and column maximum 1, so every further Ruiz pass changes nothing"""
    def make():
        p = dict(m=3, n=2, offsets=np.array([0, 1, 2, 4], np.int32), indices=np.array([0, 1, 0, 1], np.int32), values=np.array([4.0, 16.0, 2.0, 16.0]),
                 c=np.array([3.0, -8.0]), lo=np.array([-INF, 2.0, -4.0]), hi=np.array([6.0, INF, 3.0]), lb=np.array([0.0, -INF]), ub=np.array([5.0, INF]))
        return p, np.array([7.0, -2.0]), np.array([0.5, -1.0, 2.0])
    return _frozen("hand", make)


def one_by_one():
    return _frozen("1x1", lambda: (dict(rc.shape_lp("1x1")), np.array([7.0]), np.array([0.4])))


def _small(seed, change):
    p = dict(rc.kinds_lp(37, 53, 5, seed))
    change(p)
    x, y = rc.point(p, seed + 1)
    return p, x.copy(), y.copy()


def zero_c():
    return _frozen("zero-c", lambda: _small(91, lambda p: p.update(c=np.zeros(53))))


def free_rows():
    return _frozen("free-rows", lambda: _small(92, lambda p: p.update(lo=np.full(37, -INF), hi=np.full(37, INF))))


def wrap():
    def make():
        rng = np.random.default_rng(93)
        m, n = WRAP_M, WRAP_N
        cols = np.sort(rng.choice(n, size=n - n // 10, replace=False))
        weights = rng.random(m) + 0.2
        weights[rng.choice(m, size=10, replace=False)] = 0.0   # ten empty rows
        rows = rng.choice(m, size=len(cols), p=weights / weights.sum())
        order = np.lexsort((cols, rows))
        off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
        p = rc._bounds(dict(m=m, n=n, offsets=off, indices=cols[order].astype(np.int32), values=rng.standard_normal(len(cols))), rng)
        x = np.abs(rng.standard_normal(n)) * (rng.random(n) < 0.7)
        x[p["col_kind"] == 3] = 1.5
        return p, x, rng.standard_normal(m)
    return _frozen("wrap", make)


def resident():
    return tuple(resident_lps.lp("t1"))


def start(p, x0):
    """x0 with every third column at 7.5 (above every finite upper bound, 5 and 1.5) and every third at -3.25 (below every finite lower
    bound, 0 and 1.5): columns of every kind on both sides, fixed columns off their value"""
    x = np.array(x0, dtype=np.float64)
    x[0::3], x[1::3] = 7.5, -3.25
    return x


CPU_CASES = {"edge-4500": lambda: edge("stream"), "edge-4500-dense": lambda: edge("dense-stream"), "edge-2400": lambda: edge("pb"), "1x1": one_by_one,
             "hand": hand, "zero-c": zero_c, "free-rows": free_rows, "resident": resident}
