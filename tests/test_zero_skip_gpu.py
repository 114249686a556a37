"""GPU: skipping the gathers of zero entries in the A product of a PDHG attempt (CUOPT_AMD_TUNE=zero_skip) changes no bit.

k_primal writes one bit per column of xbar (set where the entry is not 0.0); k_panel_a_dual<false> keeps the current slab's bits in LDS
and fetches xbar[j] only where bit j is set.  Every test runs the same attempts on the same inputs with zero_skip=2 (on) and
zero_skip=0 (the code as it was: no bitmap exists) and compares x', xbar, y', A^T y', the running sums, the reduction partials of
both products and the control block as raw 64-bit patterns, attempt by attempt; the downloaded bitmap is compared with numpy's
bits of xbar != 0.  The geometries are the ones at which the bitmap's indexing can go wrong: n below, at and off a multiple of 64,
slabs that start in the middle of a word, slabs narrower than a word, tiles of several chunks, an empty tile, rows beyond 128
entries (summed by their wave) and a row with a workgroup of its own (which gathers without the bitmap).

With zero_skip=1 (the default) the control block's flag decides, attempt by attempt, whether the product takes the masked path
(the density guard: on at 25 % zeros, off at 13 %); test_density_guard reads it.  The A^T side of the issue is not built
(docs/design/09_next.md item 9): there is no Y_MASK."""
import numpy as np
import pytest

import attempt_reference as ar
import attempt_scenario as sc
from conftest import set_tune
from cuopt_amd import capi
from test_attempt_layouts_gpu import prepared

pytestmark = pytest.mark.gpu
INF = np.inf
BUFFERS = ("X", "Y", "ATY", "X_OTHER", "Y_OTHER", "ATY_OTHER", "SUM_X", "SUM_Y", "XBAR", "PART_A", "PART_AT")
M_SIZED = ("Y", "Y_OTHER", "SUM_Y")


@pytest.fixture(autouse=True)
def multi_launch_kernels(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")


def make_lp(m, n, k, seed, long_rows=(), avoid=None):
    """m x n, k entries per row (long_rows: {row: entries}), x >= 0, equalities on the first half of the rows and '>=' rows behind;
    avoid = (first row, last row, first column, last column): these rows have no entry in these columns (an empty tile)"""
    rng = np.random.default_rng(seed)
    lens = np.full(m, min(k, n))
    for r, l in dict(long_rows).items():
        lens[r] = l
    rows = []
    for i in range(m):
        allowed = np.arange(n)
        if avoid and avoid[0] <= i < avoid[1]:
            allowed = np.concatenate([allowed[:avoid[2]], allowed[avoid[3]:]])
        rows.append(np.sort(rng.choice(allowed, size=min(lens[i], len(allowed)), replace=False)))
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    idx = np.concatenate(rows).astype(np.int32)
    val = rng.standard_normal(len(idx))
    xs = np.where(rng.random(n) < 0.5, 0.0, rng.random(n) + 0.5)
    b = np.add.reduceat(val * xs[idx], off[:-1])
    lo, hi = b.copy(), b.copy()
    hi[m // 2:] = INF
    lo[m // 2:] -= rng.random(m - m // 2)
    p = dict(m=m, n=n, offsets=off, indices=idx, values=val, c=rng.standard_normal(n), lo=lo, hi=hi, lb=np.zeros(n), ub=np.full(n, INF),
             maximize=False, objective_offset=0.0)
    return p, np.abs(rng.standard_normal(n)) * (rng.random(n) < 0.7), rng.standard_normal(m)


# id -> (m, n, k, CUOPT_AMD_TUNE geometry, long rows, rows / columns of an empty tile)
GEOMETRY = {
    "n200-slab125": (320, 200, 7, dict(panel_nnz=2048, slab_bytes=1000), {}, None),       # n % 64 = 8, slabs start mid-word
    "n48-slab20": (300, 48, 7, dict(panel_nnz=2048, slab_bytes=160), {}, None),           # n < 64, slabs narrower than a word
    "n256-slab125": (320, 256, 7, dict(panel_nnz=2048, slab_bytes=1000), {}, None),       # no tail word
    "chunks-empty-tile": (1500, 300, 10, dict(panel_nnz=20000, slab_bytes=800), {}, (0, 1500, 100, 200)),  # tiles of ~5 000 entries
    "long-and-own-rows": (400, 4500, 6, dict(panel_nnz=2048, slab_bytes=8000), {7: 200, 300: 4200}, None),
}
_lps = {}


def lp(name):
    if name not in _lps:
        m, n, k, _, long_rows, avoid = GEOMETRY[name]
        _lps[name] = make_lp(m, n, k, 11 + len(_lps), long_rows, avoid)
        if long_rows:  # the builder's rules (pdlp_kernels.hpp): a row beyond kLongRow = 128 entries inside the panels is summed by
            # its wave (any_long), a row beyond kPanelOwnRow = 4096 gets a workgroup of its own behind the panels
            lens = np.diff(_lps[name][0]["offsets"])
            assert ((lens > 128) & (lens <= 4096)).sum() == 1 and (lens > 4096).sum() == 1, lens.max()
    return _lps[name]


def open_dev(name, zero_skip, monkeypatch):
    p, x0, y0 = lp(name)
    set_tune(monkeypatch, panel_seg=0, dense=0, zero_skip=zero_skip, **GEOMETRY[name][3])
    raw = capi.Device(p)
    lay = raw.layout()
    assert lay["A"]["layout"] == "panel" and lay["A"]["row_sums"] == "by_row" and lay["A"]["slabs"] >= 2, lay
    if GEOMETRY[name][4]:  # (A's workgroups: the panels, which panel_nnz=2048 makes of its ~6 800 other entries, and ONE own row)
        own = int((np.diff(p["offsets"]) > 4096).sum())
        panels_at_least = -(-(int(p["offsets"][-1]) - 4200) // 2048)
        assert own == 1 and lay["A"]["workgroups"] >= panels_at_least + own, lay
    dev = prepared(raw, p, x0, y0)[0]
    return raw, dev, p


def record(raw, p, masked):
    out = {k: raw.download(k, p["m"] if k in M_SIZED else p["n"] if not k.startswith("PART") else 8192) for k in BUFFERS}
    out["ctl"] = ar.ctl_dict(raw.ctl())
    if masked:
        words = raw.download("XBAR_MASK", (p["n"] + 63) // 64).view(np.uint64)
        want = np.packbits(np.concatenate([out["XBAR"] != 0.0, np.zeros(-p["n"] % 64, bool)]), bitorder="little").view(np.uint64)
        assert np.array_equal(words, want), "XBAR_MASK is not the bits of xbar != 0"
    return out


def same_bits(a, b, tag):
    for k in BUFFERS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (tag, k)
    ka = {k: np.float64(v).view(np.uint64) if isinstance(v, float) else v for k, v in a["ctl"].items()}
    kb = {k: np.float64(v).view(np.uint64) if isinstance(v, float) else v for k, v in b["ctl"].items()}
    assert ka == kb, (tag, a["ctl"], b["ctl"])


def both(name, monkeypatch, script, on=2):
    """script(raw, dev, p, masked) -> list of records; run with zero_skip=2 (or 1) and 0, compared record by record"""
    runs = []
    for zs in (on, 0):
        raw, dev, p = open_dev(name, zs, monkeypatch)
        if zs == 0:
            with pytest.raises(capi.CuOptError):
                raw.download("XBAR_MASK", 1)
        runs.append(script(raw, dev, p, zs != 0))
        if zs == 2:  # the A product of EVERY attempt took the masked branch (the kernel counts its masked launches)
            launches, made = int(raw.download("ZS_LAUNCHES", 1).view(np.uint64)[0]), raw.ctl().attempts
            assert launches == made > 0, (name, launches, made)
        raw.close()
    assert len(runs[0]) == len(runs[1]) and len(runs[0]) > 0
    for i, (a, b) in enumerate(zip(*runs)):
        same_bits(a, b, "%s record %d" % (name, i))
    return runs[1]


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_attempts_bit_for_bit(name, monkeypatch):
    """64 attempts, a forced rejection among them, one at a time"""
    def script(raw, dev, p, masked):
        recs, S = [], ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
        prob = sc.download_problem(dev)
        for i in range(64):
            if i == 20:
                held = sc.snapshot(dev)
                y_back = sc.force_rejection(dev, S, prob, dev.sp, held, name)
            raw.attempts(1)
            recs.append(record(raw, p, masked))
            if i == 20:
                assert recs[-1]["ctl"]["steps_taken"] == recs[-2]["ctl"]["steps_taken"], "attempt 20 was to be rejected"
                dev.put("Y", y_back)
        return recs
    recs = both(name, monkeypatch, script)
    accepted = recs[-1]["ctl"]["steps_taken"]
    assert 20 <= accepted < 64 and recs[-1]["ctl"]["error"] == 0, recs[-1]["ctl"]
    zeros = np.mean([np.mean(r["XBAR"] == 0.0) for r in recs[32:]])
    print("ZEROS %s: %.3f of xbar over the last 32 attempts" % (name, zeros))
    assert zeros > 0.05, "the iterates never sat on the bound: the masked path skipped nothing"


@pytest.mark.parametrize("name", ["n200-slab125", "n48-slab20", "chunks-empty-tile"])
@pytest.mark.parametrize("pattern", ["all-zero", "all-nonzero", "alternating"])
def test_uploaded_patterns(name, pattern, monkeypatch):
    """x = 0 and a gradient of +1 / -1 per column: x' = 0 resp. tau, so xbar is zero exactly where the gradient is positive"""
    def script(raw, dev, p, masked):
        n = p["n"]
        plus = dict([("all-zero", np.ones(n, bool)), ("all-nonzero", np.zeros(n, bool)), ("alternating", np.arange(n) % 2 == 0)])[pattern]
        raw.attempts(2)
        dev.put("X", np.zeros(n))
        dev.put("ATY", dev.get("C") - np.where(plus, 1.0, -1.0))
        raw.attempts(1)
        r = record(raw, p, masked)
        assert np.array_equal(r["XBAR"] == 0.0, plus), "the uploads did not make the pattern"
        raw.attempts(3)
        return [r, record(raw, p, masked)]
    both(name, monkeypatch, script)


@pytest.mark.parametrize("name", ["n200-slab125", "long-and-own-rows"])
def test_special_values(name, monkeypatch):
    """-0.0, NaN, +inf and a denormal in xbar at columns that rows gather: -0.0 counts as zero, the others do not, and every output is
    what the unmasked product gives (a row that gathers the NaN has a NaN sum, which the dual projection turns into y' = 0.0)"""
    def script(raw, dev, p, masked):
        n = p["n"]
        used = np.flatnonzero(np.bincount(p["indices"], minlength=n) > 0)
        jm, jn, ji, jd = used[[1, len(used) // 3, len(used) // 2, len(used) - 2]]
        raw.attempts(2)
        x, aty, c, lb, ub = np.zeros(n), dev.get("C") - 1.0, dev.get("C"), dev.get("LB"), dev.get("UB")
        aty[1::3] += 2.0                                # a third of the columns move: a mixed bitmap around the special ones
        lb[jm], ub[jm], aty[jm] = -INF, -0.0, c[jm] + 1.0  # x' = min(tau, -0.0) = -0.0, xbar = (-0.0 - 0.0) + -0.0 = -0.0
        x[jn] = np.nan
        aty[ji] = INF                                   # x' = +inf, xbar = +inf
        c[jd], aty[jd] = 0.0, 5e-320                    # x' = tau * 5e-320: a denormal
        for k, v in (("LB", lb), ("UB", ub), ("C", c), ("X", x), ("ATY", aty)):
            dev.put(k, v)
        raw.attempts(1)
        r = record(raw, p, masked)
        xb = r["XBAR"]
        assert xb[jm] == 0.0 and np.signbit(xb[jm]) and np.isnan(xb[jn]) and xb[ji] == INF and 0.0 < xb[jd] < 2.3e-308, xb[[jm, jn, ji, jd]]
        # (the dual projection max(low, min(up, 0)) answers 0.0 to a NaN row sum: the rows that gather the NaN show it that way)
        rows = np.flatnonzero(np.add.reduceat(p["indices"] == jn, p["offsets"][:-1]) > 0)
        assert len(rows) > 0 and any((r[k][rows] == 0.0).all() for k in ("Y", "Y_OTHER")), "no row gathered the NaN"
        return [r]
    both(name, monkeypatch, script)


def test_density_guard(monkeypatch):
    """zero_skip=1: the flag for the NEXT attempt follows the zeros of xbar with hysteresis -- up from 25 % zeros, down from 13 %,
    unchanged in between -- the count is exact, and every result is the unmasked one whichever path formed it"""
    fractions = (0.0, 0.6, 0.2, 0.05, 0.2, 0.6, 0.2)
    want_flag = (0, 1, 1, 0, 0, 1, 1)
    flags = []

    def script(raw, dev, p, masked):
        n, recs = p["n"], []
        order = np.random.default_rng(3).permutation(n)
        assert raw.ctl().zskip == 0
        for f in fractions:
            zero = np.zeros(n, bool)
            zero[order[:int(round(f * n))]] = True
            dev.put("X", np.zeros(n))
            dev.put("ATY", dev.get("C") - np.where(zero, 1.0, -1.0))
            c = raw.attempts(1)
            r = record(raw, p, masked)
            assert np.array_equal(r["XBAR"] == 0.0, zero)
            if masked:
                assert c.zs_nonzeros == n - int(zero.sum()), (f, c.zs_nonzeros)
                flags.append(c.zskip)
            else:
                assert c.zskip == 0 and c.zs_nonzeros == 0
            recs.append(r)
        return recs
    seen = []

    def counted(raw, dev, p, masked):
        recs = script(raw, dev, p, masked)
        if masked:
            seen.append(int(raw.download("ZS_LAUNCHES", 1).view(np.uint64)[0]))
        return recs
    both("n200-slab125", monkeypatch, counted, on=1)
    assert tuple(flags) == want_flag, flags
    assert seen == [sum((0,) + want_flag[:-1])], (seen, "an attempt takes the masked branch exactly when the flag in front of it is up")


def test_slabs_wider_than_the_window(monkeypatch):
    """500 000 columns in the default geometry: 3 slabs of 166 667 columns either way -- the bitmap changes no layout -- of which
    the LDS window holds the first 147 456; the columns behind it are gathered unconditionally.  The iterate and the control block
    every 10 iterations over 120, then a whole solve with its restarts: identical"""
    from cuopt_amd import synthetic
    p = synthetic.generate(100_000, 500_000, 5, seed=4)
    traces, solves, launches = [], [], 0
    for zs in (2, 0):
        set_tune(monkeypatch, zero_skip=zs)
        raw = capi.Device(p)
        lay = raw.layout()["A"]
        assert lay["layout"] == "panel" and lay["row_sums"] == "by_row" and lay["slabs"] == 3, lay
        prepared(raw, p, np.zeros(p["n"]), np.zeros(p["m"]))
        trace = []
        for target in range(10, 121, 10):
            c = raw.run(target)
            trace.append(dict(X=raw.download("X", p["n"]), Y=raw.download("Y", p["m"]), ATY=raw.download("ATY", p["n"]), ctl=ar.ctl_dict(c)))
        if zs:
            launches = int(raw.download("ZS_LAUNCHES", 1).view(np.uint64)[0])
            assert launches == raw.ctl().attempts >= 120, (launches, raw.ctl().attempts)
            assert np.mean(raw.download("XBAR", p["n"])[147_456:166_667] == 0.0) > 0.05, "no zero behind the window"
        raw.close()
        traces.append(trace)
        solves.append(capi.solve(p, method=1, iteration_limit=120, tol=1e-12))
    for i, (a, b) in enumerate(zip(*traces)):
        assert a["ctl"] == b["ctl"], (i, a["ctl"], b["ctl"])
        for k in ("X", "Y", "ATY"):
            assert ar.bits_equal(a[k], b[k]), (i, k)
    a, b = solves
    assert a["steps_taken"] == b["steps_taken"] >= 120 and a["num_restarts"] == b["num_restarts"], (a["steps_taken"], b["steps_taken"], a["num_restarts"], b["num_restarts"])
    for k in ("x", "y", "reduced_cost"):
        assert ar.bits_equal(a[k], b[k]), k
