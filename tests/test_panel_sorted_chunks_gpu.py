"""GPU: storing every chunk of the row-sum panels in column order (CUOPT_AMD_TUNE=panel_sort, on by default) changes no bit.

build_panels / k_panel_sort store the entries of a chunk in ascending order of (column inside the slab, slot) and every entry carries
its slot -- its position inside the chunk in (row, CSR) order -- beside its column; a lane gathers vec[column] and writes its product
to prod[slot], so the row sums read what they always read in the order they always did.  Every test runs the same inputs with
panel_sort=1 and panel_sort=0 (the storage and the kernels' path as they were) and compares raw 64-bit patterns: the plain products,
attempts with and without the zero skip, a convergence evaluation, two solves.  The stored words themselves are read back: per chunk
the columns ascend, the slots are a permutation of 0 .. len - 1, and word i names the entry the unsorted storage keeps at that slot;
the host construction and the device construction (the bitonic sort behind the placement) give the same arrays.

The geometries are those of test_zero_skip_gpu.py (an empty tile, chunks shorter than one round of 512 lanes, a row beyond 128
entries, a row with a workgroup of its own), a fully dense 64 x 40 matrix in one slab, where every column repeats inside a chunk and
only the slot orders the equal columns, and a 4.4e6-entry matrix whose tiles are a full chunk and a partial one (a slot counts from
its chunk's start, not its tile's; no smaller matrix has such a tile).

Not tested at size: slabs wider than 2^20 columns (more than 1.6e7 columns) keep the unsorted storage -- the branch panel_sort=0 takes."""
import numpy as np
import pytest

import attempt_reference as ar
from conftest import set_tune
from cuopt_amd import capi, synthetic
from test_attempt_layouts_gpu import prepared
from test_zero_skip_gpu import GEOMETRY as ZS_GEOMETRY, lp as zs_lp, make_lp, record, same_bits

pytestmark = pytest.mark.gpu
CHUNK = 4096  # kPanelChunk

# id -> CUOPT_AMD_TUNE geometry
GEOMETRY = {k: ZS_GEOMETRY[k][3] for k in ("n200-slab125", "n48-slab20", "chunks-empty-tile", "long-and-own-rows")}
GEOMETRY["dense-one-slab"] = dict(panel_nnz=2048, slab_bytes=4096)  # 40 columns = 320 bytes: one slab; panels of 51 and 13 full rows
# 55 000 x 2 000, 80 per row: 4.4e6 entries in 512 panels of ~8 600 over 2 slabs -- tiles of ~4 300 entries, i.e. a full chunk and a partial
# one.  (The panels are sized nonzeros / 512 however small panel_nnz is, so nothing below 2.1e6 entries has a tile of two chunks: the
# tiles of "chunks-empty-tile" hold ~1 000 entries.)
GEOMETRY["two-chunk-tiles"] = dict(panel_nnz=60000, slab_bytes=8000)
_dense, _big = [], []


@pytest.fixture(autouse=True)
def multi_launch_kernels(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")


def lp(name):
    if name == "two-chunk-tiles":
        if not _big:
            rng = np.random.default_rng(9)
            _big.append((synthetic.generate(55000, 2000, 80, seed=8), np.abs(rng.standard_normal(2000)) * (rng.random(2000) < 0.7), rng.standard_normal(55000)))
        return _big[0]
    if name != "dense-one-slab":
        return zs_lp(name)
    if not _dense:
        _dense.append(make_lp(64, 40, 40, 5))
        assert (np.diff(_dense[0][0]["offsets"]) == 40).all()
    return _dense[0]


def open_raw(name, sort, zero_skip, monkeypatch, analysis=False):
    p = lp(name)[0]
    set_tune(monkeypatch, panel_seg=0, dense=0, zero_skip=zero_skip, panel_sort=sort, **GEOMETRY[name])
    raw = capi.Device(p, analysis=capi.Analysis(p, reorder=False)) if analysis else capi.Device(p)
    lay = raw.layout()
    for side in ("A", "At"):
        assert lay[side]["layout"] == "panel" and lay[side]["row_sums"] == "by_row", lay
        assert raw.panel_words(side)["sorted"] == bool(sort), (name, side, sort)
    assert (lay["A"]["slabs"] == 1) == (name == "dense-one-slab"), lay
    return raw, p


def row_sums_left_to_right(m, off, idx, val, x):
    """sum = 0.0; sum = sum + a * x[j], entry by entry in CSR order: what a lane of the row kernel forms"""
    out, lens = np.zeros(m), np.diff(off)
    for k in range(int(lens.max())):
        rows = np.flatnonzero(lens > k)
        at = off[rows] + k
        out[rows] = out[rows] + val[at] * x[idx[at]]
    return out


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_plain_products(name, monkeypatch):
    """both sides: sorted == unsorted bit for bit on every row, and both equal the left-to-right row sum bit for bit on every row the
    kernel sums left to right (a row beyond 128 entries is summed by its wave or its own workgroup in a fixed tree: rtol 1e-12 of
    sum |a x|, the layouts' contract for such rows, in both storages)"""
    p = lp(name)[0]
    m, n = p["m"], p["n"]
    rng = np.random.default_rng(2)
    x, y = rng.standard_normal(n), rng.standard_normal(m)
    to, ti, tv = capi.csr_transpose(m, n, p["offsets"], p["indices"], p["values"])
    want = [(row_sums_left_to_right(m, p["offsets"], p["indices"], p["values"], x), np.diff(p["offsets"]),
             np.add.reduceat(np.abs(p["values"] * x[p["indices"]]), p["offsets"][:-1])),
            (row_sums_left_to_right(n, to, ti, tv, y), np.diff(to),
             np.add.reduceat(np.abs(tv * y[ti]), np.minimum(to[:-1], len(ti) - 1)) if name == "two-chunk-tiles" else None)]
    got = []
    for sort in (1, 0):
        raw, _ = open_raw(name, sort, 0, monkeypatch)
        got.append((raw.spmv(x, False, m), raw.spmv(y, True, n)))
        raw.close()
    for side in (0, 1):
        assert ar.bits_equal(got[0][side], got[1][side]), (name, side)
        ref, lens, scale = want[side]
        short = lens <= 128
        assert ar.bits_equal(got[0][side][short], ref[short]), (name, side)
        if (~short).any():
            assert (side, name) in ((0, "long-and-own-rows"), (1, "two-chunk-tiles"))
            assert (np.abs(got[0][side][~short] - ref[~short]) <= 1e-12 * scale[~short]).all(), (name, side)


@pytest.mark.parametrize("name", list(GEOMETRY))
@pytest.mark.parametrize("zero_skip", [2, 0])
def test_attempts_and_evaluation(name, zero_skip, monkeypatch):
    """three attempts one at a time (x', xbar, y', A^T y', both running sums, both partial arrays, the control block), then one
    convergence evaluation of the current iterate (its eight scalars, the reduced costs, A^T y and A x of the unscaled problem)"""
    runs = []
    for sort in (1, 0):
        raw, p = open_raw(name, sort, zero_skip, monkeypatch)
        _, x0, y0 = lp(name)
        prepared(raw, p, x0, y0)
        recs = []
        for _ in range(3):
            raw.attempts(1)
            recs.append(record(raw, p, zero_skip != 0))
        if zero_skip == 2:
            launches = int(raw.download("ZS_LAUNCHES", 1).view(np.uint64)[0])
            assert launches == raw.ctl().attempts == 3, (name, launches)
        ev = dict(scalars=np.array(list(raw.eval(capi.CURRENT).values())), rc=raw.download("RC_CURRENT", p["n"]), aty=raw.download("ATY_U_CURRENT", p["n"]),
                  ax=raw.download("AX_U_CURRENT", p["m"]))
        raw.close()
        runs.append((recs, ev))
    for i, (a, b) in enumerate(zip(runs[0][0], runs[1][0])):
        same_bits(a, b, "%s zero_skip=%d attempt %d" % (name, zero_skip, i))
    assert runs[0][0][-1]["ctl"]["error"] == 0 and runs[0][0][-1]["ctl"]["steps_taken"] >= 1, runs[0][0][-1]["ctl"]
    for k in runs[0][1]:
        assert ar.bits_equal(runs[0][1][k], runs[1][1][k]), (name, "evaluation", k)
    assert np.isfinite(runs[0][1]["scalars"]).all()


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_stored_words(name, monkeypatch):
    """the host construction == the device construction (checksums of every array), and the words of both sides chunk by chunk"""
    host, p = open_raw(name, 1, 0, monkeypatch)
    dev, _ = open_raw(name, 1, 0, monkeypatch, analysis=True)
    a, b = host.layout_checksums(), dev.layout_checksums()
    assert int(a[15]) & 3 == 3, "both sides in panels"
    np.testing.assert_array_equal(a, b)
    plain, _ = open_raw(name, 0, 0, monkeypatch)
    chunks = longest = 0
    for side in ("A", "At"):
        ws, w0 = [d.panel_words(side) for d in (host, dev)], plain.panel_words(side)
        np.testing.assert_array_equal(ws[0]["col"], ws[1]["col"])
        w = ws[0]
        np.testing.assert_array_equal(w["tile_ptr"], w0["tile_ptr"])
        S, slab_w, tp = w["slabs"], w["slab_w"], w["tile_ptr"]
        assert w["panels"] * S + 1 == len(tp) and tp[-1] == len(w["col"]) == len(w0["col"])
        for t in range(len(tp) - 1):
            for c0 in range(int(tp[t]), int(tp[t + 1]), CHUNK):
                c1 = min(c0 + CHUNK, int(tp[t + 1]))
                word = w["col"][c0:c1].view(np.uint32)
                low, slot = (word & 0xFFFFF).astype(np.int64), (word >> 20).astype(np.int64)
                assert (np.diff(low) >= 0).all(), (name, side, t, c0)
                assert (np.diff(low * CHUNK + slot) > 0).all(), (name, side, t, c0, "equal columns: ascending slots")
                np.testing.assert_array_equal(np.sort(slot), np.arange(c1 - c0))
                assert (low < slab_w).all()
                np.testing.assert_array_equal(w0["col"][c0 + slot], (t % S) * slab_w + low)  # the entry the slot held unsorted
                chunks, longest = chunks + 1, max(longest, c1 - c0)
    for d in (host, dev, plain):
        d.close()
    print("CHUNKS %s: %d chunks, the longest %d entries" % (name, chunks, longest))
    if name == "two-chunk-tiles":
        assert longest == CHUNK, "no tile of several chunks"


@pytest.mark.parametrize("mode", [1, 4])
def test_solves(mode, monkeypatch):
    """120 iterations of a 3000 x 3000 LP, 8 entries per row, in 12 panels of 6 slabs, adaptive (mode 1) and reflected Halpern (mode 4):
    the result's scalars and the three solution vectors"""
    p = synthetic.generate(3000, 3000, 8, seed=6)
    out = []
    for sort in (1, 0):
        set_tune(monkeypatch, panel_seg=0, panel_sort=sort, panel_nnz=2048, slab_bytes=4096)
        raw = capi.Device(p)
        lay = raw.layout()
        assert lay["A"]["layout"] == lay["At"]["layout"] == "panel" and lay["A"]["slabs"] == 6 and raw.panel_words("A")["sorted"] == bool(sort), lay
        raw.close()
        out.append(capi.solve(p, method=1, pdlp_solver_mode=mode, iteration_limit=120, tol=1e-12))
    a, b = out
    assert a["return_code"] == b["return_code"] == 0 and a["steps_taken"] >= 120, (a["return_code"], a["steps_taken"])
    for k in ("status", "steps_taken", "attempted_steps", "returned_average", "num_restarts", "num_major_iterations"):
        assert a[k] == b[k], (k, a[k], b[k])
    for k in ("objective", "primal_objective", "dual_objective", "gap", "relative_gap", "l2_primal_residual", "l2_dual_residual",
              "l2_relative_primal_residual", "l2_relative_dual_residual", "step_size", "primal_weight"):
        assert ar.bits_equal(a[k], b[k]), (k, a[k], b[k])
    for k in ("x", "y", "reduced_cost"):
        assert ar.bits_equal(a[k], b[k]), k
