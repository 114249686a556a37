"""GPU: the order in which the row-sum panels request a chunk (CUOPT_AMD_TUNE=panel_req_order, on by default) changes no bit.

With panel_req_order=1 a chunk's request issues the row extents first -- of the first four slots always, of the other three only in a
panel of more than 2 048 rows -- and then the stream, round by round behind uniform branches, every byte offset formed in front of the
first load; the row sums walk only the slots the panel has.  With 0 the stream goes first, through the switch on the number of rounds,
and all seven extents follow.  The loads fetch the same entries and the row sums add the same addends in the same order, so every test
runs the same inputs both ways, with the chunks column-sorted and not (panel_sort), and compares raw 64-bit patterns: the plain
products, attempts with and without the zero skip, a convergence evaluation, two solves; the stored arrays are the same either way.

The geometries are those of test_panel_sorted_chunks_gpu.py (an empty tile, chunks shorter than one round of 512 lanes, a row beyond
128 entries, a row with a workgroup of its own, the dense one-slab case, tiles of a full 4 096-entry chunk and a partial one) and two
more: 21 250 x 2 000 with 80 per row in one slab, whose tiles hold 3 073 .. 3 584 entries -- seven rounds, the last one partial, the
headline workload's case -- and 1 500 000 x 4 000 with 2 per row, whose panels hold ~2 930 rows: the only case in which the extents
of the upper three slots are requested and summed (a panel is sized rows / 512, so nothing below 1 050 000 rows has such a panel;
plain products only, to keep it short).  test_chunk_lengths asserts from the stored tile boundaries that the chunks met are the ones
the request distinguishes."""
import numpy as np
import pytest

import attempt_reference as ar
from conftest import set_tune
from cuopt_amd import capi, synthetic
from test_attempt_layouts_gpu import prepared
from test_panel_sorted_chunks_gpu import GEOMETRY as SORTED_GEOMETRY, lp as sorted_lp, row_sums_left_to_right
from test_zero_skip_gpu import record, same_bits

pytestmark = pytest.mark.gpu
CHUNK, LANES = 4096, 512  # kPanelChunk, kPanelThreads

GEOMETRY = dict(SORTED_GEOMETRY)
GEOMETRY["seven-rounds"] = dict(panel_nnz=60000, slab_bytes=16000)  # 2 000 columns = 16 000 bytes: one slab; 512 panels of ~3 320 entries
GEOMETRY["many-rows"] = dict(panel_nnz=60000, slab_bytes=8000)      # 512 panels of ~2 930 rows, ~5 860 entries in 4 slabs
ATTEMPT_GEOMETRY = [k for k in GEOMETRY if k != "many-rows"]
_seven, _rows = [], []


@pytest.fixture(autouse=True)
def multi_launch_kernels(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")


def lp(name):
    if name == "seven-rounds":
        if not _seven:
            rng = np.random.default_rng(11)
            _seven.append((synthetic.generate(21250, 2000, 80, seed=12), np.abs(rng.standard_normal(2000)) * (rng.random(2000) < 0.7), rng.standard_normal(21250)))
        return _seven[0]
    if name == "many-rows":
        if not _rows:
            _rows.append((synthetic.generate(1500000, 4000, 2, seed=13), None, None))
        return _rows[0]
    return sorted_lp(name)


def open_raw(name, order, sort, zero_skip, monkeypatch, analysis=False):
    p = lp(name)[0]
    set_tune(monkeypatch, panel_seg=0, dense=0, zero_skip=zero_skip, panel_sort=sort, panel_req_order=order, **GEOMETRY[name])
    raw = capi.Device(p, analysis=capi.Analysis(p, reorder=False)) if analysis else capi.Device(p)
    lay = raw.layout()
    for side in ("A", "At"):
        assert lay[side]["layout"] == "panel" and lay[side]["row_sums"] == "by_row", lay
        assert raw.panel_words(side)["sorted"] == bool(sort), (name, side, sort)
    return raw, p


def chunk_lengths(tile_ptr):
    out = []
    for t in range(len(tile_ptr) - 1):
        for c0 in range(int(tile_ptr[t]), int(tile_ptr[t + 1]), CHUNK):
            out.append(min(c0 + CHUNK, int(tile_ptr[t + 1])) - c0)
    return np.array(out, np.int64)


def test_chunk_lengths(monkeypatch):
    """the chunks of the geometries, from the stored tile boundaries: one round, an odd and an even number of full rounds, a partial last
    round, seven rounds, eight; the A side of the seven-round matrix has tiles of 3 073 .. 3 584 entries only; the many-rows panels pass 2 048 rows
    and no other geometry's do"""
    lens, rows_per_panel = {}, {}
    for name in GEOMETRY:
        raw, p = open_raw(name, 1, 1, 0, monkeypatch)
        per = []
        for side, nrows in (("A", p["m"]), ("At", p["n"])):
            w = raw.panel_words(side)
            per.append(chunk_lengths(w["tile_ptr"]))
            if (name, side) == ("seven-rounds", "A"):
                seven = per[-1]
            rows_per_panel[name, side] = nrows / w["panels"]  # (panels are contiguous row ranges: the largest holds at least the mean)
        raw.close()
        lens[name] = np.concatenate(per)
    every = np.concatenate(list(lens.values()))
    rounds, full, partial = (every + LANES - 1) // LANES, every // LANES, every % LANES != 0
    assert (rounds == 1).any() and (rounds == 7).any() and (rounds == 8).any(), np.unique(rounds)
    assert ((full >= 1) & (full % 2 == 1)).any() and ((full >= 2) & (full % 2 == 0)).any() and partial.any() and (~partial).any()
    assert (every == CHUNK).any(), "no full chunk"
    assert 3073 <= seven.min() and seven.max() <= 3584, (seven.min(), seven.max())  # (its A side: 41 or 42 rows of 80)
    assert rows_per_panel["many-rows", "A"] > 4 * LANES, rows_per_panel
    print("CHUNKS rounds met: %s; rows per panel (mean): %s" % (np.unique(rounds), {k: round(v) for k, v in rows_per_panel.items()}))


@pytest.mark.parametrize("sort", [1, 0])
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_plain_products(name, sort, monkeypatch):
    """both sides: the two orders agree bit for bit on every row, and equal the left-to-right row sum bit for bit on every row the kernel
    sums left to right (rows of at most 128 entries)"""
    p = lp(name)[0]
    m, n = p["m"], p["n"]
    rng = np.random.default_rng(2)
    x, y = rng.standard_normal(n), rng.standard_normal(m)
    to, ti, tv = capi.csr_transpose(m, n, p["offsets"], p["indices"], p["values"])
    want = [(row_sums_left_to_right(m, p["offsets"], p["indices"], p["values"], x), np.diff(p["offsets"])),
            (row_sums_left_to_right(n, to, ti, tv, y), np.diff(to))] if name != "many-rows" else None
    got = []
    for order in (1, 0):
        raw, _ = open_raw(name, order, sort, 0, monkeypatch)
        got.append((raw.spmv(x, False, m), raw.spmv(y, True, n)))
        raw.close()
    for side in (0, 1):
        assert ar.bits_equal(got[0][side], got[1][side]), (name, side)
        if want is not None:
            ref, lens = want[side]
            short = lens <= 128
            assert ar.bits_equal(got[0][side][short], ref[short]), (name, side)
    if want is None:  # (the transpose's rows hold 750 entries each: the A side, two per row, against the plain left-to-right sum)
        idx, val = p["indices"], p["values"]
        ref = row_sums_left_to_right(m, p["offsets"], idx, val, x)
        assert ar.bits_equal(got[0][0], ref), name


@pytest.mark.parametrize("sort", [1, 0])
@pytest.mark.parametrize("zero_skip", [2, 0])
@pytest.mark.parametrize("name", ATTEMPT_GEOMETRY)
def test_attempts_and_evaluation(name, zero_skip, sort, monkeypatch):
    """three attempts one at a time (x', xbar, y', A^T y', both running sums, both partial arrays, the control block), then one
    convergence evaluation of the current iterate (its eight scalars, the reduced costs, A^T y and A x of the unscaled problem)"""
    runs = []
    for order in (1, 0):
        raw, p = open_raw(name, order, sort, zero_skip, monkeypatch)
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
        same_bits(a, b, "%s zero_skip=%d sort=%d attempt %d" % (name, zero_skip, sort, i))
    assert runs[0][0][-1]["ctl"]["error"] == 0 and runs[0][0][-1]["ctl"]["steps_taken"] >= 1, runs[0][0][-1]["ctl"]
    for k in runs[0][1]:
        assert ar.bits_equal(runs[0][1][k], runs[1][1][k]), (name, "evaluation", k)
    assert np.isfinite(runs[0][1]["scalars"]).all()


@pytest.mark.parametrize("name", ATTEMPT_GEOMETRY)
def test_stored_arrays(name, monkeypatch):
    """the request order is the kernels' alone: the host construction == the device construction (checksums of every array) with it on,
    and the words and tile boundaries are those stored with it off"""
    host, _ = open_raw(name, 1, 1, 0, monkeypatch)
    dev, _ = open_raw(name, 1, 1, 0, monkeypatch, analysis=True)
    off, _ = open_raw(name, 0, 1, 0, monkeypatch)
    a, b = host.layout_checksums(), dev.layout_checksums()
    assert int(a[15]) & 3 == 3, "both sides in panels"
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, off.layout_checksums())
    for side in ("A", "At"):
        w, w0 = host.panel_words(side), off.panel_words(side)
        np.testing.assert_array_equal(w["tile_ptr"], w0["tile_ptr"])
        np.testing.assert_array_equal(w["col"], w0["col"])
    for d in (host, dev, off):
        d.close()


@pytest.mark.parametrize("sort", [1, 0])
@pytest.mark.parametrize("mode", [1, 4])
def test_solves(mode, sort, monkeypatch):
    """120 iterations of a 3000 x 3000 LP, 8 entries per row, in 12 panels of 6 slabs, adaptive (mode 1) and reflected Halpern (mode 4,
    the only test that runs the Halpern walkers), over sorted and unsorted chunks: the result's scalars and the three solution vectors"""
    p = synthetic.generate(3000, 3000, 8, seed=6)
    out = []
    for order in (1, 0):
        set_tune(monkeypatch, panel_seg=0, panel_sort=sort, panel_req_order=order, panel_nnz=2048, slab_bytes=4096)
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
