"""GPU: the tail of the two panel walkers -- the epilogue operands requested before the final chunk's row sums -- on LPs cut into the
panel shapes at which that tail can go wrong, every attempt against the stage-by-stage reference (tests/attempt_reference.py).

panel_spmv_block (rows per lane) and panel_seg_block (row sums by nonzero) peel their final chunk, request the operands of a lane's
first four rows there and apply the epilogue to them behind the row sums (spmv_panel.hpp).  The LP `shapes` below is cut, on the A
side, into exactly these panels (the cut is restated here from the row lengths and compared with the workgroups layout() reports):

  0  300 rows                           fewer than 512: lanes 300 .. 511 have no row at slot 0
  1  1024 = 512 * 2 rows                the last slot is full
  2  1025 = 512 * 2 + 1 rows            the last slot is filled in lane 0 only
  3  512 rows, all in the first slab    exactly one chunk: the first chunk is the final one
  4  249 rows, one of 4500 nonzeros     that row has a workgroup of its own: a requested slot falls on a "not mine" row
  5  3584 = kPanelMaxRows rows          seven rows per lane, three of them behind the requested four; rows alternate between empty
                                        and one nonzero, so that the row cap, not the 2048 nonzeros, closes the panel
  6  100 rows, all empty                no chunk at all: the loop never runs, the request is issued in front of the epilogue

A tile of more than 4096 nonzeros (several chunks in one tile, a short last one) cannot occur at panel_nnz=2048 on an LP of this
size: the target of a panel is max(2048, min(panel_nnz, nonzeros / 512)), and a single row above the target is a panel only up to
4096 nonzeros (beyond, it gets a workgroup of its own).  The LP `chunks` (2100 x 8000, rows of 1070 nonzeros, one slab, panel_nnz
=6000) has the 2.2 M nonzeros that lift the target: its panels are five rows = 5350 nonzeros, a chunk of 4096 and one of 1254.

The dense-segment variant runs on the LP of tests/test_eval_layouts_gpu.py's dense ids, cut at panel_nnz=2048.

Every LP runs with rows per lane and by nonzero, single attempts through pdlpdev_debug_attempts until an attempt has been seen from
each of cur = 0, 1 x pending_avg = 0, 1 (a first attempt, attempts behind accepted ones, one behind flush_average); each attempt is
checked by attempt_scenario.one_attempt with the bounds attempt_reference derives.  Nothing is compared with another layout."""
import numpy as np
import pytest
from conftest import set_tune

import attempt_reference as ar
import attempt_scenario as sc
from cuopt_amd import capi
from test_attempt_layouts_gpu import prepared
from test_eval_layouts_gpu import open_variant, variant_lp

pytestmark = pytest.mark.gpu
INF = np.inf
THREADS, MAX_ROWS, OWN_ROW, CHUNK, DEPTH = 512, 3584, 4096, 4096, 4  # kPanelThreads, kPanelMaxRows, kPanelOwnRow, kPanelChunk, kPanelEpiDepth


@pytest.fixture(autouse=True)
def multi_launch_kernels(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")  # these LPs are small: keep them off the resident one-workgroup path


def panel_cut(lens, cap):
    """panel_plan's cut restated from the row lengths -> (row0, own rows): rows of more than kPanelOwnRow nonzeros leave the panels;
    a panel takes rows while they fit under the target, at most kPanelMaxRows; the target grows until the panels fit the slots"""
    own = lens > OWN_ROW
    inside = np.where(own, 0, lens)
    nnz, rows = int(inside.sum()), len(lens)

    def cut(tgt):
        row0, start = [0], 0
        while start < rows:
            end, cnt = start, 0
            while end < rows and end - start < MAX_ROWS:
                if cnt > 0 and cnt + inside[end] > tgt:
                    break
                cnt += inside[end]
                end += 1
            row0.append(end)
            start = end
        return row0
    slots = max(64, 512 - int(own.sum()))
    tgt = max(2048, min(cap, (nnz + slots - 1) // slots))
    row0 = cut(tgt)
    for it in range(64):
        w = len(row0) - 1
        if w <= slots or tgt >= cap:
            break
        tgt = min(cap, int(float(tgt) * w / slots * 1.002) + 1 if it == 0 else tgt + tgt // 100 + 1)
        row0 = cut(tgt)
    return np.array(row0), np.nonzero(own)[0]


def _finish(rng, m, n, lens, idx):
    """values, kinds of rows and columns as tests/eval_lps.edge_lp mixes them, a start"""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    p = dict(m=m, n=n, offsets=off, indices=np.concatenate(idx).astype(np.int32), values=rng.standard_normal(int(off[-1])))
    row_kind, col_kind = rng.permutation(np.arange(m) % 5), rng.permutation(np.arange(n) % 5)
    b, w = rng.standard_normal(m), np.abs(rng.standard_normal(m)) + 0.5
    p["lo"] = np.choose(row_kind, [np.full(m, -INF), b - 1.0, b, np.full(m, -INF), b - 1.0])
    p["hi"] = np.choose(row_kind, [b + 3.0, np.full(m, INF), b, np.full(m, INF), b - 1.0 + w])
    p["lb"] = np.choose(col_kind, [-INF, -INF, 0.0, 1.5, 0.0]).astype(np.float64)
    p["ub"] = np.choose(col_kind, [INF, 5.0, INF, 1.5, 5.0]).astype(np.float64)
    p["c"] = rng.standard_normal(n)
    x = np.abs(rng.standard_normal(n)) * (rng.random(n) < 0.7)
    x[col_kind == 3] = 1.5
    return p, x, rng.standard_normal(m)


N_SHAPES, SLAB_BYTES = 6000, 4096          # 12 slabs of 500 columns
SHAPE_ROWS = (300, 1024, 1025, 512, 249, MAX_ROWS, 100)


def shapes_lp(seed=21):
    rng = np.random.default_rng(seed)
    n = N_SHAPES
    one = np.zeros(MAX_ROWS, dtype=np.int64)
    one[0::2] = 1  # (the first row has the nonzero: an empty one would still fit into the panel in front)
    lens = np.concatenate([
        np.r_[np.full(299, 6), 254],                      # 0: 2048 nonzeros, as every panel but the last two: the next row never fits
        np.full(1024, 2),                                 # 1
        np.r_[np.full(1023, 2), 1, 1],                    # 2
        np.full(512, 4),                                  # 3 (columns below)
        np.r_[np.full(200, 10), 4500, np.full(48, 1)],    # 4
        one,                                              # 5: 1792 nonzeros
        np.zeros(100, dtype=np.int64)])                   # 6
    m = len(lens)
    first = np.cumsum((0,) + SHAPE_ROWS)
    slab_w = 500
    idx = [np.sort(rng.choice(slab_w if first[3] <= r < first[4] else n, size=l, replace=False)) for r, l in enumerate(lens)]
    return _finish(rng, m, n, lens, idx) + (first,)


def chunks_lp(seed=22):
    rng = np.random.default_rng(seed)
    m, n, per = 2100, 8000, 1070
    lens = np.full(m, per)
    return _finish(rng, m, n, lens, [np.sort(rng.choice(n, size=per, replace=False)) for _ in range(m)])


_lps = {}


def lp(name):
    if name not in _lps:
        made = shapes_lp() if name == "shapes" else chunks_lp()
        for a in list(made[0].values()) + list(made[1:]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)  # shared between the two walkers' cases
        _lps[name] = made
    return _lps[name]


def open_panels(p, seg, monkeypatch, panel_nnz, slab_bytes):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    set_tune(monkeypatch, dense=0, panel_nnz=panel_nnz, slab_bytes=slab_bytes, panel_seg=seg)
    dev = capi.Device(p)
    lay = dev.layout()
    print("LAYOUT", lay)
    sums = "by_nonzero" if seg else "by_row"
    assert not lay["resident"] and lay["A"]["layout"] == lay["At"]["layout"] == "panel", lay
    assert lay["A"]["row_sums"] == lay["At"]["row_sums"] == sums, lay
    return dev, lay


def every_state(dev, S, prob, tag):
    """single attempts, each checked against the reference, until one has been seen from each (cur, pending_avg); an attempt with no
    average pending at a side that has only been seen with one is had by flush_average in front of it"""
    want = {(0, 0), (0, 1), (1, 0), (1, 1)}
    seen, worst = [], sc.Worst()
    for i in range(16):
        c = dev.ctl()
        key = (c["cur"], c["pending_avg"])
        if key in seen and key[1] == 1 and (key[0], 0) not in seen:
            dev.flush()
            assert dev.ctl()["pending_avg"] == 0
        r = sc.one_attempt(dev, S, prob, dev.sp, "%s attempt %d" % (tag, i), worst)[0]
        sc.assert_decided(r, "%s attempt %d" % (tag, i))
        seen.append((r["cur_before"], r["pending_before"]))
        if set(seen) == want:
            break
    print(worst.line(tag), "states", seen)
    assert seen[0] == (0, 0) and set(seen) == want, (tag, "an attempt from every (cur, pending_avg)", seen)
    assert max(worst.values()) <= 1.0, (tag, worst)


@pytest.mark.parametrize("seg", [0, 1], ids=["rows-per-lane", "by-nonzero"])
def test_tail_shapes(seg, monkeypatch):
    p, x0, y0, first = lp("shapes")
    lens = np.diff(p["offsets"])
    row0, own = panel_cut(lens, 2048)
    # the shapes, from the LP's own row counts
    assert list(row0) == list(first), (row0, first)
    rows = np.diff(row0)
    assert rows[0] < THREADS
    assert rows[1] % THREADS == 0 and rows[2] % THREADS == 1 and rows[1] // THREADS == rows[2] // THREADS == 2
    assert rows[5] == MAX_ROWS > DEPTH * THREADS and lens[row0[5]:row0[6]].sum() < 2048 and set(lens[row0[5]:row0[6]]) == {0, 1}
    assert lens[row0[6]:row0[7]].sum() == 0 and row0[7] == p["m"]
    assert list(own) == [row0[4] + 200] and own[0] - row0[4] < DEPTH * THREADS and lens[own[0]] > OWN_ROW
    dev, lay = open_panels(p, seg, monkeypatch, 2048, SLAB_BYTES)
    slab_w = -(-p["n"] // lay["A"]["slabs"])
    assert lay["A"]["slabs"] == 12 and lay["A"]["workgroups"] == len(rows) + len(own), (lay, len(rows), len(own))
    in3 = p["indices"][p["offsets"][row0[3]]:p["offsets"][row0[4]]]
    assert in3.max() < slab_w and len(in3) <= CHUNK, "panel 3 is one chunk of one tile"
    # the A^T side: whatever the columns give, the same cut
    S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
    t_row0, t_own = panel_cut(S.len_c, 2048)
    assert len(t_own) == 0 and lay["At"]["workgroups"] == len(t_row0) - 1, (lay, len(t_row0) - 1)
    od, S, prob, dr, dc = prepared(dev, p, x0, y0)
    every_state(od, S, prob, "shapes seg=%d" % seg)
    dev.close()


@pytest.mark.parametrize("seg", [0, 1], ids=["rows-per-lane", "by-nonzero"])
def test_tail_several_chunks_in_a_tile(seg, monkeypatch):
    p, x0, y0 = lp("chunks")
    lens = np.diff(p["offsets"])
    row0, own = panel_cut(lens, 6000)
    per_panel = np.diff(p["offsets"][row0])
    assert len(own) == 0 and per_panel.max() > CHUNK and (per_panel[:-1] % CHUNK != 0).all() and per_panel.max() < 2 * CHUNK, per_panel
    dev, lay = open_panels(p, seg, monkeypatch, 6000, 1 << 20)
    assert lay["A"]["slabs"] == 1 and lay["A"]["workgroups"] == len(row0) - 1, (lay, len(row0) - 1)  # one tile per panel: two chunks
    od, S, prob, dr, dc = prepared(dev, p, x0, y0)
    every_state(od, S, prob, "chunks seg=%d" % seg)
    dev.close()


@pytest.mark.parametrize("name", ["dense-panel-rows", "dense-panel-longtail"])
def test_tail_dense_segments(name, monkeypatch):
    p, x0, y0 = variant_lp(name)[:3]
    dev = open_variant(name, p, monkeypatch, panel_nnz=2048) if name == "dense-panel-rows" else open_variant(name, p, monkeypatch)
    od, S, prob, dr, dc = prepared(dev, p, x0, y0)
    every_state(od, S, prob, name)
    dev.close()
