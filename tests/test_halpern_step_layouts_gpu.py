"""GPU: the multi-launch reflected-Halpern step in EVERY SpMV layout against the stage-by-stage reference
(tests/halpern_step_reference.py).

k_primal, the A product with HalpernDualEpilogue, the A^T product with HalpernStepEpilogue, k_halpern_decision and
pdlpdev_halpern_restart -- the step every bit-for-bit test of the resident, lockstep and ray paths is compared with -- of the stream,
panel (rows per lane and long-tail), jagged (8 and 16 waves) and gather-free (both geometries) layouts, with and without the
dense-segment prologue: the 13 ids of tests/test_eval_layouts_gpu.py, on its LPs.  No device hook is used: in Halpern mode
run(steps_taken + 1) makes exactly one step, and every buffer of a step downloads.  Every single step is checked against the state
the device held in front of it: x', xbar, x^{k+1}, y^{k+1} from the device's own y', the empty rows and columns, r2, r, r_first,
r2_min and the counters bit for bit; y' per row and A^T y^{k+1} per column within bounds the reference DERIVES; the three sums within
theirs, against the vectors and against the downloaded partials; the restart's distances within theirs and its weight within the
bound its docstring states.  The scenario is tests/halpern_step_scenario.py; tests/test_halpern_step_reference.py runs the same one
on a float64 stand-in and asserts the properties it needs of these LPs.

Further cases: the same ids with their long rows turned into equality rows, so that the sums of those rows are SEEN (a free or
inactive row hides its sum behind y' = 0); the run of seven steps (graphs of 4 + 2 + 1, x' stored by the last step only) against seven
single steps and against plain launches, bit for bit; the panel walkers' tail shapes of tests/test_panel_epilogue_tail_gpu.py, where apply() and row() of one
epilogue meet in a lane of seven rows; the scalar branches (a fixed point of T; an overflow of r2) in each of the four layouts; and the
zero-skip bitmap, which the mode must never touch.

Nothing is compared with another layout or with the restatement that runs alongside in tests/test_halpern_gpu.py: a failure names
the id, the step, the stage and the element."""
import numpy as np
import pytest

import attempt_reference as ar
import attempt_scenario as asc
import halpern_reference as H
import halpern_step_reference as hr
import halpern_step_scenario as sc
from cuopt_amd import capi
from eval_lps import DENSE_ROWS, LONG_ROWS
from test_eval_layouts_gpu import VARIANTS, open_variant, variant_lp
from test_halpern_step_reference import overflow_lp
from test_panel_epilogue_tail_gpu import CHUNK, DEPTH, MAX_ROWS, OWN_ROW, SLAB_BYTES, THREADS, lp as tail_lp, open_panels, panel_cut

pytestmark = pytest.mark.gpu
M_SIZED = ("Y", "Y_OTHER", "SUM_Y", "AVG_Y", "LO", "HI", "DROW", "LAST_RESTART_Y")
MOST_PARTIALS = 1 << 16
LAYOUTS = ("stream", "panel", "jag", "pb")
SPLIT_IDS = ("stream", "panel-rows-4KiB", "panel-longtail", "jag-16", "pb")
COMPARED = ("X", "Y", "ATY", "AVG_X", "AVG_Y")


@pytest.fixture(autouse=True)
def multi_launch_kernels(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")  # these LPs are small: keep them off the resident one-workgroup path


class OnDevice:
    """halpern_step_scenario's interface over a capi.Device in Halpern mode"""

    def __init__(self, dev):
        self.dev = dev

    def ctl(self):
        return ar.ctl_dict(self.dev.ctl())

    def hal(self):
        return self.dev.halpern()  # (as the last ctl() / run() / restart read it back)

    def get(self, name):
        d = self.dev
        count = d.nnz if name in ("A_VALUES", "AT_VALUES") else MOST_PARTIALS if name.startswith("PART_") else d.m if name in M_SIZED else d.n
        out = d.download(name, count)
        assert len(out) < MOST_PARTIALS or not name.startswith("PART_"), "more partials than the test downloads"
        return out

    def put(self, name, a):
        self.dev.upload(name, a)

    def run(self, target):
        return self.dev.run(target)

    def halpern_restart(self, theta):
        return self.dev.halpern_restart(theta)[:2]


def prepared(raw, p, x0, y0, scale=True, graph=1, resident=False):
    """Ruiz 10 + Pock-Chambolle (or the identity), Halpern mode, eta = STEP_SAFETY / sigma_max, omega from the norms of c and b (as
    test_halpern_gpu.halpern_device), the start scaled and projected, A^T y, the start its own anchor
    -> (OnDevice, Structure, the scaled problem as the device holds it; resident: with AT_VALUES, for
    tests/test_halpern_resident_steps_gpu.py)"""
    raw.call("set_graph_mode", int(graph))
    if scale:
        raw.call("scaling_compute", 1, 10, 1, 1.0)
    else:
        raw.call("scaling_compute", 0, 0, 0, 1.0)
    raw.call("scale_problem")
    raw.set_halpern(True)
    sigma, products = raw.spectral_norm()
    assert sigma > 0.0 and 1 <= products <= 5000
    nr = raw.init_norms()
    omega = np.sqrt(nr[1]) / np.sqrt(nr[2]) if nr[1] > 0 and nr[2] > 0 else 1.0
    raw.call("set_step", H.STEP_SAFETY / sigma, omega)
    raw.call("set_initial", capi._ptr(np.ascontiguousarray(x0)), capi._ptr(np.ascontiguousarray(y0)))
    raw.call("project_primal")
    raw.call("compute_aty")
    raw.halpern_restart(-1.0)
    dev = OnDevice(raw)
    c = dev.ctl()
    assert (c["cur"], c["pending_avg"], c["steps_taken"], c["attempts"], c["error"]) == (0, 0, 0, 0, 0), c
    assert c["step_size"] == H.STEP_SAFETY / sigma and c["tau"] == c["step_size"] / c["primal_weight"] and c["sigma"] == c["step_size"] * c["primal_weight"], c
    if not scale:
        assert (dev.get("DROW") == 1.0).all() and (dev.get("DCOL") == 1.0).all(), "the identity scaling"
    S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
    return dev, S, sc.download_problem(dev, resident)


def scenario(name, raw, p, x0, y0):
    dev, S, prob = prepared(raw, p, x0, y0)
    before = raw.loop_stats()
    worst = sc.run_scenario(dev, S, prob, name)
    after = raw.loop_stats()
    assert after["empty_attempts"] == before["empty_attempts"], "a run enqueued a step that found its target reached"
    print(worst.line(name))
    assert max(worst.values()) <= 1.0, worst
    return worst


@pytest.mark.parametrize("name", list(VARIANTS))
def test_steps_against_the_reference(name, monkeypatch):
    p, x0, y0 = variant_lp(name)[:3]
    raw = open_variant(name, p, monkeypatch)
    scenario(name, raw, p, x0, y0)
    raw.close()


def _end_state(dev):
    out = {k: dev.get(k) for k in COMPARED}
    out["ctl"], out["hal"] = dev.ctl(), dev.hal()
    return out


@pytest.mark.parametrize("name", SPLIT_IDS)
def test_a_run_is_the_composition_of_its_steps(name, monkeypatch):
    """behind three single steps, run(+7) -- graphs of 4 + 2 + 1, of which only the last step stores x' -- leaves X, Y, A^T y, T(z^k)
    and both blocks bit for bit what seven single steps leave; for two ids also as plain launches"""
    p, x0, y0 = variant_lp(name)[:3]
    ends = []
    for how in ("one run", "single steps") + (("plain launches",) if name in ("stream", "panel-longtail") else ()):
        raw = open_variant(name, p, monkeypatch)
        dev = prepared(raw, p, x0, y0, graph=0 if how == "plain launches" else 1)[0]
        for target in (1, 2, 3):
            dev.run(target)
        for target in (range(4, 4 + sc.RUN_STEPS) if how == "single steps" else (3 + sc.RUN_STEPS,)):
            c = dev.run(target)
            assert (c.steps_taken, c.attempts, c.error) == (target, target, 0)
        ends.append(_end_state(dev))
        raw.close()
    assert ends[0]["hal"]["k"] == 3 + sc.RUN_STEPS and ends[0]["hal"]["r2_min"] > 0.0, ends[0]["hal"]
    for other, how in zip(ends[1:], ("single steps", "plain launches")):
        assert ends[0]["ctl"] == other["ctl"], (name, how, ends[0]["ctl"], other["ctl"])
        assert ends[0]["hal"] == other["hal"], (name, how, ends[0]["hal"], other["hal"])
        for k in COMPARED:
            assert ar.bits_equal(ends[0][k], other[k]), (name, how, k, int(np.argmax(ends[0][k] != other[k])))


def steps_and_a_restart(raw, p, x0, y0, tag):
    dev, S, prob = prepared(raw, p, x0, y0)
    worst = sc.steps_and_a_restart(dev, S, prob, tag)[0]
    print(worst.line(tag))
    assert max(worst.values()) <= 1.0, (tag, worst)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_long_rows_seen_at_full_weight(name, monkeypatch):
    """the same 13 ids on their LPs with the long and the dense rows turned into EQUALITY rows (the same matrix, so the same layout
    and geometry: open_variant asserts them).  On the LPs as they stand most of those rows are free or inactive, where y' is 0
    whatever their sum was (halpern_step_scenario.rows_as_equalities has the figures); here a wrong sum of the cooperative path, of a
    row with a workgroup of its own, of a row over many slabs or of a dense segment moves y' by sigma times the error."""
    p, x0, y0 = variant_lp(name)[:3]
    q = sc.rows_as_equalities(p, tuple(LONG_ROWS) + (tuple(DENSE_ROWS) if VARIANTS[name][3] else ()))
    raw = open_variant(name, q, monkeypatch)
    steps_and_a_restart(raw, q, x0, y0, name + " long rows as equalities")
    raw.close()


@pytest.mark.parametrize("seg", [0, 1], ids=["rows-per-lane", "by-nonzero"])
def test_tail_shapes(seg, monkeypatch):
    """test_panel_epilogue_tail_gpu's `shapes` LP and its assertions on the cut: fewer rows than lanes, a full and a one-row last
    slot, one chunk, a row with a workgroup of its own, seven rows per lane (apply() for four, row() for three), an empty panel"""
    p, x0, y0, first = tail_lp("shapes")
    lens = np.diff(p["offsets"])
    row0, own = panel_cut(lens, 2048)
    assert list(row0) == list(first), (row0, first)
    rows = np.diff(row0)
    assert rows[0] < THREADS
    assert rows[1] % THREADS == 0 and rows[2] % THREADS == 1 and rows[1] // THREADS == rows[2] // THREADS == 2
    assert rows[5] == MAX_ROWS > DEPTH * THREADS and lens[row0[5]:row0[6]].sum() < 2048 and set(lens[row0[5]:row0[6]]) == {0, 1}
    assert lens[row0[6]:row0[7]].sum() == 0 and row0[7] == p["m"]
    assert list(own) == [row0[4] + 200] and own[0] - row0[4] < DEPTH * THREADS and lens[own[0]] > OWN_ROW
    raw, lay = open_panels(p, seg, monkeypatch, 2048, SLAB_BYTES)
    slab_w = -(-p["n"] // lay["A"]["slabs"])
    assert lay["A"]["slabs"] == 12 and lay["A"]["workgroups"] == len(rows) + len(own), (lay, len(rows), len(own))
    in3 = p["indices"][p["offsets"][row0[3]]:p["offsets"][row0[4]]]
    assert in3.max() < slab_w and len(in3) <= CHUNK, "panel 3 is one chunk of one tile"
    S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
    t_row0, t_own = panel_cut(S.len_c, 2048)
    assert len(t_own) == 0 and lay["At"]["workgroups"] == len(t_row0) - 1, (lay, len(t_row0) - 1)
    steps_and_a_restart(raw, p, x0, y0, "shapes seg=%d" % seg)
    raw.close()


@pytest.mark.parametrize("seg", [0, 1], ids=["rows-per-lane", "by-nonzero"])
def test_tail_several_chunks_in_a_tile(seg, monkeypatch):
    p, x0, y0 = tail_lp("chunks")
    lens = np.diff(p["offsets"])
    row0, own = panel_cut(lens, 6000)
    per_panel = np.diff(p["offsets"][row0])
    assert len(own) == 0 and per_panel.max() > CHUNK and (per_panel[:-1] % CHUNK != 0).all() and per_panel.max() < 2 * CHUNK, per_panel
    raw, lay = open_panels(p, seg, monkeypatch, 6000, 1 << 20)
    assert lay["A"]["slabs"] == 1 and lay["A"]["workgroups"] == len(row0) - 1, (lay, len(row0) - 1)  # one tile per panel: two chunks
    steps_and_a_restart(raw, p, x0, y0, "chunks seg=%d" % seg)
    raw.close()


def open_tiny(p, layout, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    raw = capi.Device(p)
    lay = raw.layout()
    assert not lay["resident"] and lay["A"]["layout"] == lay["At"]["layout"] == layout, lay
    return raw


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_fixed_point_of_the_operator(layout, monkeypatch):
    """attempt_scenario.tiny_lp("fixed-point") is a fixed point of T under any tau and sigma (tests/test_halpern_step_reference.py says
    why): r2 = r = r_first = r2_min = 0 and no error; the first step (w = w0 = 1/2) keeps every bit of the iterate"""
    p, x0, y0 = asc.tiny_lp("fixed-point")
    raw = open_tiny(p, layout, monkeypatch)
    dev, S, prob = prepared(raw, p, x0, y0, scale=False)
    start = sc.snapshot(dev)
    for i in range(2):
        r, before, after = sc.one_step(dev, S, prob, "fixed point %s %d" % (layout, i))
        assert (r["r2"], r["dx2"], r["dy2"], r["inter"], r["error"]) == (0.0, 0.0, 0.0, 0.0, 0), r
        assert (after["hal"]["r"], after["hal"]["r_first"], after["hal"]["r2"], after["hal"]["r2_min"]) == (0.0, 0.0, 0.0, 0.0), after["hal"]
        assert after["ctl"]["error"] == 0
        if i == 0:
            assert all(ar.bits_equal(after[k], start[k]) for k in ("X", "Y", "ATY")), "the fixed point moved"
    raw.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_an_overflow_raises_the_step_error(layout, monkeypatch):
    """Y with 1e200 on a "<=" row: y' = 0 there, dy^2 overflows, r2 = inf >= 1e100 raises `error`; hal keeps every field, the control
    block's counters are as halpern_decision.hpp writes them, and the next run enqueues nothing
    (docs/design/04d_halpern_mode.md: "a NaN or r2 >= 1e100 raises error")"""
    p, x0, y0 = overflow_lp()
    raw = open_tiny(p, layout, monkeypatch)
    dev, S, prob = prepared(raw, p, x0, y0, scale=False)
    assert prob["LO"][0] == -np.inf and np.isfinite(prob["HI"][0])
    y = dev.get("Y")
    y[0] = 1e200
    dev.put("Y", y)
    before = sc.snapshot(dev)
    assert before["Y"][0] == 1e200
    c = dev.run(1)
    after = sc.snapshot(dev, hr.AFTER)
    assert hr.check_decision(before, after, "overflow " + layout)["error"] == 1
    assert after["ctl"]["last_dy2"] == np.inf and after["ctl"]["last_movement"] == np.inf and after["AVG_Y"][0] == 0.0, after["ctl"]
    assert after["hal"] == before["hal"], (before["hal"], after["hal"])
    assert (c.error, c.attempts, c.steps_taken, c.k, c.cur, c.its_since_restart) == (1, 1, 1, 1, 1, 1)
    c = dev.run(2)
    assert (c.error, c.attempts, c.steps_taken) == (1, 1, 1) and dev.hal() == before["hal"]
    raw.close()


def test_zero_skip_is_out_of_the_modes_way(monkeypatch):
    """zero_skip=2 builds the bitmap of xbar and would mask every A product of an averaging attempt; the Halpern products never read
    it: the same scenario passes and the masked-launch counter stays 0"""
    name = "panel-rows-4KiB"
    p, x0, y0 = variant_lp(name)[:3]
    raw = open_variant(name, p, monkeypatch, zero_skip=2)
    assert int(raw.download("ZS_LAUNCHES", 1).view(np.uint64)[0]) == 0
    scenario(name + " zero_skip=2", raw, p, x0, y0)
    assert int(raw.download("ZS_LAUNCHES", 1).view(np.uint64)[0]) == 0 and raw.ctl().attempts > 0
    raw.close()
