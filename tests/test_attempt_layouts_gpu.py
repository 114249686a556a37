"""GPU: the adaptive PDHG attempt in EVERY SpMV layout against the stage-by-stage reference (tests/attempt_reference.py).

k_primal, the A product with DualEpilogue, the A^T product with StepEpilogue and k_step_decision of the stream, panel (rows per lane
and long-tail), jagged (8 and 16 waves) and gather-free (both geometries) layouts, with and without the dense-segment prologue -- the
13 ids of tests/test_eval_layouts_gpu.py, on its LPs -- one attempt at a time through pdlpdev_debug_attempts, so that a REJECTED
attempt is there to be looked at.  Every attempt is checked against the state the device held in front of it: x', xbar, the running
sums, movement, the decision, the counters, tau / sigma and the weight sum bit for bit; y' per row and A^T y' per column within bounds
the reference DERIVES; the three reductions within theirs; the new step at rel 1e-14 (pow).  Then k_flush_average, k_make_average and
restart_block with the squared distances pdlpdev_restart returns.  The scenario is tests/attempt_scenario.py; tests/
test_attempt_reference.py runs the same one on a float64 stand-in and asserts the properties it needs of these LPs.

The forced rejection is NOT set_step(64 step, w) alone: no step and weight reject a consistent state with step / limit >= 2 (it
tends to 1 as the step grows; attempt_scenario.force_rejection has the figures).  Behind that call the dual iterate is moved off its
A^T y through the upload hook, by an amount the reference sizes for step / limit = 4; the assertions are the ones that were asked for.

Nothing is compared with another layout or with the oracle: a failure names the id, the attempt, the stage and the element."""
import ctypes as C

import numpy as np
import pytest

import attempt_reference as ar
import attempt_scenario as sc
from cuopt_amd import capi
from oracle import orcbind
from test_eval_layouts_gpu import VARIANTS, open_variant, variant_lp

pytestmark = pytest.mark.gpu
M_SIZED = ("Y", "Y_OTHER", "SUM_Y", "AVG_Y", "LO", "HI", "DROW", "LAST_RESTART_Y")


@pytest.fixture(autouse=True)
def multi_launch_kernels(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")  # these LPs are small: keep them off the resident one-workgroup path


def step_params(mode=1):
    h, H = orcbind.hyper_preset(mode), orcbind.H
    return {k: float(h[H["ORC_H_" + k.upper()]]) for k in ("reduction_exponent", "growth_exponent", "primal_distance_smoothing", "dual_distance_smoothing")}


class OnDevice:
    """attempt_scenario's interface over a capi.Device"""

    def __init__(self, dev, sp):
        self.dev, self.sp = dev, sp
        dev.call("set_step_params", C.byref(capi.StepParams(**sp)))

    def ctl(self):
        return ar.ctl_dict(self.dev.ctl())

    def get(self, name):
        d = self.dev
        return d.download(name, d.nnz if name == "A_VALUES" else d.m if name in M_SIZED else d.n)

    def put(self, name, a):
        self.dev.upload(name, a)

    def attempt(self):
        return self.dev.attempts(1)

    def flush(self):
        self.dev.call("flush_average")

    def make_average(self, mode):
        self.dev.call("make_average", int(mode))

    def restart(self, which, unscaled):
        dist = np.zeros(2)
        self.dev.call("restart", int(which), int(unscaled), capi._ptr(dist))
        return dist

    def set_step(self, step, weight):
        self.dev.call("set_step", float(step), float(weight))

    def compute_aty(self):
        self.dev.call("compute_aty")


def prepared(raw, p, x0, y0, scale=True, graph=1):
    """step 1: Ruiz 10 + Pock-Chambolle, the scaled problem, the start scaled and projected, the step 1 / max|A| at weight 1, A^T y
    -> (OnDevice, Structure, the scaled problem as the device holds it, D_r, D_c)"""
    raw.call("set_graph_mode", int(graph))
    dev = OnDevice(raw, step_params(1))
    if scale:
        raw.call("scaling_compute", 1, 10, 1, 1.0)
        raw.call("scale_problem")
    raw.call("set_initial", capi._ptr(np.ascontiguousarray(x0)), capi._ptr(np.ascontiguousarray(y0)))
    raw.call("project_primal")
    raw.call("set_step", 1.0 / raw.init_norms()[0], 1.0)
    raw.call("compute_aty")
    c = dev.ctl()
    assert (c["cur"], c["pending_avg"], c["steps_taken"], c["attempts"], c["error"]) == (0, 0, 0, 0, 0) and c["sigma"] == c["step_size"], c
    S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
    return dev, S, sc.download_problem(dev), dev.get("DROW"), dev.get("DCOL")


@pytest.mark.parametrize("name", list(VARIANTS))
def test_attempts_against_the_reference(name, monkeypatch):
    p, x0, y0 = variant_lp(name)[:3]
    raw = open_variant(name, p, monkeypatch)
    dev, S, prob, dr, dc = prepared(raw, p, x0, y0)
    before = raw.loop_stats()
    worst = sc.run_scenario(dev, S, prob, dev.sp, dr, dc, name)
    after = raw.loop_stats()
    assert after["empty_attempts"] == before["empty_attempts"], "the hook enqueued an attempt that found its target reached"
    raw.close()
    print(worst.line(name))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("which", ["both", "lb-only", "ub-only"])
def test_uniform_bounds_fast_path(which, monkeypatch):
    """k_primal takes a uniform lower / upper bound (all 0, all +inf) as a constant instead of reading the array"""
    p, x0, y0 = variant_lp("stream")[:3]
    q = sc.uniform_bounds_variants(p)[which]
    raw = open_variant("stream", q, monkeypatch)
    dev, S, prob, dr, dc = prepared(raw, q, x0, y0)
    worst = sc.Worst()
    for i in range(3):  # (x' and xbar bit for bit, and everything else of an attempt)
        sc.assert_decided(sc.one_attempt(dev, S, prob, dev.sp, "uniform %s attempt %d" % (which, i), worst)[0], which)
    raw.close()
    print(worst.line("uniform-" + which))


@pytest.mark.parametrize("name", ["stream", "panel-longtail"])
def test_plain_launches_equal_graph_replay(name, monkeypatch):
    """the same eight attempts as plain launches: every buffer and the control block bit for bit what the replayed graphs leave"""
    p, x0, y0 = variant_lp(name)[:3]
    records = []
    for graph in (1, 0):
        raw = open_variant(name, p, monkeypatch)
        dev, S, prob, dr, dc = prepared(raw, p, x0, y0, graph=graph)
        records.append([])
        sc.natural_attempts(dev, S, prob, dev.sp, "%s graph=%d" % (name, graph), sc.Worst(), records[-1])
        raw.close()
    for i, (g, plain) in enumerate(zip(*records)):
        assert g["ctl"] == plain["ctl"], (name, i, g["ctl"], plain["ctl"])
        for k in ar.STATE + ("XBAR",):
            assert ar.bits_equal(g[k], plain[k]), (name, i, k)


@pytest.mark.parametrize("layout", ["stream", "panel", "jag", "pb"])
@pytest.mark.parametrize("kind", ["fixed-point", "dual-only"])
def test_scalar_branches(kind, layout, monkeypatch):
    """a fixed point (movement 0: the step error, k and the step untouched, the buffers flip, the weight sum grows by the step) and
    dx = 0 with dy != 0 (interaction 0: accepted, the step grows by its full factor), on a 40 x 60 LP forced into each layout"""
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    p, x0, y0 = sc.tiny_lp(kind)
    raw = capi.Device(p)
    lay = raw.layout()
    assert not lay["resident"] and lay["A"]["layout"] == lay["At"]["layout"] == layout, lay
    dev, S, prob, dr, dc = prepared(raw, p, x0, y0, scale=False)
    r, before, after = sc.one_attempt(dev, S, prob, dev.sp, "%s %s" % (kind, layout))
    sc.assert_scalar_branch(kind, r, before, after, dev.sp)
    if kind == "fixed-point":  # (with the error up the next call enqueues nothing and says so)
        c = dev.attempt()
        assert (c.error, c.attempts, c.steps_taken) == (1, 1, 1)
    raw.close()


def test_hook_is_refused_where_no_multi_launch_attempt_runs(monkeypatch):
    """-7 in Halpern mode, on the resident small-LP path (whose averaging loop the hook does serve: tests/test_resident_attempts_gpu.py)
    and off it; -1 for a count outside 1 .. 64 on a resident context.  A context behind a communicator is NOT refused any more (the
    sharded attempt is what tests/test_sharded_attempts_gpu.py looks at through the hook): one rank behind one serves an attempt, and
    refuses the same counts."""
    p, x0, y0 = sc.tiny_lp("dual-only")
    monkeypatch.setenv("CUOPT_AMD_SMALL", "1")
    raw = capi.Device(p)
    assert raw.layout()["resident"]
    for count in (0, 65):
        with pytest.raises(capi.CuOptError) as e:
            raw.attempts(count)
        assert e.value.code == -1
    raw.call("scaling_compute", 1, 10, 1, 1.0)
    raw.call("scale_problem")
    raw.set_halpern(True)
    with pytest.raises(capi.CuOptError) as e:
        raw.attempts(1)
    assert e.value.code == -7
    raw.close()
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")
    raw = capi.Device(p)
    raw.call("scaling_compute", 1, 10, 1, 1.0)
    raw.call("scale_problem")
    raw.set_halpern(True)
    with pytest.raises(capi.CuOptError) as e:
        raw.attempts(1)
    assert e.value.code == -7
    raw.close()
    solver = capi.Solver(p, rank=0, world=1, comm_id=capi.softcomm_id(1))
    assert capi.lib.pdlpdev_shard_dataflow(solver.device.handle) == 3
    for count in (0, 65):
        with pytest.raises(capi.CuOptError) as e:
            solver.device.attempts(count)
        assert e.value.code == -1
    c = solver.device.attempts(1)
    assert (c.error, c.attempts, c.target_steps) == (0, 1, 1)
    solver.close()
