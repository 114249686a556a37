"""GPU: a chunk of N attempts that decides each step at the head of the NEXT attempt's primal kernel (CUOPT_AMD_TUNE=primal_decides,
enqueue_single_chunk: primal, a_dual, at_step | primal_decide, a_dual, at_step | ... | decision) against the one-at-a-time sequence.

pdlpdev_debug_attempts(1) is a chunk of one -- the four launches tests/test_attempt_layouts_gpu.py pins stage by stage -- and the
reference here: attempts(N) must leave, BIT FOR BIT, what N calls of attempts(1) leave from the same state: the whole control block
(counters, tau, sigma, the weight sum, cur, pending_avg, the zero-skip flag and count) and both sides of x, y and A^T y, xbar and the
two running sums.  On the LPs and ids of tests/test_eval_layouts_gpu.py (n = 6000: two workgroups of the fused kernel, the second one
ending inside a wave; bounds from the arrays), with graph replay and with plain launches.

Chunk sizes: a context takes chunks of 2, 3, 5, 8 and 64 attempts one behind the other while the reference context takes as many
single attempts; the states are compared behind every chunk, so every chunk starts from a state the two share.  With graphs a chunk of
3 is a graph of 2 and a graph of 1, one of 5 a graph of 4 and a graph of 1; with plain launches it is one chunk."""
import numpy as np
import pytest

import attempt_reference as ar
import attempt_scenario as sc
from cuopt_amd import capi, synthetic
from conftest import set_tune
from test_attempt_layouts_gpu import prepared
from test_eval_layouts_gpu import open_variant, variant_lp

pytestmark = pytest.mark.gpu
BUFFERS = ar.STATE + ("XBAR",)  # X, Y, ATY and their other sides, SUM_X, SUM_Y, XBAR
CHUNKS = (2, 3, 5, 8, 64)
# id -> (id of test_eval_layouts_gpu.VARIANTS, further CUOPT_AMD_TUNE keys)
CASES = {
    "stream": ("stream", dict()),
    "panel-rows": ("panel-rows-4KiB", dict()),  # the zero-skip guard as it is by default: the flag decides
    "panel-rows-zs-forced": ("panel-rows-4KiB", dict(zero_skip=2)),
    "panel-longtail": ("panel-longtail", dict()),  # (panels that sum by nonzero: no bitmap, the plain decision)
    "jag-8": ("jag-8", dict()),
    "pb": ("pb", dict()),
    "dense-stream": ("dense-stream", dict()),  # (the dense prologue reads the control block too)
    "dense-pb": ("dense-pb", dict()),
}


@pytest.fixture(autouse=True)
def multi_launch_kernels(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")  # these LPs are small: keep them off the resident one-workgroup path


def state(dev):
    """every buffer an attempt writes and the control block's bytes -- without target_steps, which no kernel of an attempt writes: the
    hook sets it to steps_taken + count in front of its attempts, so behind a chunk with a rejection in it the host has left another
    value there than in front of the last of as many single attempts"""
    out = {k: dev.get(k) for k in BUFFERS}
    c = dev.dev.ctl()
    c.target_steps = 0
    out["ctl"] = bytes(c)
    return out


def assert_same(got, want, tag):
    if got["ctl"] != want["ctl"]:
        c = lambda b: ar.ctl_dict(capi.Ctl.from_buffer_copy(b))  # noqa: E731
        raise AssertionError((tag, "control block", c(got["ctl"]), c(want["ctl"])))
    for k in BUFFERS:
        assert ar.bits_equal(got[k], want[k]), (tag, k, int(np.sum(got[k].view(np.int64) != want[k].view(np.int64))), "elements differ")


_references = {}


def reference_states(case, monkeypatch):
    """the states behind 2, 2 + 3, ... single attempts of `case`, computed once and shared (read-only) by its tests"""
    if case not in _references:
        name, tune = CASES[case]
        p, x0, y0 = variant_lp(name)[:3]
        raw = open_variant(name, p, monkeypatch, **tune)
        dev = prepared(raw, p, x0, y0)[0]
        states = []
        for n in CHUNKS:
            for _ in range(n):
                dev.attempt()
            states.append(state(dev))
        c = raw.ctl()
        raw.close()
        assert c.attempts == sum(CHUNKS) and c.error == 0 and 0 < c.steps_taken, "the reference made its attempts"
        for s in states:
            for a in s.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _references[case] = (states, c.attempts - c.steps_taken)
    return _references[case]


@pytest.mark.parametrize("graph", [1, 0], ids=["graphs", "plain-launches"])
@pytest.mark.parametrize("case", list(CASES))
def test_chunks_equal_single_attempts(case, graph, monkeypatch):
    name, tune = CASES[case]
    want, rejected = reference_states(case, monkeypatch)
    p, x0, y0 = variant_lp(name)[:3]
    raw = open_variant(name, p, monkeypatch, primal_decides=1, **tune)
    dev = prepared(raw, p, x0, y0, graph=graph)[0]
    for n, ref in zip(CHUNKS, want):
        raw.attempts(n)
        assert_same(state(dev), ref, "%s graph=%d chunk of %d" % (case, graph, n))
    print("CHUNKS %s graph=%d: %d attempts, %d of them rejected" % (case, graph, sum(CHUNKS), rejected))
    raw.close()


def test_the_key_switched_off_is_the_same_too(monkeypatch):
    """primal_decides=0 (the decision kernel behind every attempt of a chunk, what A/B runs compare with)"""
    name, tune = CASES["panel-rows"]
    want = reference_states("panel-rows", monkeypatch)[0]
    p, x0, y0 = variant_lp(name)[:3]
    raw = open_variant(name, p, monkeypatch, primal_decides=0, **tune)
    dev = prepared(raw, p, x0, y0)[0]
    for n, ref in zip(CHUNKS, want):
        raw.attempts(n)
        assert_same(state(dev), ref, "primal_decides=0 chunk of %d" % n)
    raw.close()


@pytest.mark.parametrize("case", ["stream", "panel-rows"])
def test_grid_stride_remainder(case, monkeypatch):
    """an LP of more columns than the fused kernel's grid holds in its first pass (n > 512 workgroups x 4096 columns in real use): with
    the grid capped at ONE workgroup (CUOPT_AMD_TUNE=primal_decide_grid=1) columns 4096 .. 5999 go through the remainder loop, the
    last wave of it partly beyond n"""
    name, tune = CASES[case]
    want = reference_states(case, monkeypatch)[0]
    p, x0, y0 = variant_lp(name)[:3]
    raw = open_variant(name, p, monkeypatch, primal_decides=1, primal_decide_grid=1, **tune)
    dev = prepared(raw, p, x0, y0)[0]
    for n, ref in zip(CHUNKS, want):
        raw.attempts(n)
        assert_same(state(dev), ref, "%s one workgroup, chunk of %d" % (case, n))
    raw.close()


@pytest.mark.parametrize("graph", [1, 0], ids=["graphs", "plain-launches"])
@pytest.mark.parametrize("case", ["stream", "panel-rows", "panel-rows-zs-forced"])
def test_rejection_inside_a_chunk(case, graph, monkeypatch):
    """attempt_scenario.force_rejection in front of a chunk of 4: the chunk's first attempt is rejected, so the fused kernel of attempt
    2 decides "rejected", loads x and A^T y again from the side that did not flip, and the attempts behind it run"""
    name, tune = CASES[case]
    p, x0, y0 = variant_lp(name)[:3]
    states = []
    for chunked in (False, True):
        raw = open_variant(name, p, monkeypatch, primal_decides=1, **tune)
        dev, S, prob, dr, dc = prepared(raw, p, x0, y0, graph=graph)
        for _ in range(sc.NATURAL_ATTEMPTS):
            dev.attempt()
        held = sc.check_flush(dev, case + " flush")
        sc.force_rejection(dev, S, prob, dev.sp, held, case, recoverable=True)  # (a displacement the attempts get past by themselves)
        before = raw.ctl()
        if chunked:
            raw.attempts(4)
        else:
            for _ in range(4):
                dev.attempt()
        after = raw.ctl()
        states.append(state(dev))
        raw.close()
        print("REJECTION %s graph=%d chunked=%d: %d attempts, %d steps" % (case, graph, chunked, after.attempts - before.attempts, after.steps_taken - before.steps_taken))
        assert after.error == 0 and after.attempts - before.attempts == 4, "the attempts behind the rejection ran"
        assert after.steps_taken - before.steps_taken < 4, "no rejection inside the chunk"
    assert_same(states[1], states[0], "%s graph=%d rejection inside a chunk of 4" % (case, graph))


def _edge_lp(n, bounds, seed=17):
    rng = np.random.default_rng(seed + n)
    p = synthetic.generate(n, n, 4, seed=seed)
    p = {k: p[k] for k in ("m", "n", "offsets", "indices", "values", "c", "lo", "hi", "lb", "ub")}
    if bounds == "arrays":  # (k_primal and its twin read lb / ub per column)
        p["lb"] = np.where(rng.random(n) < 0.5, 0.0, -1.0)
        p["ub"] = 1.0 + 4.0 * rng.random(n)
    else:
        assert (p["lb"] == 0.0).all() and np.isinf(p["ub"]).all(), "synthetic.generate: x >= 0"
    return p, np.abs(rng.standard_normal(n)), rng.standard_normal(n)


@pytest.mark.parametrize("bounds", ["uniform", "arrays"])
@pytest.mark.parametrize("n", [700, 1025, 4097])
def test_edges_of_the_element_loop(n, bounds, monkeypatch):
    """n below one workgroup of the fused kernel (1024 threads, 4 columns each) and no multiple of 64; one above the workgroup's
    threads; one above its columns (a second workgroup with a single column); uniform bounds (constants) and the array path"""
    p, x0, y0 = _edge_lp(n, bounds)
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    states = []
    for chunk in (1, 8):
        set_tune(monkeypatch, primal_decides=1)
        raw = capi.Device(p)
        lay = raw.layout()
        assert not lay["resident"] and lay["A"]["layout"] == "stream", lay
        dev = prepared(raw, p, x0, y0)[0]
        for _ in range(8 // chunk):
            raw.attempts(chunk)
        c = raw.ctl()
        assert c.attempts == 8 and c.error == 0 and c.steps_taken >= 1, (c.attempts, c.error, c.steps_taken)
        states.append(state(dev))
        raw.close()
    assert_same(states[1], states[0], "n=%d %s bounds" % (n, bounds))


SOLVE_KEYS = ("status", "steps_taken", "attempted_steps", "returned_average", "num_restarts", "num_major_iterations", "primal_objective", "dual_objective", "gap",
              "relative_gap", "l2_primal_residual", "l2_dual_residual", "l2_relative_primal_residual", "l2_relative_dual_residual", "step_size",
              "primal_weight")


BUDGET = 600


def test_target_reached_inside_a_chunk(monkeypatch):
    """a solve of a fixed iteration budget goes through pdlpdev_run_period and its spare attempts: attempts behind the one that reaches
    the target find the loop inactive, the fused kernels copy the block through and the last decision brings the loop's own block up to
    date.  primal_decides=1 against =0: the same solve, bit for bit"""
    p = variant_lp("panel-rows-4KiB")[0]  # (6000 x 6000 with long rows and columns: its attempts are rejected now and then)
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    out = []
    for on in (0, 1):
        set_tune(monkeypatch, primal_decides=on, panel_seg=0, slab_bytes=4096, dense=0)
        s = capi.Solver(p, mode=1, tol=0.0)
        lay = s.device.layout()
        assert not lay["resident"] and lay["A"]["layout"] == lay["At"]["layout"] == "panel", lay
        r = s.advance(BUDGET)
        stats = s.device.loop_stats()
        x, y, z = s.solution()
        out.append((r, x, y, z, stats))
        s.close()
        print("SOLVE primal_decides=%d steps=%d attempts=%d restarts=%d empty_attempts=%d" % (on, r["steps_taken"], r["attempted_steps"], r["num_restarts"],
                                                                                             stats["empty_attempts"]))
        assert r["steps_taken"] == BUDGET and r["attempted_steps"] > BUDGET, "the budget was spent, with rejections on the way"
        assert stats["empty_attempts"] > 0, "no attempt found its target reached: the copy-through case did not run"
    (r0, x0, y0, z0, st0), (r1, x1, y1, z1, st1) = out
    for k in SOLVE_KEYS:
        assert np.array([r0[k]]).tobytes() == np.array([r1[k]]).tobytes(), (k, r0[k], r1[k])
    assert st0["empty_attempts"] == st1["empty_attempts"]
    assert ar.bits_equal(x1, x0) and ar.bits_equal(y1, y0) and ar.bits_equal(z1, z0)
