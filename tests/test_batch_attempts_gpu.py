"""GPU: the shared-matrix lockstep batch's attempt -- kb_primal, kb_a_dual, kb_at_step, the jagged twins kbj_a_dual and kbj_at_step,
k_step_decision_batch, and batch_block_sums / batch_cross_over / batch_block_partials of cuopt_amd/csrc/batch_common.hpp -- stage by
stage against the reference (tests/attempt_reference.py), at the shapes no synthetic matrix reaches.

The LP is tests/batch_cases.edge_lp (7244 x 7200, built from explicit row-length lists; its docstring derives the size), under
CUOPT_AMD_SMALL=0 and CUOPT_AMD_TUNE panel_seg=0, dense=0, panel_nnz=2048, slab_bytes=4096.  Every test first asserts, on the block
boundaries the batch itself reports (pdlpdev_debug_batch_view), that EVERY feature of batch_cases.FEATURES is present on BOTH sides for
its K: blocks of 512 rows with 0 (in the middle and as the matrix's last block, off[r0] == nnz), 1, 2 and 3 chunks; CHUNK, CHUNK + 1 and
2 CHUNK entries; a 128-entry row across a chunk boundary, rows starting and ending on one, an empty row on one; workgroups of 1, fewer
than 64, 512, 513 and 662 rows; empty rows and columns.  n = 7200 leaves kb_primal a tail tile of 32 columns.

Members: the parent (lb = 0, ub = +inf: the uniform-bounds constants; a second parametrisation gives it non-uniform bounds), a clone
with non-uniform bounds, a clone RESET BACK to the uniform ones (its flags must follow, and the batch's table with them), a clone with
row bounds of its own (other infinite sides, other equality rows), further bound variants.  Every member is prepared like
tests/test_attempt_layouts_gpu.py's context and looked at through its own solver.device.

The scenario (batch_cases.run_batch_scenario), ONE lockstep attempt per pdlpdev_debug_batch_attempts call:
  1. eight natural attempts, all members on; per member both cur parities accepted from and both pending_avg states seen;
  2. attempt_scenario.force_rejection on member 1 alone: it is rejected at step / limit >= 2, the others are accepted, in one launch;
  3. the running sums flushed on members 0 and 2 only (K = 2: pending_avg differs by the rejection already), one attempt;
  4. every second member off: all of ar.STATE, the control block and A.part / At.part of a resting member bit for bit untouched, its
     entries of xK exactly +0.0 (one field is let move: a target_steps still beyond steps_taken is taken back to it, which is how the
     hook makes a member rest that an earlier round rejected);
  5. the last member reset -- while the batch lives -- to free rows, with A^T y := c and y = 0 (attempt_scenario.tiny_lp's fixed-point
     kind): the step error for it alone; in the attempt behind it its buffers are frozen and the others go on.
Per attempt and member: everything attempt_reference.check_attempt asserts (x', xbar -- read from xK[j K + l] --, the running sums,
movement, the decision, the counters, tau / sigma and the weight sum bit for bit; the step at STEP_REL; y', A^T y' and the three
reductions within the derived bounds), and on panel and stream sides y', A^T y' and yK[i K + l] BIT FOR BIT against
attempt_reference.rowsums_f64 (left to right, products rounded once: the order kernels_batch.hip's header promises), an empty column's
A^T y' +0.0 by its sign bit on every layout.  On jagged sides y' and A^T y' keep the derived bounds as the pass condition; how their
bits compare with the left-to-right sums is printed (JAGBITS), and batch_cases.jag_features asserts on the reported boundaries that
a pass of fewer than 64 rows, kmax not a multiple of U (where U > 1), rows without nonzeros and several blocks are there.  Two ids
run the attempts as plain launches instead of graph replays.  No tolerance is new: max(worst) <= 1.0.

Then the existing contract at these shapes: advance(130) and advance() of the batch against single solves (test_shared_batch_gpu.same),
the reflected-Halpern lockstep batch after 1, 2, 3, 40 and 130 steps (halpern_lockstep_case.same / state), and kb_plain through
batch.spmv against the parent's own product."""
import contextlib
import functools
import os

import numpy as np
import pytest
from conftest import set_tune

import attempt_reference as ar
import batch_cases as bc
import halpern_lockstep_case as hc
from cuopt_amd import capi
from test_attempt_layouts_gpu import OnDevice, step_params
from test_shared_batch_gpu import same

pytestmark = pytest.mark.gpu
KW = dict(tol=1e-5, iteration_limit=1000)


@pytest.fixture(autouse=True)
def small_blocks(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")
    set_tune(monkeypatch, **bc.TUNE)


@functools.lru_cache(maxsize=None)
def edge():
    p, x0, y0 = bc.edge_lp()
    S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
    return p, x0, y0, S


@functools.lru_cache(maxsize=None)
def banded():
    p, x0, y0 = bc.banded_edge_lp()
    return p, x0, y0, ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])


class MemberOnDevice(OnDevice):
    """attempt_scenario's interface over ONE member's context; attempt() is the batch's hook with this member alone switched on"""

    def __init__(self, solver, p, sp, x0, index):
        raw = solver.device
        raw.m, raw.n, raw.nnz = p["m"], p["n"], len(p["values"])
        super().__init__(raw, sp)
        self.solver, self.x0, self.index, self.batch = solver, np.ascontiguousarray(x0, dtype=np.float64), index, None

    def prepare(self, y0):
        raw = self.dev
        raw.call("set_initial", capi._ptr(self.x0), capi._ptr(np.ascontiguousarray(y0, dtype=np.float64)))
        raw.call("project_primal")
        raw.call("set_step", 1.0 / raw.init_norms()[0], 1.0)
        raw.call("compute_aty")
        c = self.ctl()
        assert (c["cur"], c["pending_avg"], c["steps_taken"], c["attempts"], c["error"]) == (0, 0, 0, 0, 0) and c["sigma"] == c["step_size"], c

    def attempt(self):
        return self.batch.debug_attempts(1, [int(l == self.index) for l in range(len(self.batch.solvers))])[self.index]

    def parts(self):
        return self.dev.download("PART_A", 1 << 14), self.dev.download("PART_AT", 1 << 14)

    def bounds(self):
        return {k: self.get(k) for k in ("LB", "UB", "LO", "HI")}

    def free_rows(self):
        m = self.dev.m
        self.solver.reset(lo=np.full(m, -np.inf), hi=np.full(m, np.inf))
        self.dev.call("set_step_params", capi.C.byref(capi.StepParams(**self.sp)))
        self.prepare(np.zeros(m))
        self.put("ATY", self.get("C"))


def open_batch(p, x0, y0, K, layout, monkeypatch, uniform_parent=True, graph=1, **kw):
    """the K members of batch_cases.members as a parent and its clones, prepared, in one batch -> (batch, solvers, members, problems)"""
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    solvers = make_solvers(p, bc.members(p, K, uniform_parent), **dict(KW, **kw))
    lay = solvers[0].device.layout()
    assert not lay["resident"] and lay["A"]["layout"] == lay["At"]["layout"] == layout, lay
    if layout == "panel":
        assert lay["A"]["row_sums"] == lay["At"]["row_sums"] == "by_row", lay
    batch = capi.SharedMatrixBatch(solvers)
    sp = step_params(1)
    devs = [MemberOnDevice(s, p, sp, x0, l) for l, s in enumerate(solvers)]
    shared = dict(A_VALUES=devs[0].get("A_VALUES"), AT_VALUES=devs[0].dev.download("AT_VALUES", len(p["values"])), C=devs[0].get("C"))
    probs = []
    for d in devs:
        d.batch = batch
        d.dev.call("set_graph_mode", int(graph))  # (the hook replays captured graphs or launches plainly as the parent's context says)
        d.prepare(y0)
        probs.append(dict(shared, **d.bounds()))
    return batch, solvers, devs, probs, sp


def make_solvers(p, ms, **kw):
    lb, ub, lo, hi, _ = ms[0]
    parent = capi.Solver(dict(p, lb=lb, ub=ub, lo=lo, hi=hi), **kw)
    solvers = [parent]
    for lb, ub, lo, hi, how in ms[1:]:
        rows = {} if lo is p["lo"] else dict(lo=lo, hi=hi)
        if how == "reset-back":  # (created with member 1's non-uniform bounds, then reset to these)
            s = parent.clone(lb=ms[1][0], ub=ms[1][1])
            s.reset(lb=lb, ub=ub, **rows)
        else:
            s = parent.clone(lb=lb, ub=ub, **rows)
        solvers.append(s)
    return solvers


def close_all(batch, solvers):
    if batch is not None:
        batch.close()
    for s in solvers[1:]:
        s.close()
    solvers[0].close()


@contextlib.contextmanager
def batch_of(p, ms, **kw):
    """(batch, solvers) of the members ms, closed on every way out"""
    solvers, batch = make_solvers(p, ms, **kw), None
    try:
        batch = capi.SharedMatrixBatch(solvers)
        yield batch, solvers
    finally:
        close_all(batch, solvers)


def assert_features(batch, S, K, layout, p):
    sides = ((S.off, S.idx, p["n"]), (S.t_off, S.t_rows, p["m"]))
    cuts = bc.stream_cuts if layout == "stream" else bc.panel_cuts
    for side, (off, idx, ncols) in enumerate(sides):
        v = batch.view(side)
        assert (v["K"], v["layout"], v["rows"]) == (K, layout, len(off) - 1) and v["row0"][0] == 0 and v["row0"][-1] == len(off) - 1, v
        if not np.array_equal(v["row0"], cuts(off)):
            print("CUTS %s side %d: the batch's boundaries are not batch_cases' restatement of the rule" % (layout, side))
        missing = set(bc.FEATURES) - bc.features(off, v["row0"], K, idx, ncols)
        assert not missing, (layout, K, "side %d" % side, sorted(missing))


# (K, layout, uniform parent, graph mode): the last two make the attempts as plain launches (batch_enqueue) instead of graph replays
CASES = ([(K, layout, True, 1) for K in (2, 4, 8, 16) for layout in ("stream", "panel")] + [(4, "stream", False, 1), (4, "panel", False, 1)] +
         [(4, "stream", True, 0), (16, "panel", True, 0)])


def case_id(K, layout, uniform_parent, graph):
    return "K%d-%s-%s%s" % (K, layout, "uniform" if uniform_parent else "nonuniform-parent", "" if graph else "-plain-launches")


@pytest.mark.parametrize("K,layout,uniform_parent,graph", CASES, ids=[case_id(*c) for c in CASES])
def test_batch_attempts_against_the_reference(K, layout, uniform_parent, graph, monkeypatch):
    p, x0, y0, S = edge()
    batch, solvers, devs, probs, sp = open_batch(p, x0, y0, K, layout, monkeypatch, uniform_parent, graph)
    name = case_id(K, layout, uniform_parent, graph)
    try:
        assert_features(batch, S, K, layout, p)
        worst = bc.run_batch_scenario(batch, devs, S, probs, sp, name, refresh=lambda l: dict(probs[l], **devs[l].bounds()))
    finally:
        close_all(batch, solvers)
    print(worst.line(name))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("waves", [8, 16])
@pytest.mark.parametrize("K", [2, 16])
def test_jagged_batch_attempts_against_the_reference(K, waves, monkeypatch):
    """kbj_a_dual / kbj_at_step on the banded edge LP (rows of 0 .. 14 entries, stretches of empty rows, empty columns, m and n no
    multiple of anything): y' and A^T y' within the derived bounds, everything else as on the other layouts"""
    set_tune(monkeypatch, jag_waves=waves)
    p, x0, y0, S = banded()
    batch, solvers, devs, probs, sp = open_batch(p, x0, y0, K, "jag", monkeypatch, batch_lanes=16)
    name = "K%d-jag-%d-waves" % (K, waves)
    try:
        want = set(bc.JAG_FEATURES) - ({"kmax not a multiple of U"} if bc.jag_unroll(K, waves) == 1 else set())
        for side, off in enumerate((S.off, S.t_off)):
            v = batch.view(side)
            assert (v["K"], v["layout"], v["rows"]) == (K, "jag", len(off) - 1) and v["row0"][0] == 0 and v["row0"][-1] >= v["rows"], v
            missing = want - bc.jag_features(off, v["row0"], K, waves)
            assert not missing, (name, "side %d" % side, sorted(missing), v["row0"])
        worst = bc.run_batch_scenario(batch, devs, S, probs, sp, name, refresh=lambda l: dict(probs[l], **devs[l].bounds()), jag=(True, True))
    finally:
        close_all(batch, solvers)
    print(worst.line(name))
    print("JAGBITS %s %s" % (name, " ".join("%s=%d" % kv for kv in sorted(worst.bits.items()))))
    assert max(worst.values()) <= 1.0, worst


def test_the_hooks_refuse_what_they_do_not_serve(monkeypatch):
    p, x0, y0, S = edge()
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    with batch_of(p, bc.members(p, 2), **KW) as (batch, solvers):
        for count in (0, 65):
            with pytest.raises(capi.CuOptError) as e:
                batch.debug_attempts(count)
            assert e.value.code == -1
    with batch_of(p, bc.members(p, 2), **hc.KW) as (batch, solvers):
        with pytest.raises(capi.CuOptError) as e:
            batch.debug_attempts(1)
        assert e.value.code == -7


# ---- the existing contract at the edge shapes: bit-identity with single solves ------------------------------------------------------------
_singles = {}


def single(p, l, member, steps, state, **kw):
    """member l's single solve under the layout and tune of the caller's environment: its state after each of `steps` (None: to the
    end).  Computed once per LP, member, environment, steps and settings and shared, never changed."""
    key = (id(p), l, os.environ.get("CUOPT_AMD_SPMV_LAYOUT"), os.environ.get("CUOPT_AMD_TUNE"), steps, tuple(sorted(kw.items())))
    if key not in _singles:
        lb, ub, lo, hi, _ = member
        s = capi.Solver(dict(p, lb=lb, ub=ub, lo=lo, hi=hi), **kw)
        try:
            _singles[key] = [state(s, s.advance() if n is None else s.advance(n)) for n in steps]
        finally:
            s.close()
    return _singles[key]


def averaging_state(s, result):
    return result, s.solution()


def check_trajectories(p, K, layout, monkeypatch, **kw):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    ms = bc.members(p, K)
    kw = dict(KW, **kw)
    want = [single(p, l, ms[l], (130, None), averaging_state, **kw) for l in range(K)]
    with batch_of(p, ms, **kw) as (batch, solvers):
        lay = solvers[0].device.layout()
        assert lay["A"]["layout"] == lay["At"]["layout"] == layout, lay
        for i, n in enumerate((130, None)):
            got = batch.advance() if n is None else batch.advance(n)
            assert n is None or all(g["steps_taken"] == n for g in got), [g["steps_taken"] for g in got]  # (nobody is done before the checkpoint)
            for l in range(K):
                same(got[l], want[l][i][0], solvers[l].solution(), want[l][i][1], "LP %d, checkpoint %d" % (l, i))
        print("TRAJECTORIES %s K=%d: steps %s, status %s" % (layout, K, [g["steps_taken"] for g in got], sorted({g["status_name"] for g in got})))


@pytest.mark.parametrize("layout", ["stream", "panel"])
@pytest.mark.parametrize("K", [2, 4, 8, 16])
def test_batch_trajectories_at_the_edge_shapes(K, layout, monkeypatch):
    check_trajectories(edge()[0], K, layout, monkeypatch)


@pytest.mark.parametrize("K", [2, 16])
def test_jagged_batch_trajectories_at_the_edge_shapes(K, monkeypatch):
    check_trajectories(banded()[0], K, "jag", monkeypatch, batch_lanes=16)


HALPERN_STEPS = (1, 1, 1, 37, 90)  # checkpoints after 1, 2, 3, 40 and 130 steps (a Halpern step is never rejected)


@pytest.mark.parametrize("layout", ["stream", "panel"])
@pytest.mark.parametrize("K", [2, 16])
def test_halpern_batch_trajectories_at_the_edge_shapes(K, layout, monkeypatch):
    """kb_a_halpern / kb_at_halpern on blocks of 0, 1 and 3 chunks, 128-entry rows and workgroups of fewer than 64 rows"""
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    p = edge()[0]
    ms = bc.members(p, K)
    want = [single(p, l, ms[l], HALPERN_STEPS, hc.state, **hc.KW) for l in range(K)]
    with batch_of(p, ms, **hc.KW) as (batch, solvers):
        hc.layout_is(solvers[0], layout)
        taken = 0
        for i, n in enumerate(HALPERN_STEPS):
            got = batch.advance(n)
            taken += n
            assert all(g["steps_taken"] == taken for g in got), (taken, [g["steps_taken"] for g in got])
            for l in range(K):
                hc.same(hc.state(solvers[l], got[l]), want[l][i], "LP %d after %d steps" % (l, taken))


@pytest.mark.parametrize("layout", ["stream", "panel"])
def test_k_wide_plain_product_at_the_edge_shapes(layout, monkeypatch):
    """kb_plain (pdlpdev_batch_spmv) on the edge LP: every member's product bit for bit the parent's own"""
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    p, K = edge()[0], 4
    with batch_of(p, bc.members(p, K), **hc.KW) as (batch, solvers):
        hc.layout_is(solvers[0], layout)
        parent, rng = solvers[0], np.random.default_rng(17)
        for transpose in (False, True):
            cols, rows = (parent.m, parent.n) if transpose else (parent.n, parent.m)
            vs = [rng.standard_normal(cols) for _ in range(K)]
            want = [parent.device.spmv(v, transpose, rows) for v in vs]
            for on in (None, [1, 0, 1, 1]):
                got = batch.spmv(vs, transpose=transpose, on=on)
                for l in range(K):
                    if on is None or on[l]:
                        assert ar.bits_equal(got[l], want[l]), (layout, transpose, l, ar._first(got[l], want[l]))
                    else:
                        assert np.isnan(got[l]).all(), (layout, transpose, l)
