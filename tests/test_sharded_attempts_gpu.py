"""GPU: the adaptive PDHG attempt and the convergence evaluation of the ROW-BLOCK SHARDED path against the stage-by-stage references
(tests/attempt_reference.py, tests/eval_reference.py), on the GLOBAL LP.

W ranks -- host threads with a solver each, on one device behind the in-process communicator -- sit behind the scenario's interface
(tests/sharded_ranks.py); tests/attempt_scenario.run_scenario and attempt_reference.check_attempt run unchanged on what the ranks'
buffers assemble to.  This reaches what no single-GPU test does, the four sharded sequences that enqueue_attempt chooses among
(cuopt_amd/csrc/pdlp_device.hip enqueue_replicated, enqueue_rsag, enqueue_owner_collective, enqueue_owner_p2p): k_primal on a column
slice with a short or empty last slice (launch_primal_slice), the partial A^T product with the dy2 partial behind it,
k_sum_partials_to, k_step_stats, k_pack_step_sums, k_step_decision fed with all-reduced scalars (launch_decision_reduced), the
owner-computes column block (its own layout, its own scaling order), the gathered dual at ypad strides, the direct peer transport's
k_pull / k_pull_ranges (p2p_pull) / k_step_decision_p2p, the three all-gathers of run_epilogue -- and, for the evaluation,
k_eval_dual_elementwise behind the n + 3 all-reduce.  No bound is wider than
the single-GPU tests' (attempt_reference's docstring, "THE SHARDED PATH", says why none needs to be).

The 6000 x 6000 LP's row blocks (capi.partition_rows) and slices, asserted in tests/test_attempt_reference.py:
    world 2   rows 2979 / 3021                  slice 3008, the last one 2992
    world 3   rows 1924 / 1955 / 2121           slice 2000, the last one full
    world 4   rows 1501 / 1478 / 1442 / 1579    slice 1504, the last one 1488
    world 8   rows 649 .. 796                   slice 752,  the last one 736
tests/test_attempt_reference.py runs every case below on float64 stand-in ranks first: the LPs keep the scenario's properties in the
sharded order of summation, and the assembly reads nothing a rank does not own.

A zero-row block is not among the cases: cuoptamd_solver_create refuses an LP whose partition has one (tests/test_capi_host.py)."""
import numpy as np
import pytest
from conftest import set_tune

import attempt_reference as ar
import attempt_scenario as sc
import eval_reference as er
import sharded_ranks as sr
from cuopt_amd import capi
from oracle import orcbind
from test_attempt_layouts_gpu import step_params
from test_eval_layouts_gpu import VARIANTS, _check_scalars, _check_vectors, variant_lp

pytestmark = pytest.mark.gpu
FLOWS = ("allreduce", "rsag", "owner")
LAYOUT_IDS = ("panel-rows-4KiB", "panel-longtail", "jag-8", "pb", "dense-stream", "dense-panel-longtail")
LAYOUT_CASES = [(f, i) for f in ("allreduce", "owner") for i in LAYOUT_IDS] + [("rsag", "stream"), ("rsag", "panel-longtail")]
TRANSPORTS = {"collective-halo": (None, None), "p2p": ("p2p", 0), "p2p-halo": ("p2p", None)}  # id -> (CUOPT_AMD_SHARD_TRANSPORT, shard_halo)


@pytest.fixture(autouse=True)
def multi_launch_kernels(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")  # keep the small LPs' single context off the resident one-workgroup path


_single = {}


def single_context_scaling(key, p):
    """D_r and D_c of ONE context (Ruiz 10 + Pock-Chambolle alpha 1, as the solver's mode 1 scales).  Computed once per LP."""
    if key not in _single:
        raw = capi.Device(p)
        raw.call("scaling_compute", 1, 10, 1, 1.0)
        _single[key] = (raw.download("DROW", raw.m), raw.download("DCOL", raw.n))
        raw.close()
    return _single[key]


def check_scaling(p, S, prob, dr, dc, one, tag):
    """D_r assembled from the ranks is a single context's bit for bit.  D_c is NOT, and cannot be: the Pock-Chambolle pass divides by
    the square root of a column's 1-norm, which a sharded context adds up as per-rank partial sums in rank order (the all-reduce of
    pdlpdev_scaling_compute) and a single context as one chain down the column -- two summation trees over the same L_j positive
    terms, each within (L_j - 1) u of the exact sum.  Behind the square root and the division that is at most (L_j + 4) u of D_c
    (the ten Ruiz passes take maxima, which are exact in any order; D_r's sums run along a rank's own rows).  Every rank holds the same
    D_c (Assembled.get asserts it), and the scaled problem the ranks hold is the global LP scaled with the assembled D_r and D_c by
    pdlpdev_scale_problem's expressions, bit for bit: sharding adds no other difference."""
    assert ar.bits_equal(dr, one[0]), (tag, "D_r assembled from the ranks is not a single context's")
    ratio = np.abs(dc - one[1]) / ((S.len_c + 4) * er.U * one[1])
    print("SCALING %s: D_c differs from a single context's in %d of %d columns, at most %.3f of (L + 4) u" % (tag, (dc != one[1]).sum(), len(dc), ratio.max()))
    assert ratio.max() <= 1.0, (tag, "D_c further from a single context's than two summation orders of a column explain", int(np.argmax(ratio)), ratio.max())
    want = dict(A_VALUES=np.asarray(p["values"], float) * dr[S.rows] * dc[S.idx], C=p["c"] * dc, LB=p["lb"] / dc, UB=p["ub"] / dc, LO=p["lo"] * dr, HI=p["hi"] * dr)
    for k in ar.PROBLEM:
        assert ar.bits_equal(prob[k], want[k]), (tag, "%s of the ranks is not the global LP scaled with the assembled D_r and D_c" % k)


def open_ranks(key, p, x0, y0, world, flow, monkeypatch, name="stream", scaled=True, **solver_kw):
    """W prepared ranks under dataflow `flow`, both local sides in the layout of id `name` (test_eval_layouts_gpu.VARIANTS)
    -> (Assembled, Structure, the scaled problem as the ranks hold it, D_r, D_c)"""
    layout, knobs = VARIANTS[name][:2]
    monkeypatch.setenv("CUOPT_AMD_SHARD_DATAFLOW", flow)
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    set_tune(monkeypatch, dense=1 if VARIANTS[name][3] else 0, **knobs)
    dev = sr.on_device(p, x0, y0, step_params(1), world, flow, **solver_kw)
    try:
        for rank, info in enumerate(dev.b.info):
            lay = info["layout"]
            assert not lay["resident"] and lay["A"]["layout"] == lay["At"]["layout"] == layout, (name, rank, lay)
            if layout == "panel":
                assert lay["A"]["row_sums"] == lay["At"]["row_sums"] == ("by_nonzero" if knobs["panel_seg"] else "by_row"), (name, rank, lay)
            assert not info["dense"]["on"], "dense row segments are a single-GPU layout: a rank multiplies its whole block"
        if flow == "owner":
            print("OWNER_LAYOUT %s world %d: %s" % (name, world, " ".join(i["owner_layout"]["layout"] for i in dev.b.info)))
        c = dev.ctl()
        assert (c["cur"], c["pending_avg"], c["steps_taken"], c["attempts"], c["error"]) == (0, 0, 0, 0, 0) and c["sigma"] == c["step_size"], c
        S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
        prob, dr, dc = sc.download_problem(dev), dev.get("DROW"), dev.get("DCOL")
        if scaled:
            check_scaling(p, S, prob, dr, dc, single_context_scaling(key, p), "%s %s world %d" % (name, flow, world))
    except BaseException:
        dev.close()
        raise
    return dev, S, prob, dr, dc


def scenario(key, p, x0, y0, world, flow, monkeypatch, name="stream", tag=None, **solver_kw):
    dev, S, prob, dr, dc = open_ranks(key, p, x0, y0, world, flow, monkeypatch, name, **solver_kw)
    try:
        tag = tag or "%s %s world %d" % (name, flow, world)
        worst = sc.run_scenario(dev, S, prob, dev.sp, dr, dc, tag)
    finally:
        dev.close()
    print(worst.line(tag.replace(" ", "-")))
    assert max(worst.values()) <= 1.0, worst


# ---- a. dataflows and worlds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("flow", FLOWS)
def test_sharded_attempts_against_the_reference(flow, world, monkeypatch):
    p, x0, y0 = variant_lp("stream")[:3]
    scenario(VARIANTS["stream"][2:4], p, x0, y0, world, flow, monkeypatch)


# ---- b. the SpMV layouts at world 4 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow,name", LAYOUT_CASES, ids=["%s-%s" % c for c in LAYOUT_CASES])
def test_sharded_attempts_in_the_layouts(flow, name, monkeypatch):
    p, x0, y0 = variant_lp(name)[:3]
    scenario(VARIANTS[name][2:4], p, x0, y0, 4, flow, monkeypatch, name)


# ---- c. the direct peer transport and the halo exchange (owner-computes, world 4) -----------------------------------------------------------
_band = {}


def band_case():
    if not _band:
        _band["lp"] = sr.band_lp(*sr.BAND_LP)
    return _band["lp"]


def open_band(transport, monkeypatch, **solver_kw):
    kind, halo = TRANSPORTS[transport]
    if kind:
        monkeypatch.setenv("CUOPT_AMD_SHARD_TRANSPORT", kind)
    else:
        monkeypatch.delenv("CUOPT_AMD_SHARD_TRANSPORT", raising=False)
    set_tune(monkeypatch, shard_halo=halo, reorder=0)  # (the ranks keep the caller's order: the assembly is by the caller's rows and columns)
    p, x0, y0 = band_case()
    out = open_ranks("band", p, x0, y0, 4, "owner", monkeypatch, **solver_kw)
    for rank, info in enumerate(out[0].b.info):
        if info["wire"]["halo"] != (halo is None) or info["p2p"] != (kind == "p2p"):
            out[0].close()
            raise AssertionError((transport, rank, info["wire"], info["p2p"]))
    return out


@pytest.mark.parametrize("transport", list(TRANSPORTS))
def test_transport_and_halo_against_the_reference(transport, monkeypatch):
    dev, S, prob, dr, dc = open_band(transport, monkeypatch)
    try:
        worst = sc.run_scenario(dev, S, prob, dev.sp, dr, dc, "band " + transport)
    finally:
        dev.close()
    print(worst.line("band-%d-%d-%s" % (*sr.BAND_LP, transport)))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("transport", ["p2p", "p2p-halo"])
def test_peer_transport_plain_launches_equal_graph_replay(transport, monkeypatch):
    """the direct peer transport is kernels only and replays attempt graphs: the same eight attempts as plain launches leave every
    buffer and the control block bit for bit (the in-process communicator's collectives are never captured)"""
    records = []
    for graph in (1, 0):
        dev, S, prob, dr, dc = open_band(transport, monkeypatch, use_graph=graph)
        records.append([])
        try:
            sc.natural_attempts(dev, S, prob, dev.sp, "band %s graph=%d" % (transport, graph), sc.Worst(), records[-1])
        finally:
            dev.close()
    for i, (g, plain) in enumerate(zip(*records)):
        assert g["ctl"] == plain["ctl"], (transport, i, g["ctl"], plain["ctl"])
        for k in ar.STATE + ("XBAR",):
            assert ar.bits_equal(g[k], plain[k]), (transport, i, k)


# ---- d. empty slices: 40 x 60 at world 8, slices of 16 columns ------------------------------------------------------------------------------
@pytest.mark.parametrize("flow", FLOWS)
@pytest.mark.parametrize("kind", ["fixed-point", "dual-only"])
def test_scalar_branches_with_empty_slices(kind, flow, monkeypatch):
    """rank 3 holds 12 columns and ranks 4 .. 7 none: k_primal, k_step_stats and the column block's product over an empty range, the
    all-gathers and the reduce-scatter of slices that lie behind the vector's end"""
    p, x0, y0 = sc.tiny_lp(kind)
    monkeypatch.setenv("CUOPT_AMD_SHARD_DATAFLOW", flow)
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    dev = sr.on_device(p, x0, y0, step_params(1), 8, flow)
    try:
        assert flow == "allreduce" or [s[1] for s in dev.slices] == [16, 16, 16, 12, 0, 0, 0, 0], dev.slices
        S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
        prob = sc.download_problem(dev)
        r, before, after = sc.one_attempt(dev, S, prob, dev.sp, "%s %s" % (kind, flow))
        sc.assert_scalar_branch(kind, r, before, after, dev.sp)
    finally:
        dev.close()


# ---- e. a call of twelve attempts is twelve calls of one ------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow", ["allreduce", "owner"])
def test_one_call_is_the_composition_of_single_attempts(flow, monkeypatch):
    """attempt_scenario.check_composition's part (a): the current side and the control block bit for bit, target_steps apart (it is
    what each call was asked for) -- between the single calls run_epilogue replicates the primal side, inside the one call it does not"""
    p, x0, y0 = variant_lp("stream")[:3]
    ends = []
    for single in (False, True):
        dev = open_ranks(VARIANTS["stream"][2:4], p, x0, y0, 4, flow, monkeypatch)[0]
        try:
            first = dev.ctl()
            for _ in range(sc.LAUNCH_ATTEMPTS if single else 1):
                dev.attempts(1 if single else sc.LAUNCH_ATTEMPTS)
            ends.append(sc.snapshot(dev))
        finally:
            dev.close()
    sc._same(ends[0], ends[1], "%s: one call against single attempts" % flow, skip=("target_steps",))
    c = ends[0]["ctl"]
    assert c["attempts"] - first["attempts"] == sc.LAUNCH_ATTEMPTS and c["error"] == 0 and c["steps_taken"] > first["steps_taken"], c


# ---- the sharded evaluation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stream", "dense-panel-rows"])
@pytest.mark.parametrize("flow", FLOWS)
def test_sharded_evaluation_against_the_reference(flow, name, monkeypatch):
    """pdlpdev_eval on row blocks: the A product on the rank's rows, the partial A^T product and the three dual-side row sums in ONE
    all-reduce of n + 3, k_eval_dual_elementwise on the replicated sum.  The eight scalars at the tolerances of the single-GPU test and
    identical on all ranks; A x per row from the row blocks, A^T y and the reduced costs per column (replicated) within the reference's
    derived bounds; the infeasibility information against the oracle."""
    p, x0, y0, empty_rows, empty_cols = variant_lp(name)
    dev, S, prob, dr, dc = open_ranks(VARIANTS[name][2:4], p, x0, y0, 4, flow, monkeypatch, name)
    tag = "%s %s" % (name, flow)
    worst = {}

    def evaluated(which, slot, xname, yname, rule, phase):
        xs, ys = dev.get(xname) * dc, dev.get(yname) * dr
        for eps in (1e-4, -1.0):
            ref = er.evaluate(p, xs, ys, rule_finite=rule, eps_p=eps, eps_d=eps)
            ev = dev.eval(which, rule, eps)
            _check_scalars(ev, ref, eps >= 0, "%s %s %s eps=%g" % (tag, phase, slot or "LAST_RESTART", eps))
            if slot:
                for k, v in _check_vectors(dev, slot, ref, empty_rows, empty_cols, "%s %s %s eps=%g" % (tag, phase, slot, eps)).items():
                    worst[k] = max(worst.get(k, 0.0), v)
        return xs, ys

    try:
        dev.run(2)  # two accepted steps: the ping-pong pairs have been on side 1 and are back on side 0
        c = dev.ctl()
        assert (c["steps_taken"], c["cur"], c["error"]) == (2, 0, 0) and c["attempts"] >= 2, c
        evaluated(capi.CURRENT, "CURRENT", "X", "Y", True, "two steps")
        dev.run(3)  # one more: side 1, and an average made
        c = dev.ctl()
        assert (c["steps_taken"], c["cur"], c["error"]) == (3, 1, 0), c
        dev.flush()
        dev.make_average(2)
        xa, ya = evaluated(capi.AVERAGE, "AVERAGE", "AVG_X", "AVG_Y", True, "three steps")
        xc, yc = evaluated(capi.CURRENT, "CURRENT", "X", "Y", True, "three steps")
        assert np.abs(xc - xa).max() > 1e-3 and np.abs(yc - ya).max() > 1e-3
        got = dev.eval_infeasibility(capi.CURRENT, rule_finite=True)
        orc = orcbind.evaluate_infeasibility(p, xc, yc, finite_bounds_rule=True)
        for k in orc:
            assert got[k] == pytest.approx(orc[k], rel=1e-10, abs=1e-12), (tag, k)
        # the last restart point: restart to the average, two more steps, so that the anchor is neither the current iterate nor the average
        dev.restart(capi.AVERAGE, 0)
        dev.compute_aty()
        dev.run(5)
        assert dev.ctl()["steps_taken"] == 5 and ar.bits_equal(dev.get("LAST_RESTART_X") * dc, xa)
        kept = {k: dev.get(k) for k in ("RC_CURRENT", "AX_U_CURRENT", "ATY_U_CURRENT")}
        evaluated(capi.LAST_RESTART, None, "LAST_RESTART_X", "LAST_RESTART_Y", False, "restarted")
        for k, v in kept.items():  # (its vectors go to slots of their own, the reduced costs to scratch)
            assert ar.bits_equal(dev.get(k), v), (tag, "the evaluation of the last restart point wrote", k)
    finally:
        dev.close()
    print("WORST-EVAL %s ax=%.3f aty=%.3f rc=%.3f" % (tag.replace(" ", "-"), worst["ax"], worst["aty"], worst["rc"]))
