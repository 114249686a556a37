"""GPU: the reflected-Halpern step of the ROW-BLOCK SHARDED path (cuoptamd_settings::halpern_sharded, owner-computes dataflow) against
the stage-by-stage reference (tests/halpern_step_reference.py), on the GLOBAL LP.

W ranks -- host threads with a mode-4 solver each, on one device behind the in-process communicator -- sit behind the scenario's
interface (tests/halpern_sharded_ranks.py); tests/halpern_step_scenario.run_scenario, check_step and check_restart run unchanged on
what the ranks' buffers assemble to.  This reaches what no single-GPU test does: k_primal on a slice with pending_avg = 0, the A
product with HalpernShardedDualEpilogue (y' into the average slot, the gathered dual and -- peer transport -- the peers' blocks), the
column block's A^T product with HalpernStepEpilogue on sliced anchors, k_halpern_decision_sums behind the 3-scalar all-reduce,
k_halpern_decision_p2p, the all-reduced dual distance of pdlpdev_halpern_restart, the sharded power iteration, and run_epilogue's
replication of x^{k+1}, A^T y^{k+1} and x'.

Bit for bit: x', xbar, x^{k+1}, y^{k+1} from the device's own y', the counters and pdlpdev_halpern; within the reference's derived
bounds: y' and A^T y^{k+1}, the three sums, the distances and the weight.  The control block and pdlpdev_halpern are identical on all
ranks, the restart's distances the same bits on all ranks (the assembly asserts both on every read).  No bound is widened.

The 6000 x 6000 LP's row blocks and short last slices are the ones tests/test_sharded_attempts_gpu.py lists.  The peer transport's
cases stay at world 4: the ranks' kernels wait for each other and need a hardware queue each.

Every case fails on a library without the feature: capi.Solver(mode=4, halpern_sharded=1, world=...) has no such field / answers -7."""
import numpy as np
import pytest
from conftest import set_tune

import attempt_reference as ar
import attempt_scenario as asc
import eval_reference as er
import halpern_sharded_ranks as hs
import halpern_step_reference as hr
import halpern_step_scenario as sc
import sharded_ranks as sr
from cuopt_amd import capi
from test_eval_layouts_gpu import VARIANTS, _check_scalars, variant_lp
from test_halpern_step_reference import overflow_lp

pytestmark = pytest.mark.gpu
LAYOUT_IDS = ("stream", "panel-rows-4KiB", "panel-longtail", "jag-8", "pb")
TRANSPORTS = {"collective-halo": (None, None), "p2p": ("p2p", 0), "p2p-halo": ("p2p", None)}  # id -> (CUOPT_AMD_SHARD_TRANSPORT, shard_halo)
COMPARED = ("X", "Y", "ATY", "AVG_X", "AVG_Y")


@pytest.fixture(autouse=True)
def multi_launch_kernels(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")  # keep the small LPs off the resident one-workgroup path
    monkeypatch.setenv("CUOPT_AMD_SHARD_DATAFLOW", "owner")
    monkeypatch.delenv("CUOPT_AMD_SHARD_TRANSPORT", raising=False)


def open_ranks(p, x0, y0, world, monkeypatch, name="stream", **solver_kw):
    """W prepared Halpern ranks, both local sides in the layout of id `name` -> (HalpernAssembled, Structure, the scaled problem)"""
    layout, knobs = VARIANTS[name][:2]
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    set_tune(monkeypatch, dense=0, **knobs)
    return _opened(p, x0, y0, world, name, layout, **solver_kw)


def _opened(p, x0, y0, world, name, layout, **solver_kw):
    dev = hs.on_device(p, x0, y0, world, **solver_kw)
    try:
        for rank, info in enumerate(dev.b.info):
            lay = info["layout"]
            assert not lay["resident"] and (layout is None or lay["A"]["layout"] == lay["At"]["layout"] == layout), (name, rank, lay)
        print("OWNER_LAYOUT %s world %d: %s" % (name, world, " ".join(i["owner_layout"]["layout"] for i in dev.b.info)))
        c = dev.ctl()
        assert (c["cur"], c["pending_avg"], c["steps_taken"], c["attempts"], c["error"]) == (0, 0, 0, 0, 0), c
        assert c["step_size"] == hs.H.STEP_SAFETY / dev.sigma_max() and c["tau"] == c["step_size"] / c["primal_weight"], c
        S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
        prob = sc.download_problem(dev)
    except BaseException:
        dev.close()
        raise
    return dev, S, prob


def scenario(dev, S, prob, tag):
    try:
        worst = sc.run_scenario(dev, S, prob, tag)
    finally:
        dev.close()
    print(worst.line(tag.replace(" ", "-")))
    assert max(worst.values()) <= 1.0, worst


# ---- a. worlds --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 8])
def test_sharded_steps_against_the_reference(world, monkeypatch):
    p, x0, y0 = variant_lp("stream")[:3]
    dev, S, prob = open_ranks(p, x0, y0, world, monkeypatch)
    scenario(dev, S, prob, "stream world %d" % world)


# ---- b. the SpMV layouts at world 4 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAYOUT_IDS)
def test_sharded_steps_in_the_layouts(name, monkeypatch):
    p, x0, y0 = variant_lp(name)[:3]
    dev, S, prob = open_ranks(p, x0, y0, 4, monkeypatch, name)
    scenario(dev, S, prob, "%s world 4" % name)


# ---- c. the transports at world 4 on the band LP ----------------------------------------------------------------------------------------
_band = {}


def open_band(transport, monkeypatch, **solver_kw):
    kind, halo = TRANSPORTS[transport]
    if kind:
        monkeypatch.setenv("CUOPT_AMD_SHARD_TRANSPORT", kind)
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    set_tune(monkeypatch, shard_halo=halo, reorder=0)  # (the ranks keep the caller's order: the assembly is by the caller's rows and columns)
    if not _band:
        _band["lp"] = sr.band_lp(*sr.BAND_LP)
    p, x0, y0 = _band["lp"]
    out = _opened(p, x0, y0, 4, "band " + transport, "stream", **solver_kw)
    for rank, info in enumerate(out[0].b.info):  # (the wire figures say which exchange runs)
        if info["wire"]["halo"] != (halo is None) or info["p2p"] != (kind == "p2p"):
            out[0].close()
            raise AssertionError((transport, rank, info["wire"], info["p2p"]))
    return out


@pytest.mark.parametrize("transport", list(TRANSPORTS))
def test_transport_and_halo_against_the_reference(transport, monkeypatch):
    dev, S, prob = open_band(transport, monkeypatch)
    scenario(dev, S, prob, "band " + transport)


def _end_state(dev):
    out = {k: dev.get(k) for k in COMPARED}
    out["ctl"], out["hal"] = dev.ctl(), dev.hal()
    return out


def _same_ends(a, b, tag, skip=()):
    assert {k: v for k, v in a["ctl"].items() if k not in skip} == {k: v for k, v in b["ctl"].items() if k not in skip}, (tag, a["ctl"], b["ctl"])
    assert a["hal"] == b["hal"], (tag, a["hal"], b["hal"])
    for k in COMPARED:
        assert ar.bits_equal(a[k], b[k]), (tag, k, int(np.argmax(a[k] != b[k])))


@pytest.mark.parametrize("transport", ["p2p", "p2p-halo"])
def test_peer_transport_plain_launches_equal_graph_replay(transport, monkeypatch):
    """the peer transport is kernels only and replays step graphs (4 + 2 + 1): the same seven steps as plain launches leave every
    buffer, the control block and pdlpdev_halpern bit for bit"""
    ends = []
    for graph in (1, 0):
        dev = open_band(transport, monkeypatch, use_graph=graph)[0]
        try:
            c = dev.run(sc.RUN_STEPS)
            assert (c["steps_taken"], c["attempts"], c["error"]) == (sc.RUN_STEPS, sc.RUN_STEPS, 0), c
            ends.append(_end_state(dev))
        finally:
            dev.close()
    assert ends[0]["hal"]["k"] == sc.RUN_STEPS and ends[0]["hal"]["r2_min"] > 0.0
    _same_ends(ends[0], ends[1], transport + ": graph replay against plain launches")


# ---- d. empty slices: 40 x 60 at world 8, slices 16, 16, 16, 12, 0, 0, 0, 0 -------------------------------------------------------------
def open_tiny(p, x0, y0, world, monkeypatch, transport=None):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    if transport:
        monkeypatch.setenv("CUOPT_AMD_SHARD_TRANSPORT", transport)
    return _opened(p, x0, y0, world, "tiny", "stream")


def test_a_fixed_point_with_empty_slices(monkeypatch):
    p, x0, y0 = asc.tiny_lp("fixed-point")
    dev, S, prob = open_tiny(p, x0, y0, 8, monkeypatch)
    try:
        assert [s[1] for s in dev.slices] == [16, 16, 16, 12, 0, 0, 0, 0], dev.slices
        start = sc.snapshot(dev)
        for i in range(2):
            r, before, after = sc.one_step(dev, S, prob, "fixed point %d" % i)
            assert (r["r2"], r["dx2"], r["dy2"], r["inter"], r["error"]) == (0.0, 0.0, 0.0, 0.0, 0), r
            assert (after["hal"]["r"], after["hal"]["r_first"], after["hal"]["r2"], after["hal"]["r2_min"]) == (0.0, 0.0, 0.0, 0.0), after["hal"]
            if i == 0:
                assert all(ar.bits_equal(after[k], start[k]) for k in ("X", "Y", "ATY")), "the fixed point moved"
    finally:
        dev.close()


@pytest.mark.parametrize("world,transport", [(8, None), (4, "p2p")], ids=["collective-world-8", "p2p-world-4"])
def test_an_overflow_raises_the_step_error_on_every_rank(world, transport, monkeypatch):
    """Y with 1e200 on a "<=" row: dy^2 overflows on the rank that owns the row, the reduced r2 = inf reaches every rank: error = 1 on
    every rank, pdlpdev_halpern keeps every field on every rank, the counters advance -- the step error, not the transport's fault flag
    (a fault would make the run answer -6)"""
    p, x0, y0 = overflow_lp()
    dev, S, prob = open_tiny(p, x0, y0, world, monkeypatch, transport)
    try:
        if world == 8:
            assert [s[1] for s in dev.slices] == [16, 16, 16, 12, 0, 0, 0, 0], dev.slices
        assert prob["LO"][0] == -np.inf and np.isfinite(prob["HI"][0])
        y = dev.get("Y")
        y[0] = 1e200
        dev.put("Y", y)
        before = sc.snapshot(dev)
        assert before["Y"][0] == 1e200
        c = dev.run(1)
        after = sc.snapshot(dev, hr.AFTER)  # (ctl() and hal() assert that every rank holds rank 0's)
        assert hr.check_decision(before, after, "overflow world %d" % world)["error"] == 1
        assert after["ctl"]["last_dy2"] == np.inf and after["ctl"]["last_movement"] == np.inf and after["AVG_Y"][0] == 0.0, after["ctl"]
        assert after["hal"] == before["hal"], (before["hal"], after["hal"])
        assert tuple(c[k] for k in ("error", "attempts", "steps_taken", "k", "cur", "its_since_restart")) == (1, 1, 1, 1, 1, 1), c
        c = dev.run(2)
        assert (c["error"], c["attempts"], c["steps_taken"]) == (1, 1, 1) and dev.hal() == before["hal"]
    finally:
        dev.close()


# ---- e. a run of seven steps is seven runs of one ---------------------------------------------------------------------------------------
def test_a_run_is_the_composition_of_its_steps(monkeypatch):
    """the current side, T(z^k), the control block and pdlpdev_halpern bit for bit, target_steps apart -- between the single runs
    run_epilogue replicates the primal side, inside the one run it does not"""
    p, x0, y0 = variant_lp("stream")[:3]
    ends = []
    for single in (False, True):
        dev = open_ranks(p, x0, y0, 4, monkeypatch)[0]
        try:
            for target in (range(1, sc.RUN_STEPS + 1) if single else (sc.RUN_STEPS,)):
                c = dev.run(target)
                assert (c["steps_taken"], c["attempts"], c["error"]) == (target, target, 0), c
            ends.append(_end_state(dev))
        finally:
            dev.close()
    _same_ends(ends[0], ends[1], "one run against single steps", skip=("target_steps",))


# ---- f. the evaluation of T(z^k) and sigma_max ------------------------------------------------------------------------------------------
def test_sharded_evaluation_of_the_operator_output(monkeypatch):
    """behind a run, eval(AVERAGE) on every rank sees the replicated x' and the row-block y': the eight scalars at the tolerances of
    test_sharded_attempts_gpu.test_sharded_evaluation_against_the_reference, identical on all ranks (Assembled.eval asserts it)"""
    p, x0, y0 = variant_lp("stream")[:3]
    dev = open_ranks(p, x0, y0, 4, monkeypatch)[0]
    try:
        dr, dc = dev.get("DROW"), dev.get("DCOL")
        dev.run(3)
        xs, ys = dev.get("AVG_X") * dc, dev.get("AVG_Y") * dr
        assert np.isfinite(xs).all() and np.isfinite(ys).all() and np.abs(xs).max() > 0.0
        for eps in (1e-4, -1.0):
            ref = er.evaluate(p, xs, ys, rule_finite=True, eps_p=eps, eps_d=eps)
            _check_scalars(dev.eval(capi.AVERAGE, True, eps), ref, eps >= 0, "T(z^3) eps=%g" % eps)
    finally:
        dev.close()


def test_sigma_max_is_the_same_on_every_rank_and_a_single_contexts(monkeypatch):
    """the sharded power iteration returns the same bits on every rank (HalpernAssembled.sigma_max asserts it), also when it is run
    again, and lies within the iteration's own relative tolerance of a single context's on the same LP"""
    p, x0, y0 = variant_lp("stream")[:3]
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    one = capi.Solver(p, mode=4)
    tol = 1e-6  # (capi.Device.spectral_norm's default rel_tol, which both sides run with)
    single = one.device.spectral_norm(rel_tol=tol)[0]
    one.close()
    dev = open_ranks(p, x0, y0, 4, monkeypatch)[0]
    try:
        first = dev.sigma_max()
        xbar = dev.b.each("get_many", ("XBAR",))
        again = dev.sigma_max(again=True)
        print("SIGMA_MAX sharded %.17g single %.17g rel %.3g" % (first, single, abs(first - single) / single))
        assert again == first, (first, again)
        assert abs(first - single) <= tol * single, (first, single)
        for a, b in zip(xbar, dev.b.each("get_many", ("XBAR",))):
            assert ar.bits_equal(a["XBAR"], b["XBAR"]), "the power iteration left xbar changed"
    finally:
        dev.close()
