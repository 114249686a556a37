"""GPU: the frame around the iteration against tests/frame_reference.py -- the code that PRODUCES what the attempt, evaluation and
restart tests download and take as given (D_r, D_c, the scaled problem, the norms behind the first step, the primal weight and the
termination thresholds, the start), the reset between two solves, and the code that hands the result back.

(a) scaling          D_r, D_c and the nine scaled buffers bit for bit, A^T's own values among them, in every layout whose set-up takes
                     another norm kernel shape; pdlpdev_scaling_stats tells which shape served which side, and every shape must have run
(b) norms            pdlpdev_init_norms, pdlpdev_weight_norms(0 / 1), pdlpdev_problem_norms on the vectors the device holds: max|A| as
                     bits, the sums inside gamma_N S (printed as WORST lines), exact zeros; under 2 and 4 ranks
(c) the start        pdlpdev_set_initial, pdlpdev_project_primal as bits; pdlpdev_initial_solution_stats stage by stage in both forms
(d) reset            every iterate buffer and the control block zero, new bounds scaled as bits, NULL keeps; bounds array -> uniform ->
                     array: one attempt behind each reset is a fresh context's, bit for bit
(e) read-back        pdlpdev_get_solution(CURRENT / AVERAGE) at cur = 0 and cur = 1 as bits, NULL outputs skipped; beyond the wrap point

No bound here is measured: each is derived in tests/frame_reference.py, and tests/test_frame_reference.py proves on the CPU that the
reference alone stays inside it and that each comparison below can fail."""
import ctypes as C

import numpy as np
import pytest

import attempt_reference as ar
import attempt_scenario as sc
import frame_cases as fc
import frame_reference as fr
import sharded_ranks as sr
from attempt_reference import bits_equal
from cuopt_amd import capi
from oracle import orcbind
from test_attempt_layouts_gpu import step_params
from test_eval_layouts_gpu import open_variant

pytestmark = pytest.mark.gpu
CONTEXTS = fc.EDGE_IDS + ("1x1", "resident", "wrap")
START_CONTEXTS = ("stream", "panel-rows-4KiB", "jag-8", "pb", "resident", "1x1", "wrap")
ITERATE_BUFFERS = ("X", "Y", "X_OTHER", "Y_OTHER", "ATY", "ATY_OTHER", "XBAR", "SUM_X", "SUM_Y", "AVG_X", "AVG_Y", "LAST_RESTART_X", "LAST_RESTART_Y",
                   "RC_CURRENT", "RC_AVERAGE")
M_SIZED = ("Y", "Y_OTHER", "SUM_Y", "AVG_Y", "LO", "HI", "DROW", "LAST_RESTART_Y")

_refs = {}


def _lp_of(ctx):
    """(key of the LP, (p, x0, y0))"""
    if ctx in fc.EDGE_IDS:
        return ("edge-2400" if ctx == "pb" else "edge-4500-dense" if ctx.startswith("dense") else "edge-4500"), fc.edge(ctx)
    return ctx, {"1x1": fc.one_by_one, "resident": fc.resident, "wrap": fc.wrap, "zero-c": fc.zero_c, "free-rows": fc.free_rows}[ctx]()


def reference(ctx, preset):
    """(Structure, the scaled problem of the reference) per LP and preset: computed once, shared, read-only"""
    key, (p, x0, y0) = _lp_of(ctx)
    if (key, preset) not in _refs:
        S = _refs.setdefault((key, "S"), ar.Structure(p["m"], p["n"], p["offsets"], p["indices"]))
        dr, dc = fr.scaling(p, fc.PRESETS[preset], True, S)
        prob = fr.scaled_problem(p, dr, dc, S)
        for a in prob.values():
            a.setflags(write=False)
        _refs[(key, preset)] = (S, prob)
    return _refs[(key, preset)]


def open_context(ctx, monkeypatch):
    """-> (capi.Device, p, x0, y0) in the layout the id names"""
    key, (p, x0, y0) = _lp_of(ctx)
    if ctx in fc.EDGE_IDS:
        monkeypatch.setenv("CUOPT_AMD_SMALL", "0")
        return open_variant(ctx, p, monkeypatch), p, x0, y0
    monkeypatch.delenv("CUOPT_AMD_SPMV_LAYOUT", raising=False)
    if ctx == "resident":
        monkeypatch.delenv("CUOPT_AMD_SMALL", raising=False)
    else:
        monkeypatch.setenv("CUOPT_AMD_SMALL", "0")
    dev = capi.Device(p)
    lay = dev.layout()
    print("LAYOUT %s %s" % (ctx, lay))
    assert lay["resident"] == (ctx == "resident"), lay
    return dev, p, x0, y0


def get(dev, name):
    return dev.download(name, dev.nnz if name in ("A_VALUES", "AT_VALUES") else dev.m if name in M_SIZED else dev.n)


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not bits_equal(got, want):
        bad = np.nonzero(np.ascontiguousarray(got).view(np.int64) != np.ascontiguousarray(want).view(np.int64))[0]
        raise AssertionError("%s: %d of %d elements differ, the first at %d: %r against %r" % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]]))
    return True


def scaled(dev, iterations=10):
    dev.call("scaling_compute", 1, iterations, 1, 1.0)
    dev.call("scale_problem")


def flat(stats):
    return {(side, what, shape): v for side, d in stats.items() for what, e in d.items() for shape, v in e.items()}


# ---- (a) scaling -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", list(fc.PRESETS))
@pytest.mark.parametrize("ctx", CONTEXTS)
def test_scaling_bit_for_bit(ctx, preset, monkeypatch):
    dev, p, x0, y0 = open_context(ctx, monkeypatch)
    S, ref = reference(ctx, preset)
    tag = "%s %s" % (ctx, preset)
    assert_bits(get(dev, "AT_VALUES"), np.asarray(p["values"])[S.order], tag + ": A^T in front of the scaling (the stable transposition)")
    assert flat(dev.scaling_stats()) == {k: 0 for k in flat(dev.scaling_stats())}
    dev.call("scaling_compute", 1, fc.PRESETS[preset], 1, 1.0)
    dr, dc = get(dev, "DROW"), get(dev, "DCOL")
    assert_bits(dr, ref["DROW"], tag + " DROW")
    assert_bits(dc, ref["DCOL"], tag + " DCOL")
    assert (dr[S.len_r == 0] == 1.0).all() and (dc[S.len_c == 0] == 1.0).all(), tag
    assert ctx == "1x1" or ((S.len_r == 0).any() and (S.len_c == 0).any() and np.abs(dr - 1.0).max() > 1e-3 and np.abs(dc - 1.0).max() > 1e-3)
    dev.call("scale_problem")
    for k in fr.SCALED:
        assert_bits(get(dev, k), ref[k], "%s %s" % (tag, k))
    # the launches: per pass one of {row blocks, a lane per row} on each side, the long-row kernel wherever a side has a long row
    st = dev.scaling_stats()
    print("LAUNCHES %s %s" % (tag, " ".join("%s.%s.%s=%d" % (k + (v,)) for k, v in flat(st).items())))
    for side, lens in (("A", S.len_r), ("At", S.len_c)):
        for what, passes in (("max", fc.PRESETS[preset]), ("sum", 1), ("scale", 1)):
            e = st[side][what]
            assert sorted((e["blocks"], e["lanes"])) == [0, passes], (tag, side, what, e)
            assert e["long"] == (passes if (lens > fc.K_LONG_ROW).any() else 0), (tag, side, what, e)
    dev.close()


def test_every_scaling_kernel_shape_ran(monkeypatch):
    """over the contexts of test_scaling_bit_for_bit: row blocks, a lane per row and long rows, on A and on A^T, for the max passes, the
    sum pass and the value scaling.  The counters are the library's own (pdlpdev_scaling_stats), one per launch site."""
    total = {}
    for ctx in CONTEXTS:
        dev, p, x0, y0 = open_context(ctx, monkeypatch)
        scaled(dev, 1)
        st = flat(dev.scaling_stats())
        dev.close()
        print("SHAPES %-16s %s" % (ctx, " ".join("%s.%s.%s=%d" % (k + (v,)) for k, v in st.items())))
        for k, v in st.items():
            total[k] = total.get(k, 0) + v
    print("SHAPES %-16s %s" % ("total", " ".join("%s.%s.%s=%d" % (k + (v,)) for k, v in total.items())))
    assert len(total) == 18
    missing = [k for k, v in total.items() if v == 0]
    assert not missing, ("kernel shapes that no context ran", missing)


def test_pow_preset_against_the_oracle(monkeypatch):
    """preset 3 (no Ruiz, Pock-Chambolle with alpha = 2: pow() of ocml against libm's): the project's own figure, rtol 1e-14"""
    dev, p, x0, y0 = open_context("stream", monkeypatch)
    h, H = orcbind.hyper_preset(3), orcbind.H
    assert h[H["ORC_H_ALPHA_POCK_CHAMBOLLE"]] != 1.0
    dev.call("scaling_compute", int(h[H["ORC_H_DO_RUIZ"]]), int(h[H["ORC_H_RUIZ_ITERATIONS"]]), int(h[H["ORC_H_DO_POCK_CHAMBOLLE"]]),
             float(h[H["ORC_H_ALPHA_POCK_CHAMBOLLE"]]))
    dr, dc = orcbind.compute_scaling(p["m"], p["n"], p["offsets"], p["indices"], p["values"], h)
    got_r, got_c = get(dev, "DROW"), get(dev, "DCOL")
    dev.close()
    worst = max(np.abs(got_r / dr - 1.0).max(), np.abs(got_c / dc - 1.0).max())
    print("WORST pow-preset relative difference of D_r, D_c against the oracle: %.3e" % worst)
    np.testing.assert_allclose(got_r, dr, rtol=1e-14, atol=0)
    np.testing.assert_allclose(got_c, dc, rtol=1e-14, atol=0)


# ---- (b) norms ---------------------------------------------------------------------------------------------------------------------------
def norm_ratios(figures, p, prob, extra=0):
    """figures = dict(init=[3], w0=(2), w1=(2), prob=(2)) as the device returned them; prob: the scaled buffers the device holds.
    max|A| is compared as bits here -> the ratios of the sums"""
    mx, c2, b2 = fr.init_norms(prob, extra)
    assert figures["init"][0] == mx, ("max|A|", figures["init"][0], mx)
    c2u, b2u = fr.sum_squares(p["c"]), fr.sum_squares(fr.combine_bounds(p["lo"], p["hi"]), extra)
    nc, nb = fr.problem_norms(p["c"], p["lo"], p["hi"], extra)
    out = dict(init_c2=fr.ratio(c2, figures["init"][1]), init_b2=fr.ratio(b2, figures["init"][2]), w0_c2=fr.ratio(c2, figures["w0"][0]),
               w0_b2=fr.ratio(b2, figures["w0"][1]), w1_c2=fr.ratio(c2u, figures["w1"][0]), w1_b2=fr.ratio(b2u, figures["w1"][1]),
               norm_c=fr.ratio(nc, figures["prob"][0]), norm_b=fr.ratio(nb, figures["prob"][1]))
    return out, dict(c2=float(c2[0]), b2=float(b2[0]), c2u=float(c2u[0]), b2u=float(b2u[0]))


def device_norms(dev):
    return dict(init=dev.init_norms().tolist(), w0=dev.weight_norms(False), w1=dev.weight_norms(True), prob=dev.problem_norms())


@pytest.mark.parametrize("ctx", CONTEXTS + ("zero-c", "free-rows"))
def test_norms_against_the_reference(ctx, monkeypatch):
    dev, p, x0, y0 = open_context(ctx, monkeypatch)
    scaled(dev)
    prob = {k: get(dev, k) for k in ("A_VALUES", "C", "LO", "HI")}
    figures = device_norms(dev)
    dev.close()
    ratios, exact = norm_ratios(figures, p, prob)
    print("WORST norms %s " % ctx + " ".join("%s=%.3g" % kv for kv in ratios.items()))
    assert max(ratios.values()) <= 1.0, (ctx, ratios)
    if ctx == "zero-c":
        assert figures["init"][1] == 0.0 and figures["w0"][0] == 0.0 and figures["w1"][0] == 0.0 and figures["prob"][0] == 0.0, figures
        assert figures["init"][2] > 0.0
    elif ctx == "free-rows":
        assert figures["init"][2] == 0.0 and figures["w0"][1] == 0.0 and figures["w1"][1] == 0.0 and figures["prob"][1] == 0.0, figures
        assert figures["init"][1] > 0.0
    else:
        assert min(exact.values()) > 0.0


class FrameRank(sr.RankOnDevice):
    """a rank of tests/sharded_ranks.py with the frame's calls"""

    def norms(self):
        return device_norms(self.dev)

    def initial_stats(self, x0, y0):
        d = self.dev
        d.call("set_initial", capi._ptr(np.ascontiguousarray(x0)), capi._ptr(np.ascontiguousarray(y0[self.r0:self.r1])))
        first = d.initial_solution_stats().tolist()
        state = [d.download("X", self.n), d.download("Y", self.ml)]
        second = d.initial_solution_stats(np.ascontiguousarray(x0), np.ascontiguousarray(y0[self.r0:self.r1])).tolist()
        return dict(scaled=first, unscaled=second, x=state[0], y=state[1])


@pytest.mark.parametrize("world", [2, 4])
def test_norms_and_start_under_sharding(world, monkeypatch):
    """the all-reduced slots (max|A|, the sums over the rows, ||y0||^2, max|y0|): every rank returns rank 0's bits, and they are the
    whole LP's inside gamma_{N + world}; the interaction with the compound bound (the product's bound carried through the dot)"""
    p, x0, y0 = fc.edge("stream")
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")
    monkeypatch.setenv("CUOPT_AMD_SHARD_DATAFLOW", "allreduce")
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    monkeypatch.setattr(sr, "RankOnDevice", FrameRank)
    ranks = sr.DeviceRanks(p, x0, y0, step_params(1), world, "allreduce")
    try:
        dev = sr.Assembled(ranks, step_params(1))
        prob = {k: dev.get(k) for k in ("A_VALUES", "C", "LO", "HI")}
        dr, dc = dev.get("DROW"), dev.get("DCOL")
        per_rank = ranks.each("norms")
        for r, f in enumerate(per_rank):
            for k in f:
                assert bits_equal(np.array(f[k]), np.array(per_rank[0][k])), ("rank %d returns other %s norms than rank 0" % (r, k), f[k], per_rank[0][k])
        ratios, exact = norm_ratios(per_rank[0], p, prob, extra=world)
        print("WORST norms sharded-world%d " % world + " ".join("%s=%.3g" % kv for kv in ratios.items()))
        assert max(ratios.values()) <= 1.0 and min(exact.values()) > 0.0, ratios
        if world == 2:
            xs = fc.start(p, x0)
            stats = ranks.each("initial_stats", xs, y0)
            for r, s in enumerate(stats):
                for k in ("scaled", "unscaled"):
                    assert bits_equal(np.array(s[k]), np.array(stats[0][k])), ("rank %d returns other %s figures than rank 0" % (r, k), s[k], stats[0][k])
                assert_bits(s["x"], xs / dc, "rank %d X behind set_initial" % r)
                assert_bits(s["y"], y0[ranks.bounds[r]:ranks.bounds[r + 1]] / dr[ranks.bounds[r]:ranks.bounds[r + 1]], "rank %d Y behind set_initial" % r)
            S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
            for form, (x, y) in (("scaled", (xs / dc, y0 / dr)), ("unscaled", (xs, y0))):
                out = stats[0][form]
                product = ar.aty_product(S, prob, y)
                r5 = dict(interaction=fr.ratio(fr.interaction_through_product(x, product), out[0]), x2=fr.ratio(fr.sum_squares(x), out[1]),
                          y2=fr.ratio(fr.sum_squares(y, world), out[2]))
                print("WORST start sharded-world2 %s " % form + " ".join("%s=%.3g" % kv for kv in r5.items()))
                assert out[3] == fr.max_abs(x) and out[4] == fr.max_abs(y), (form, out)
                assert max(r5.values()) <= 1.0, (form, r5)
    finally:
        ranks.close()


# ---- (c) the start -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx", START_CONTEXTS)
def test_start_against_the_reference(ctx, monkeypatch):
    dev, p, x0, y0 = open_context(ctx, monkeypatch)
    S, ref = reference(ctx, "ruiz10-pc")
    scaled(dev)
    prob = {k: get(dev, k) for k in fr.SCALED}
    dr, dc = prob["DROW"], prob["DCOL"]
    xs = fc.start(p, x0)
    assert dev.ctl().cur == 0
    dev.call("set_initial", capi._ptr(xs), capi._ptr(np.ascontiguousarray(y0)))
    xh, yh = fr.to_scaled_start(xs, y0, dr, dc)
    assert_bits(get(dev, "X"), xh, ctx + " X behind set_initial")
    assert_bits(get(dev, "Y"), yh, ctx + " Y behind set_initial")
    worst = {}

    def stats(form, out, x, y, aty):
        product = ar.aty_product(S, prob, y)
        inter, x2, y2, mx, my = fr.initial_stats(x, y, aty)
        r = dict(aty=ar.worst_ratio(ar.abs_err(product, aty), product["bound"]), interaction=fr.ratio(inter, out[0]), x2=fr.ratio(x2, out[1]),
                 y2=fr.ratio(y2, out[2]))
        assert out[3] == mx and out[4] == my, (ctx, form, out[3], mx, out[4], my)
        assert (aty[S.len_c == 0] == 0.0).all(), (ctx, form)
        worst.update({form + "_" + k: v for k, v in r.items()})
        assert max(r.values()) <= 1.0, (ctx, form, r)

    # the scaled form: on the iterate set_initial left, A^T y0 stays in the current A^T y buffer
    out = dev.initial_solution_stats()
    assert_bits(get(dev, "X"), xh, ctx + " X behind the scaled form") and assert_bits(get(dev, "Y"), yh, ctx + " Y behind the scaled form")
    stats("scaled", out, xh, yh, get(dev, "ATY"))
    # the unscaled form: the caller's vectors pass through the other side, the current side is left alone
    kept = {k: get(dev, k) for k in ("X", "Y", "ATY")}
    out = dev.initial_solution_stats(xs, y0)
    for k, v in kept.items():
        assert_bits(get(dev, k), v, "%s %s behind the unscaled form" % (ctx, k))
    assert_bits(get(dev, "X_OTHER"), xs, ctx + " X_OTHER") and assert_bits(get(dev, "Y_OTHER"), np.asarray(y0), ctx + " Y_OTHER")
    stats("unscaled", out, xs, np.asarray(y0, dtype=np.float64), get(dev, "ATY_OTHER"))
    # the projection: the iterate and the average, each against its own input
    avg = np.ascontiguousarray(xh[::-1]) * 0.75
    dev.upload("AVG_X", avg)
    dev.call("project_primal")
    X, AVG = get(dev, "X"), get(dev, "AVG_X")
    dev.close()
    assert_bits(X, fr.clamp(xh, prob["LB"], prob["UB"]), ctx + " X behind project_primal")
    assert_bits(AVG, fr.clamp(avg, prob["LB"], prob["UB"]), ctx + " AVG_X behind project_primal")
    free = np.isinf(p["lb"]) & np.isinf(p["ub"])
    assert_bits(X[free], xh[free], ctx + " free columns") and assert_bits(AVG[free], avg[free], ctx + " free columns of the average")
    assert ctx == "1x1" or (free.any() and (X != xh).sum() > len(xh) // 4 and (AVG != avg).any())
    assert (X >= prob["LB"]).all() and (X <= prob["UB"]).all()
    print("WORST start %s " % ctx + " ".join("%s=%.3g" % kv for kv in worst.items()))


# ---- (d) reset ---------------------------------------------------------------------------------------------------------------------------
def begin(dev, x0, y0):
    """the start of test_attempt_layouts_gpu.prepared on a context already scaled"""
    dev.call("set_step_params", C.byref(capi.StepParams(**step_params(1))))
    dev.call("set_initial", capi._ptr(np.ascontiguousarray(x0)), capi._ptr(np.ascontiguousarray(y0)))
    dev.call("project_primal")
    dev.call("set_step", 1.0 / dev.init_norms()[0], 1.0)
    dev.call("compute_aty")


def to_cur_1(dev):
    """attempts until the current side is buffer 1 -> the control block"""
    taken = dev.ctl().steps_taken
    for _ in range(16):
        c = dev.attempts(1)
        assert c.error == 0
        if c.cur == 1 and c.steps_taken > taken:
            return c
    raise AssertionError("no accepted attempt left cur == 1")


def dirty(dev, x0, y0):
    """every iterate buffer non-zero, cur == 1"""
    begin(dev, x0, y0)
    dev.attempts(2)
    dist = np.zeros(2)
    dev.call("restart", capi.CURRENT, 0, capi._ptr(dist))
    dev.call("compute_aty")
    c = to_cur_1(dev)
    dev.call("flush_average")
    dev.call("make_average", 2)
    dev.eval(capi.CURRENT)
    dev.eval(capi.AVERAGE)
    assert c.cur == 1 and c.steps_taken >= 1
    for k in ITERATE_BUFFERS:
        assert np.abs(get(dev, k)).max() > 0.0, k


def after_one_attempt(dev, x0, y0):
    begin(dev, x0, y0)
    c = dev.attempts(1)
    return dict(X=get(dev, "X"), Y=get(dev, "Y"), ATY=get(dev, "ATY"), ctl=ar.ctl_dict(c))


@pytest.mark.parametrize("name", ["stream", "panel-rows-4KiB"])
def test_reset(name, monkeypatch):
    p, x0, y0 = fc.edge(name)
    dev = open_variant(name, p, monkeypatch)
    dev.call("set_graph_mode", 1)
    scaled(dev)
    dr, dc = get(dev, "DROW"), get(dev, "DCOL")
    rng = np.random.default_rng(17)
    new = dict(LB=np.where(np.isfinite(p["lb"]), p["lb"] - 0.25, p["lb"]), UB=np.where(np.isfinite(p["ub"]), p["ub"] + rng.random(p["n"]), p["ub"]),
               LO=np.where(np.isfinite(p["lo"]), p["lo"] - rng.random(p["m"]), p["lo"]), HI=np.where(np.isfinite(p["hi"]), p["hi"] + 0.5, p["hi"]))
    scale = dict(LB=lambda v: v / dc, UB=lambda v: v / dc, LO=lambda v: v * dr, HI=lambda v: v * dr)
    for given in (("LB", "UB", "LO", "HI"), ("LB",), ("UB",), ("LO",), ("HI",), ()):
        dirty(dev, x0, y0)
        held = {k: get(dev, k) for k in new}
        # (every call brings bounds the context does not hold yet: the ones before, shifted again)
        fresh = {k: np.where(np.isfinite(new[k]), new[k] + 0.125 * (1 + len(given)), new[k]) for k in given}
        dev.reset(**{k.lower(): fresh.get(k) for k in new})
        for k in ITERATE_BUFFERS:
            assert_bits(get(dev, k), np.zeros(dev.m if k in M_SIZED else dev.n), "%s reset%r %s" % (name, given, k))
        c = ar.ctl_dict(dev.ctl())
        assert all(v == 0 for v in c.values()), (given, c)
        for k in new:
            assert_bits(get(dev, k), scale[k](fresh[k]) if k in given else held[k], "%s reset%r %s" % (name, given, k))
    # bounds array -> uniform -> array: one attempt behind each reset is a fresh context's
    uniform = sc.uniform_bounds_variants(p)["both"]
    for step, q in enumerate((dict(p, lb=new["LB"], ub=new["UB"], lo=p["lo"], hi=p["hi"]), uniform, p)):
        dirty(dev, x0, y0)
        dev.reset(lb=q["lb"], ub=q["ub"], lo=q["lo"], hi=q["hi"])
        got = after_one_attempt(dev, x0, y0)
        other = open_variant(name, q, monkeypatch)
        other.call("set_graph_mode", 1)
        scaled(other)
        want = after_one_attempt(other, x0, y0)
        other.close()
        assert got["ctl"] == want["ctl"] and want["ctl"]["attempts"] == 1, (name, step, got["ctl"], want["ctl"])
        for k in ("X", "Y", "ATY"):
            assert_bits(got[k], want[k], "%s bounds step %d: %s behind one attempt against a fresh context" % (name, step, k))
    dev.close()


# ---- (e) read-back -----------------------------------------------------------------------------------------------------------------------
def check_read_back(dev, dr, dc, tag):
    n, m = dev.n, dev.m
    for which, xn, yn, rn in ((capi.CURRENT, "X", "Y", "RC_CURRENT"), (capi.AVERAGE, "AVG_X", "AVG_Y", "RC_AVERAGE")):
        X, Y, RC = get(dev, xn), get(dev, yn), get(dev, rn)
        x, y, rc = dev.solution(which, n, m)
        ux, uy = fr.unscaled(X, Y, dr, dc)
        assert_bits(x, ux, "%s which=%d x" % (tag, which)) and assert_bits(y, uy, "%s which=%d y" % (tag, which))
        assert_bits(rc, RC, "%s which=%d reduced costs" % (tag, which))
        # NULL outputs are skipped: each output alone is what it was with the others, and a call without any is no error
        for alone in range(3):
            bufs = [np.full(n, 7.0), np.full(m, 7.0), np.full(n, 7.0)]
            ptrs = [capi._ptr(b) if i == alone else None for i, b in enumerate(bufs)]
            dev._ck(capi.lib.pdlpdev_get_solution(dev.handle, which, *ptrs))
            assert_bits(bufs[alone], (x, y, rc)[alone], "%s which=%d output %d alone" % (tag, which, alone))
        dev._ck(capi.lib.pdlpdev_get_solution(dev.handle, which, None, None, None))
        for k, v in ((xn, X), (yn, Y), (rn, RC)):  # (reading changes nothing)
            assert_bits(get(dev, k), v, "%s %s behind the read-back" % (tag, k))


@pytest.mark.parametrize("ctx", ["stream", "wrap"])
def test_read_back(ctx, monkeypatch):
    dev, p, x0, y0 = open_context(ctx, monkeypatch)
    scaled(dev)
    dr, dc = get(dev, "DROW"), get(dev, "DCOL")
    begin(dev, fc.start(p, x0), y0)
    dev.upload("AVG_X", np.ascontiguousarray(get(dev, "X")[::-1]) * 0.5)
    dev.upload("AVG_Y", np.ascontiguousarray(get(dev, "Y")[::-1]) * 0.5)
    dev.eval(capi.CURRENT)
    dev.eval(capi.AVERAGE)
    assert dev.ctl().cur == 0 and np.abs(get(dev, "RC_CURRENT")).max() > 0 and not bits_equal(get(dev, "RC_CURRENT"), get(dev, "RC_AVERAGE"))
    check_read_back(dev, dr, dc, ctx + " cur=0")
    before = get(dev, "X")
    dev.attempts(2)
    c = to_cur_1(dev)
    dev.call("flush_average")
    dev.call("make_average", 2)
    dev.eval(capi.CURRENT)
    dev.eval(capi.AVERAGE)
    assert c.cur == 1 and not bits_equal(get(dev, "X"), before) and not bits_equal(get(dev, "X"), get(dev, "AVG_X"))
    assert not bits_equal(get(dev, "X"), get(dev, "X_OTHER")) and not bits_equal(get(dev, "Y"), get(dev, "Y_OTHER"))
    check_read_back(dev, dr, dc, ctx + " cur=1")
    dev.close()
