"""GPU: what decides every Methodical1 restart and every infeasible / unbounded verdict of the averaging modes -- k_tr_stats, k_tr_pass,
k_tr_final and tr_element behind pdlpdev_trust_region_bounds, k_infeas_rows, k_infeas_cols and compute_remaining_stats behind
pdlpdev_eval_infeasibility (cuopt_amd/csrc/pdlp_eval.hip) -- against the extended-precision reference tests/restart_reference.py, the way
the solver calls them: the CURRENT, AVERAGE and LAST_RESTART slots holding three different vectors, non-zero anchors, cur = 0 and 1, the
own distance and a radius handed in, both reduced-cost rules, scaled iterates in the four SpMV layouts, shapes from 1 x 1 to one whose
grid-stride loops wrap, the resident context filled by pdlpdev_major_eval, and row-block sharded ranks.

Every figure is taken against the reference at the vectors and the products the device holds (downloaded), never against another layout
or the C oracle: error / bound <= 1 with the reference's DERIVED bounds, the two maxima of the infeasibility information bit for bit.
tests/test_restart_reference.py proves the reference, the cases and their branches on the CPU first."""
import numpy as np
import pytest

import eval_reference as er
import restart_cases as rc
import restart_reference as rr
import sharded_ranks as sr
from cuopt_amd import capi
from test_attempt_layouts_gpu import step_params

pytestmark = pytest.mark.gpu
WHICH = dict(CURRENT=capi.CURRENT, AVERAGE=capi.AVERAGE, LAST_RESTART=capi.LAST_RESTART)
BUFS = dict(CURRENT=("X", "Y"), AVERAGE=("AVG_X", "AVG_Y"), LAST_RESTART=("LAST_RESTART_X", "LAST_RESTART_Y"))
BITWISE = ("max_primal_ray_infeasibility", "max_dual_ray_infeasibility")
W0, W1 = rc.WEIGHTS


class Worst(dict):
    def add(self, key, q):
        self[key] = max(self.get(key, 0.0), q)

    def line(self, case):
        return "WORST %s " % case + " ".join("%s=%.3g" % kv for kv in sorted(self.items()))


class Ranks:
    """sharded_ranks.Assembled behind the calls of capi.Device this file makes: a vector goes to every rank (its rows of an m-sized
    one), comes back assembled, and every rank's figures are asserted to be rank 0's bits on the way"""

    def __init__(self, assembled):
        self.a, self.slices = assembled, assembled.slices

    def upload(self, name, values):
        self.a.put(name, values)

    def download(self, name, count):
        return self.a.download(name, count)

    def eval(self, which, rule_finite=True, eps_p=-1.0, eps_d=-1.0):
        return self.a.eval(which, rule_finite, eps_p)

    def eval_infeasibility(self, which, rule_finite=True):
        return self.a.eval_infeasibility(which, rule_finite)

    def trust_region_bounds(self, which, *args, **kw):
        return self.a.trust_region_bounds(which, *args, **kw)

    def close(self):
        self.a.close()


def bits(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


def open_context(p, monkeypatch, scale=True, resident=False, layout=None):
    """-> (context, D_r, D_c); resident: the one-workgroup path a small LP takes by itself, else the multi-launch kernels"""
    if resident:
        monkeypatch.delenv("CUOPT_AMD_SMALL", raising=False)
    else:
        monkeypatch.setenv("CUOPT_AMD_SMALL", "0")
    if layout:
        monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    dev = capi.Device(p)
    lay = dev.layout()
    assert lay["resident"] == resident, lay
    assert layout is None or lay["A"]["layout"] == lay["At"]["layout"] == layout, lay
    if scale:
        dev.call("scaling_compute", 1, 10, 1, 1.0)
        dev.call("scale_problem")
    return dev, dev.download("DROW", p["m"]), dev.download("DCOL", p["n"])


def flip(dev, p, x, y):
    """one accepted attempt: cur = 1, a weight sum and a pending average behind it"""
    dev.call("set_initial", capi._ptr(np.ascontiguousarray(x)), capi._ptr(np.ascontiguousarray(y)))
    dev.call("set_step", 1.0 / dev.init_norms()[0], 1.0)
    dev.call("compute_aty")
    ctl = dev.run(1)
    assert (ctl.error, ctl.steps_taken, ctl.cur) == (0, 1, 1), (ctl.error, ctl.steps_taken, ctl.cur)
    return ctl


def fill(dev, pts, dr, dc, scaled=False, slots=rc.SLOTS):
    """the three different vectors into the three slots: a point is given in the space of the centers, which with scaled iterates is
    the space of the buffers themselves"""
    for slot in slots:
        x, y = pts[slot]
        dev.upload(BUFS[slot][0], x if scaled else rc.to_scaled(x, dc))
        dev.upload(BUFS[slot][1], y if scaled else rc.to_scaled(y, dr))


def held(dev, p, slot):
    return dev.download(BUFS[slot][0], p["n"]), dev.download(BUFS[slot][1], p["m"])


def check_products(dev, p, slot, x, y, tag, worst, again=True):
    """the downloaded products of the slot against (L + 16) u sum |a v| per element -> (ax, aty); again = False: nothing has written
    them since they were last checked"""
    ax, aty = dev.download("AX_U_" + slot, p["m"]), dev.download("ATY_U_" + slot, p["n"])
    if not again:
        return ax, aty
    ref = er.evaluate(p, x, y, eps_p=-1.0, eps_d=-1.0)
    qa, qt = er.worst_ratio(er.abs_err(ref, "ax", ax), ref["bound_ax"]), er.worst_ratio(er.abs_err(ref, "aty", aty), ref["bound_aty_prod"])
    worst.add("ax", qa), worst.add("aty", qt)
    assert np.isfinite(ax).all() and np.isfinite(aty).all(), tag
    assert qa <= 1.0 and qt <= 1.0, dict(case=tag, slot=slot, figure="products", ratio_ax=qa, ratio_aty=qt)
    return ax, aty


def compare(tag, slot, keys, got, ref, worst):
    for k in keys:
        if k in BITWISE:
            assert bits(got[k]) == bits(ref[k]), dict(case=tag, slot=slot, figure=k, got=got[k], want=ref[k], bound="bit for bit")
            continue
        q = rr.ratio(got[k], ref[k], ref["bound"][k])
        worst.add(k, q)
        assert q <= 1.0, dict(case=tag, slot=slot, figure=k, got=got[k], want=ref[k], bound=ref["bound"][k], ratio=q)


def check_infeasibility(dev, p, slot, dr, dc, rule, tag, worst, counts=None):
    """eval(which) fills the products; then the entry point; the reference on the iterate as the device unscales it"""
    dev.eval(WHICH[slot], rule_finite=rule, eps_p=-1.0, eps_d=-1.0)
    xh, yh = held(dev, p, slot)
    x, y = xh * dc, yh * dr
    ax, aty = check_products(dev, p, slot, x, y, tag, worst)
    got = dev.eval_infeasibility(WHICH[slot], rule_finite=rule)
    ref = rr.infeasibility(p, x, y, ax, aty, rule_finite=rule)
    compare("%s rule=%d" % (tag, rule), slot, rr.INFEAS_KEYS, got, ref, worst)
    for k, v in ref["counts"].items():
        if counts is not None:
            counts[(k, rule)] = counts.get((k, rule), 0) + v
    return got


def check_trust_region(dev, p, slot, dr, dc, weights, radius, tag, worst, scaled=False, counts=None, exits=None, evaluate=True):
    """eval(which) fills the products (scaled iterates: the entry point forms its own, downloaded behind the call)"""
    wp, wd, pds, dds, pw = weights
    if evaluate and not scaled:
        dev.eval(WHICH[slot], eps_p=-1.0, eps_d=-1.0)
    xh, yh = held(dev, p, slot)
    lrx, lry = held(dev, p, "LAST_RESTART")
    got = dev.trust_region_bounds(WHICH[slot], wp, wd, pds=pds, dds=dds, primal_weight=pw, radius=radius, scaled_iterates=scaled)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(held(dev, p, slot), (xh, yh))), (tag, slot, "the entry point changed the point")
    x, y = (xh, yh) if scaled else (xh * dc, yh * dr)
    ax, aty = check_products(dev, p, slot, x, y, tag, worst, again=evaluate or scaled)
    ref = rr.trust_region(p, xh, yh, lrx, lry, None if scaled else dr, None if scaled else dc, ax, aty, wp, wd, pds, dds, pw, radius)
    assert ref["assumed_cancellation"]["dual"] <= ref["assumed_cancellation"]["room"], (tag, slot, ref["assumed_cancellation"])
    compare("%s r=%g %s" % (tag, radius, ref["exit"]), slot, rr.TR_KEYS, got, ref, worst)
    if counts is not None:
        for k, v in ref["counts"].items():
            counts[k] = counts.get(k, 0) + v
    if exits is not None:
        exits.add(ref["exit"])
    return got, ref


def solver_sequence(dev, p, dr, dc, weights, tag, worst, scaled=False, counts=None, exits=None):
    """major_head's calls: AVERAGE and CURRENT at their own distances, LAST_RESTART at the candidate's"""
    avg, _ = check_trust_region(dev, p, "AVERAGE", dr, dc, weights, -1.0, tag, worst, scaled, counts=counts, exits=exits)
    cur, _ = check_trust_region(dev, p, "CURRENT", dr, dc, weights, -1.0, tag, worst, scaled, counts=counts, exits=exits)
    assert avg["distance"] > 0.0 and cur["distance"] > 0.0 and avg["distance"] != cur["distance"], (tag, avg, cur)
    ng_avg, ng_cur = (avg["upper_bound"] - avg["lower_bound"]) / avg["distance"], (cur["upper_bound"] - cur["lower_bound"]) / cur["distance"]
    cand = avg if ng_cur / cur["distance"] >= ng_avg / avg["distance"] else cur
    lr, ref = check_trust_region(dev, p, "LAST_RESTART", dr, dc, weights, cand["distance"], tag + " candidate", worst, scaled, counts=counts, exits=exits)
    assert lr["primal_distance2"] == 0.0 and lr["dual_distance2"] == 0.0 and lr["distance"] == 0.0 and ref["radius"] == cand["distance"], (tag, lr)


def assert_reached(name, counts_tr, counts_inf, exits):
    need_tr, need_inf = rc.required(name)
    missing = [k for k in need_tr if not counts_tr.get(k)]
    if counts_inf is not None:
        missing += [(k, r) for k in need_inf for r in (True, False) if not counts_inf.get((k, r))]
    assert not missing, (name, "branches the case is meant to reach", missing)
    assert name == "1x1" or {"T==0", "inside-first", "across"} <= exits, (name, exits)


# ---- a. slots, anchors, cur, radii, rules; the shapes ----------------------------------------------------------------------------------------
def run_shape(name, monkeypatch, resident=False):
    p, pts = rc.shape_lp(name), rc.shape_points(name)
    big = name == "wrap"
    dev, dr, dc = open_context(p, monkeypatch, resident=resident)
    worst, counts_tr, counts_inf, exits = Worst(), {}, {}, set()
    for cur in (0, 1):
        if cur == 1:
            flip(dev, p, *pts["CURRENT"])
        assert dev.ctl().cur == cur
        fill(dev, pts, dr, dc)
        tag = "%s%s cur=%d" % (name, " resident" if resident else "", cur)
        for slot in rc.SLOTS:
            xh, yh = held(dev, p, slot)
            others = [held(dev, p, s) for s in rc.SLOTS if s != slot]
            assert name == "1x1" or all(np.abs(xh - ox).max() > 1e-3 and np.abs(yh - oy).max() > 1e-3 for ox, oy in others), (tag, slot, "three different vectors")
        for slot in ("CURRENT", "AVERAGE"):
            for rule in (True, False):
                check_infeasibility(dev, p, slot, dr, dc, rule, tag, worst, counts_inf)
        solver_sequence(dev, p, dr, dc, W0, tag, worst, counts=counts_tr, exits=exits)
        for radius in (rc.WRAP_RADII[1:] if big else ()):
            check_trust_region(dev, p, "CURRENT", dr, dc, W1, radius, tag, worst, exits=exits, evaluate=False)
        if big:
            check_trust_region(dev, p, "LAST_RESTART", dr, dc, W1, -1.0, tag, worst, exits=exits, evaluate=False)  # (one pass over the half million elements: the wrap does not depend on cur)
            break
        for slot in rc.SLOTS:
            for weights in rc.WEIGHTS:
                for radius in rc.RADII:
                    check_trust_region(dev, p, slot, dr, dc, weights, radius, tag, worst, counts=counts_tr, exits=exits, evaluate=radius == -1.0)
    dev.close()
    print(worst.line(name + ("-resident" if resident else "")))
    print("EXITS %s %s" % (name, sorted(exits)))
    assert_reached(name, counts_tr, counts_inf, exits)


@pytest.mark.parametrize("name", rc.SHAPES)
def test_shapes_slots_and_anchors(name, monkeypatch):
    run_shape(name, monkeypatch)


# ---- b. the resident context ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.SMALL_SHAPES)
def test_resident_context(name, monkeypatch):
    """the small LPs once more on the one-workgroup path; then the slots filled by pdlpdev_major_eval, the way the solver does it"""
    run_shape(name, monkeypatch, resident=True)
    p, pts = rc.shape_lp(name), rc.shape_points(name)
    dev, dr, dc = open_context(p, monkeypatch, resident=True)
    ctl = flip(dev, p, *pts["CURRENT"])
    fill(dev, pts, dr, dc, slots=("CURRENT", "LAST_RESTART"))
    ax, ay = pts["AVERAGE"]
    dev.upload("SUM_X", rc.to_scaled(ax, dc) * ctl.sum_weights)
    dev.upload("SUM_Y", rc.to_scaled(ay, dr) * ctl.sum_weights)
    worst, tag = Worst(), "%s resident major_eval" % name
    for rule in (True, False):
        dev.major_eval(2, rule_finite=rule)
        (xc, yc), (xa, ya) = held(dev, p, "CURRENT"), held(dev, p, "AVERAGE")
        assert name == "1x1" or (np.abs(xc - xa).max() > 1e-3 and np.abs(yc - ya).max() > 1e-3), tag
        assert np.isfinite(xa).all() and np.isfinite(ya).all(), tag
        for slot, (xh, yh) in (("CURRENT", (xc, yc)), ("AVERAGE", (xa, ya))):
            x, y = xh * dc, yh * dr
            pax, paty = check_products(dev, p, slot, x, y, tag, worst)
            got = dev.eval_infeasibility(WHICH[slot], rule_finite=rule)
            compare("%s rule=%d" % (tag, rule), slot, rr.INFEAS_KEYS, got, rr.infeasibility(p, x, y, pax, paty, rule_finite=rule), worst)
            check_trust_region(dev, p, slot, dr, dc, W0, -1.0, tag, worst, evaluate=False)
            check_trust_region(dev, p, slot, dr, dc, W1, 0.5, tag, worst, evaluate=False)
    dev.close()
    print(worst.line(name + "-resident-major-eval"))


# ---- c. scaled iterates in the four layouts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["stream", "panel", "jag", "pb"])
def test_scaled_iterates_in_the_layouts(layout, monkeypatch):
    """scaled_iterates = 1: the scaled vectors meet the unscaled problem, and the entry point forms its own products
    D_r^-1 (A^ (D_c^-1 v)) with the layout's plain kernels; they are downloaded, checked per element, then handed to the reference"""
    name = "37x53"
    p, pts = rc.shape_lp(name), rc.shape_points(name)
    dev, dr, dc = open_context(p, monkeypatch, layout=layout)
    assert np.abs(dr - 1.0).max() > 1e-3 and np.abs(dc - 1.0).max() > 1e-3
    worst, counts, exits = Worst(), {}, set()
    for cur in (0, 1):
        if cur == 1:
            flip(dev, p, *pts["CURRENT"])
        fill(dev, pts, dr, dc, scaled=True)
        tag = "scaled %s cur=%d" % (layout, cur)
        solver_sequence(dev, p, dr, dc, W0, tag, worst, scaled=True, exits=exits)
        for slot in rc.SLOTS:
            for radius in rc.RADII:
                check_trust_region(dev, p, slot, dr, dc, W1, radius, tag, worst, scaled=True, counts=counts, exits=exits)
    dev.close()
    print(worst.line("scaled-" + layout))
    assert_reached(name, counts, None, exits)


# ---- d. sharded ranks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,flow,name", [(2, "allreduce", "300x257"), (3, "allreduce", "300x257"), (8, "rsag", "300x257")],
                         ids=["world2", "world3", "world8-empty-slices"])
def test_sharded_ranks(world, flow, name, monkeypatch):
    """W ranks behind the in-process communicator on one device (tests/sharded_ranks.py): rank 0 counts the primal coordinates, every
    rank its rows (first = n), three all-reduces per pass, the maxima apart from the sums.  Every rank returns the same bits
    (Assembled asserts it) and they are inside the reference's bounds for the WHOLE LP: the bounds hold for any summation tree, the
    communicator's over the ranks included, so there is no further tolerance."""
    p, pts = rc.shape_lp(name), rc.shape_points(name)
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")
    monkeypatch.setenv("CUOPT_AMD_SHARD_DATAFLOW", flow)
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    dev = Ranks(sr.on_device(p, pts["CURRENT"][0], pts["CURRENT"][1], step_params(1), world, flow))
    try:
        if flow != "allreduce":
            assert [s[1] for s in dev.slices][-2:] == [0, 0], dev.slices
        dr, dc = dev.download("DROW", p["m"]), dev.download("DCOL", p["n"])
        fill(dev, pts, dr, dc)
        worst, counts_tr, counts_inf, exits, tag = Worst(), {}, {}, set(), "sharded world %d" % world
        for slot in ("CURRENT", "AVERAGE"):
            for rule in (True, False):
                check_infeasibility(dev, p, slot, dr, dc, rule, tag, worst, counts_inf)
        solver_sequence(dev, p, dr, dc, W0, tag, worst, exits=exits)
        for slot in rc.SLOTS:
            for radius in rc.RADII:
                check_trust_region(dev, p, slot, dr, dc, W1, radius, tag, worst, counts=counts_tr, exits=exits, evaluate=radius == -1.0)
        if world == 2:
            fill(dev, pts, dr, dc, scaled=True)
            solver_sequence(dev, p, dr, dc, W0, tag + " scaled", worst, scaled=True)
    finally:
        dev.close()
    print(worst.line("sharded-world%d" % world))
    assert_reached(name, counts_tr, counts_inf, exits)


# ---- e. the degenerate exits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [False, True], ids=["unscaled", "scaled"])
def test_point_on_its_anchor(scale, monkeypatch):
    """T = 0 (radius -1 at the anchor itself): t = 0, nothing moves, both bounds ARE the Lagrangian, bit for bit.  Behind the scaling a
    column sitting on a bound that fl(xhat D_c) misses by a rounding (no xhat need give 1.5 on a fixed column) is outside its bounds as
    tr_element sees it, and k_tr_final clamps it back even at t = 0; the reference does the same.  So the lower bound is the
    Lagrangian's bits on the unscaled context, and on the scaled one whenever no column is outside; the upper bound always (a dual
    bound is 0 or infinite, and yhat D_r keeps a zero and a sign)."""
    p, pts = rc.shape_lp("37x53"), rc.shape_points("37x53")
    dev, dr, dc = open_context(p, monkeypatch, scale=scale)
    assert scale or ((dr == 1.0).all() and (dc == 1.0).all())
    worst = Worst()
    fill(dev, dict(pts, LAST_RESTART=pts["CURRENT"]), dr, dc)
    x = held(dev, p, "CURRENT")[0] * dc
    inside = bool(np.all(x >= p["lb"]) and np.all(x <= p["ub"]))
    assert scale or inside
    for slot in ("CURRENT", "LAST_RESTART"):
        got, ref = check_trust_region(dev, p, slot, dr, dc, W0, -1.0, "T==0 scale=%d" % scale, worst)
        assert ref["exit"] == "T==0" and got["distance"] == 0.0, (slot, ref["exit"], got)
        assert bits(got["upper_bound"]) == bits(got["lagrangian"]), (slot, got)
        assert not inside or bits(got["lower_bound"]) == bits(got["lagrangian"]), (slot, got)
    dev.close()
    print(worst.line("T==0-scale%d" % scale) + " inside=%d" % inside)


def test_objective_vector_is_zero(monkeypatch):
    """c = A^T y and every row satisfied, exactly (small integers, no scaling): ||objective|| = 0, t = 0 whatever the radius"""
    p, x, y = rc.integer_lp()
    dev, dr, dc = open_context(p, monkeypatch, scale=False)
    assert (dr == 1.0).all() and (dc == 1.0).all()
    dev.upload("X", x), dev.upload("Y", y)
    worst = Worst()
    for radius in (-1.0, 3.0):
        got, ref = check_trust_region(dev, p, "CURRENT", dr, dc, W0, radius, "obj==0", worst)
        assert ref["exit"] == "obj==0" and ref["t"] == 0.0 and got["distance"] > 0.0, (ref["exit"], got)
        assert bits(got["lower_bound"]) == bits(got["lagrangian"]) == bits(got["upper_bound"]), got
    dev.close()
    print(worst.line("obj==0"))


def test_radius_beyond_every_breakpoint(monkeypatch):
    """every moving element has a finite threshold and the radius lies beyond all of them: high(t) runs out, t = the largest threshold"""
    p, x, y = rc.all_finite_lp()
    dev, dr, dc = open_context(p, monkeypatch)
    dev.upload("X", rc.to_scaled(x, dc)), dev.upload("Y", rc.to_scaled(y, dr))
    worst = Worst()
    for radius in (1e6, 1e9, 3.0):
        got, ref = check_trust_region(dev, p, "CURRENT", dr, dc, W0, radius, "beyond-all", worst)
        c = ref["counts"]
        assert c["moving"] > 10 and c["moving_forever"] == 0, c
        assert ref["exit"] == ("across" if radius == 3.0 else "beyond-all"), (radius, ref["exit"])
    dev.close()
    print(worst.line("beyond-all"))


def test_last_restart_products_are_download_only(monkeypatch):
    p = rc.shape_lp("37x53")
    dev, dr, dc = open_context(p, monkeypatch)
    assert len(dev.download("AX_U_LAST_RESTART", p["m"])) == p["m"] and len(dev.download("ATY_U_LAST_RESTART", p["n"])) == p["n"]
    for name, count in (("AX_U_LAST_RESTART", p["m"]), ("ATY_U_LAST_RESTART", p["n"])):
        with pytest.raises(capi.CuOptError):
            dev.upload(name, np.zeros(count))
    dev.close()
