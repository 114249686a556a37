"""CPU: tests/restart_reference.py is tested before it is believed -- against the C oracle on the LPs of the two kernel-level GPU tests,
against an independent bisection, against a float64 re-enactment of the device's passes on every case of
tests/test_restart_inputs_gpu.py (which must stay inside the reference's bounds), and for the branches each case is meant to reach."""
import numpy as np
import pytest

import restart_cases as rc
import restart_reference as rr
from cuopt_amd import synthetic
from oracle import orcbind

INF = np.inf


def products(p, x, y):
    """float64 products, rows left to right (the oracle's)"""
    to, ti, tv = orcbind.transpose(p["m"], p["n"], p["offsets"], p["indices"], p["values"])
    return orcbind.spmv(p["offsets"], p["indices"], p["values"], x), orcbind.spmv(to, ti, tv, y)


def infeasible_lp():
    from test_solve_gpu import infeasible_lp_of_the_c_api_test
    return infeasible_lp_of_the_c_api_test()


# ---- the float64 re-enactment of the device ------------------------------------------------------------------------------------------------
def reenact_trust_region(p, xhat, yhat, lrx, lry, dr, dc, ax, aty, wp, wd, pds, dds, pw, radius):
    """pdlpdev_trust_region_bounds in float64: tr_element's elements, numpy's sums for the workgroups' trees, the host loop's fixed point"""
    if dc is None:
        x, y, dx, dy = xhat, yhat, lrx - xhat, lry - yhat
    else:
        x, y, dx, dy = xhat * dc, yhat * dr, (lrx - xhat) * dc, (lry - yhat) * dr
    e = rr.elements(p, x, y, ax, aty, wp, wd)
    n, center, d, thr, w, lb, ub, grad = e["n"], e["center"], e["dir"], e["thr"], e["w"], e["lb"], e["ub"], e["grad"]
    pd2, dd2 = float(np.sum(dx * dx)), float(np.sum(dy * dy))
    st2, st3 = float(np.sum(p["c"] * x)), float(np.sum(x * aty))
    st4 = float(np.sum(np.where(y == 0.0, 0.0, y * np.where(y == 0.0, 0.0, e["sub"]))))
    st5, st6 = float(np.sum(e["obj"] * e["obj"])), float(np.sum(w * d * d))
    fin = np.isfinite(thr)
    st7 = float(thr[fin].max()) if fin.any() else 0.0
    own = np.sqrt(pd2 * pds * pw + dd2 * (dds / pw))
    T = radius if radius >= 0.0 else own
    lag = (st2 - st3) + st4
    t, mv = 0.0, d != 0.0

    def moved(t):
        with np.errstate(invalid="ignore"):
            return np.where(mv, np.minimum(np.maximum(center + t * d, lb), ub) - center, 0.0)
    if not (T == 0.0 or np.sqrt(st5) == 0.0):
        t = T / np.sqrt(st6) if st6 > 0.0 else 0.0
        for _ in range(200):
            at = mv & (thr <= t)
            step = moved(t)
            low, high = float(np.sum((step * step * w)[at])), float(np.sum((d * d * w)[mv & ~at]))
            if high <= 0.0:
                t = st7
                break
            rem = T * T - low
            tn = np.sqrt(rem / high) if rem > 0.0 else t
            if not tn > t:
                break
            t = tn
    fs = moved(t) * np.where(mv, grad, 0.0)
    return dict(primal_distance2=pd2, dual_distance2=dd2, distance=float(own), lagrangian=lag, lower_bound=lag + float(np.sum(fs[:n])),
                upper_bound=lag + float(np.sum(fs[n:])))


def reenact_infeasibility(p, x, y, ax, aty, rule_finite):
    lo, hi, lb, ub = p["lo"], p["hi"], p["lb"], p["ub"]
    hl, hu = np.where(np.isfinite(lo), 0.0, lo), np.where(np.isfinite(hi), 0.0, hi)
    viol = np.where(ax < hl, hl - ax, np.where(ax > hu, ax - hu, 0.0))

    def bvp(v, lower, upper):
        b = np.where(v > 0.0, lower, np.where(v < 0.0, upper, 0.0))
        with np.errstate(invalid="ignore"):
            return np.where(np.isfinite(b), v * np.where(np.isfinite(b), b, 0.0), 0.0)
    r = [float(np.abs(viol).max()), float(np.abs(y).max()), float(np.sum(bvp(y, lo, hi)))]
    g = -1.0 * aty
    bv = np.where(g > 0.0, lb, ub)
    with np.errstate(invalid="ignore"):
        take = np.isfinite(bv) if rule_finite else np.abs(x - bv) <= np.abs(x)
    red = np.where(g == 0.0, g, np.where(take, g, 0.0))
    v = np.maximum(np.where(np.isfinite(lb), -x, 0.0), np.where(np.isfinite(ub), x, 0.0))
    c = [float(np.abs(g - red).max()), float(np.abs(red).max()), float(np.abs(x).max()), float(np.maximum(v, 0.0).max()),
         float(np.sum(bvp(red, lb, ub))), float(np.sum(p["c"] * x))]
    max_primal, primal_obj = r[0], 0.0 if c[2] == 0.0 else c[5] * (1.0 / c[2])
    max_dual, dual_obj = c[0], r[2] + c[4]
    scaling = max(r[1], c[1])
    max_dual, dual_obj = (max_dual / scaling, dual_obj / scaling) if scaling != 0.0 else (0.0, 0.0)
    max_primal, primal_obj = (max(max_primal, c[3]) / c[2], primal_obj) if c[2] > 0.0 else (0.0, 0.0)
    return dict(zip(rr.INFEAS_KEYS, (max_primal, primal_obj, max_dual, dual_obj)))


def check_tr(tag, got, ref, worst):
    assert ref["assumed_cancellation"]["dual"] <= ref["assumed_cancellation"]["room"], (tag, ref["assumed_cancellation"])
    for k in rr.TR_KEYS:
        q = rr.ratio(got[k], ref[k], ref["bound"][k])
        worst[k] = max(worst.get(k, 0.0), q)
        assert q <= 1.0, dict(case=tag, figure=k, got=got[k], want=ref[k], bound=ref["bound"][k], ratio=q, exit=ref["exit"])


def check_infeas(tag, got, ref, worst):
    for k in ("max_primal_ray_infeasibility", "max_dual_ray_infeasibility"):
        assert got[k] == ref[k], dict(case=tag, figure=k, got=got[k], want=ref[k])
    for k in ("primal_ray_linear_objective", "dual_ray_linear_objective"):
        q = rr.ratio(got[k], ref[k], ref["bound"][k])
        worst[k] = max(worst.get(k, 0.0), q)
        assert q <= 1.0, dict(case=tag, figure=k, got=got[k], want=ref[k], bound=ref["bound"][k], ratio=q)


# ---- 1. the oracle ---------------------------------------------------------------------------------------------------------------------------
def test_infeasibility_agrees_with_the_oracle():
    """the LPs and vectors of test_solve_gpu.test_infeasibility_information_matches_oracle, at its tolerances"""
    for p in (synthetic.generate(3000, 2500, 8, seed=41), infeasible_lp()):
        rng = np.random.default_rng(7)
        x = np.abs(rng.standard_normal(p["n"])) * (rng.random(p["n"]) < 0.8)
        y = rng.standard_normal(p["m"])
        ax, aty = products(p, x, y)
        for rule in (True, False):
            got = rr.infeasibility(p, x, y, ax, aty, rule_finite=rule)
            ref = orcbind.evaluate_infeasibility(p, x, y, finite_bounds_rule=rule)
            for k in ref:
                assert got[k] == pytest.approx(ref[k], rel=1e-10, abs=1e-12), (k, rule)


def test_trust_region_agrees_with_the_oracle(golden_problems):
    """the LPs, vectors, weights and radii of test_solve_gpu.test_trust_region_bounds_match_oracle, at its tolerances"""
    for p in (synthetic.generate(2500, 2000, 8, seed=51), golden_problems["afiro"]["problem"]):
        rng = np.random.default_rng(9)
        x = np.abs(rng.standard_normal(p["n"])) * (rng.random(p["n"]) < 0.7)
        y = rng.standard_normal(p["m"])
        y = np.where(np.isinf(p["lo"]), -np.abs(y), y)
        y = np.where(np.isinf(p["hi"]), np.abs(y), y) * (rng.random(p["m"]) < 0.8)
        ax, aty = products(p, x, y)
        zx, zy = np.zeros(p["n"]), np.zeros(p["m"])
        exits = set()
        for wp, wd, radius in ((2.0, 0.7, 1e-3), (2.0, 0.7, 0.5), (0.3, 5.0, 10.0), (1.0, 1.0, 1e4)):
            got = rr.trust_region(p, x, y, zx, zy, None, None, ax, aty, wp, wd, radius=radius)
            ref = orcbind.trust_region_bounds(p, x, y, wp, wd, radius)
            scale = 1.0 + abs(ref["lagrangian"])
            exits.add(got["exit"])
            assert got["lagrangian"] == pytest.approx(ref["lagrangian"], rel=1e-10, abs=1e-10 * scale)
            assert got["lower_bound"] == pytest.approx(ref["lower_bound"], rel=1e-9, abs=1e-9 * scale), (wp, wd, radius)
            assert got["upper_bound"] == pytest.approx(ref["upper_bound"], rel=1e-9, abs=1e-9 * scale), (wp, wd, radius)
        assert "across" in exits, exits
        got = rr.trust_region(p, x, y, zx, zy, None, None, ax, aty, 1.0, 1.0, pds=0.5, dds=0.5, primal_weight=2.0)
        assert got["primal_distance2"] == pytest.approx(float(x @ x), rel=1e-12)
        assert got["dual_distance2"] == pytest.approx(float(y @ y), rel=1e-12)
        assert got["distance"] == pytest.approx(np.sqrt(x @ x * 0.5 * 2.0 + y @ y * 0.5 / 2.0), rel=1e-12)


# ---- 2. an independent solution --------------------------------------------------------------------------------------------------------------
def test_trust_region_against_an_independent_bisection():
    """the plain bisection on the step length of test_oracle_golden.test_trust_region_bounds_against_an_independent_solution (no sort, no
    breakpoints, float64), its LPs, points, weights and radii, its tolerances"""
    rng = np.random.default_rng(5)
    for seed in (1, 2, 3):
        p = synthetic.generate(400, 300, 6, seed=seed)
        p["ub"] = np.where(rng.random(p["n"]) < 0.5, 1.5, np.inf)
        x = np.clip(np.abs(rng.standard_normal(p["n"])) * (rng.random(p["n"]) < 0.7), p["lb"], p["ub"])
        y = rng.standard_normal(p["m"])
        y = np.where(np.isinf(p["lo"]), -np.abs(y), y)
        y = np.where(np.isinf(p["hi"]), np.abs(y), y) * (rng.random(p["m"]) < 0.8)
        ax, aty = products(p, x, y)
        exits = set()
        for wp, wd, radius in ((2.0, 0.7, 1e-3), (2.0, 0.7, 0.5), (0.3, 5.0, 10.0), (1.0, 1.0, 1e4)):
            e = rr.elements(p, x, y, ax, aty, wp, wd)
            center, w, low, upp = e["center"], e["w"], e["lb"], e["ub"]
            direction = np.where(e["dir"] != 0.0, -e["obj"] / w, 0.0)
            lagrangian = p["c"] @ x - x @ aty + y @ np.where(y == 0.0, 0.0, e["sub"])

            def moved(t):
                with np.errstate(invalid="ignore"):
                    z = np.clip(center + t * direction, low, upp)
                return np.where(direction == 0.0, 0.0, z - center)

            def radius2(t):
                d = moved(t)
                return float(np.sum(w * d * d))
            t_hi, t_lo = 1.0, 0.0
            while radius2(t_hi) < radius * radius and t_hi < 1e30:
                t_hi *= 4.0
            if radius2(t_hi) >= radius * radius:
                for _ in range(200):
                    mid = 0.5 * (t_lo + t_hi)
                    t_lo, t_hi = (t_lo, mid) if radius2(mid) >= radius * radius else (mid, t_hi)
            d = moved(t_hi)
            lower, upper = lagrangian + float(d[:p["n"]] @ e["grad"][:p["n"]]), lagrangian + float(d[p["n"]:] @ e["grad"][p["n"]:])
            got = rr.trust_region(p, x, y, np.zeros(p["n"]), np.zeros(p["m"]), None, None, ax, aty, wp, wd, radius=radius)
            exits.add(got["exit"])
            scale = 1.0 + abs(lagrangian)
            assert got["lagrangian"] == pytest.approx(lagrangian, rel=1e-12, abs=1e-12 * scale)
            assert got["lower_bound"] == pytest.approx(lower, rel=1e-8, abs=1e-8 * scale), (seed, wp, wd, radius, got["exit"])
            assert got["upper_bound"] == pytest.approx(upper, rel=1e-8, abs=1e-8 * scale), (seed, wp, wd, radius, got["exit"])
        assert {"inside-first", "across"} <= exits, exits


# ---- 3. the re-enactment inside the bounds, 4. the branches, on the cases of the GPU test ----------------------------------------------------------
def host_slots(name, scaled):
    """the three slots as a context would hold them (synthetic scalings), with float64 products -> (p, {slot: (xhat, yhat, x, y, ax, aty)}, dr, dc)"""
    p, pts = rc.shape_lp(name), rc.shape_points(name)
    rng = np.random.default_rng(3)
    dr, dc = (None, None) if scaled else (rng.uniform(0.25, 4.0, p["m"]), rng.uniform(0.25, 4.0, p["n"]))
    out = {}
    for slot, (x, y) in pts.items():
        xh, yh = (x, y) if scaled else (rc.to_scaled(x, dc), rc.to_scaled(y, dr))
        xu, yu = (xh, yh) if scaled else (xh * dc, yh * dr)
        out[slot] = (xh, yh, xu, yu) + products(p, xu, yu)
    return p, out, dr, dc


@pytest.mark.parametrize("name,scaled", [(n, s) for n in rc.SHAPES for s in (False, True) if not (n == "wrap" and s)])  # (as the GPU test)
def test_reenactment_stays_inside_the_bounds_on_the_shapes(name, scaled):
    p, slots, dr, dc = host_slots(name, scaled)
    big = name == "wrap"
    need_tr, need_inf = rc.required(name)
    lrx, lry = slots["LAST_RESTART"][:2]
    worst, exits, seen_tr, seen_inf = {}, set(), {}, {}
    for slot, (xh, yh, x, y, ax, aty) in slots.items():
        for wi, (wp, wd, pds, dds, pw) in enumerate(rc.WEIGHTS[:1] if big else rc.WEIGHTS):
            for radius in (rc.WRAP_RADII if big else rc.RADII):
                if big and slot != "CURRENT" and radius != -1.0:  # (the GPU test's calls on the half million elements)
                    continue
                args =(p, xh, yh, lrx, lry, dr, dc, ax, aty, wp, wd, pds, dds, pw, radius)
                ref = rr.trust_region(*args)
                check_tr("%s %s w%d r=%g" % (name, slot, wi, radius), reenact_trust_region(*args), ref, worst)
                exits.add(ref["exit"])
                for k, v in ref["counts"].items():
                    seen_tr[k] = seen_tr.get(k, 0) + v
        for rule in (True, False):
            ref = rr.infeasibility(p, x, y, ax, aty, rule_finite=rule)
            check_infeas("%s %s rule=%d" % (name, slot, rule), reenact_infeasibility(p, x, y, ax, aty, rule), ref, worst)
            for k, v in ref["counts"].items():
                seen_inf[(k, rule)] = seen_inf.get((k, rule), 0) + v
    print("WORST %s scaled=%d %s" % (name, scaled, " ".join("%s=%.3f" % kv for kv in sorted(worst.items()))))
    print("EXITS %s %s" % (name, sorted(exits)))
    missing = [k for k in need_tr if not seen_tr.get(k)] + [(k, r) for k in need_inf for r in (True, False) if not seen_inf.get((k, r))]
    assert not missing, (name, missing)
    if name != "1x1":
        assert {"T==0", "inside-first", "across"} <= exits, exits  # (LAST_RESTART against itself at radius -1 is T == 0)
    else:
        assert "T==0" in exits, exits


def degenerate(kind):
    """-> (p, x, y, anchors, radius, the exit it must take)"""
    if kind == "T==0":
        p = rc.shape_lp("37x53")
        x, y = rc.shape_points("37x53")["CURRENT"]
        return p, x, y, (x, y), -1.0, "T==0"
    if kind == "obj==0":
        p, x, y = rc.integer_lp()
        return p, x, y, (np.zeros(p["n"]), np.zeros(p["m"])), 3.0, "obj==0"
    p, x, y = rc.all_finite_lp()
    return p, x, y, (np.zeros(p["n"]), np.zeros(p["m"])), 1e6, "beyond-all"


@pytest.mark.parametrize("kind", ["T==0", "obj==0", "beyond-all"])
def test_degenerate_exits(kind):
    p, x, y, (lrx, lry), radius, want = degenerate(kind)
    ax, aty = products(p, x, y)
    args = (p, x, y, lrx, lry, None, None, ax, aty, 2.0, 0.7, 0.5, 0.5, 1.5, radius)
    ref, got = rr.trust_region(*args), reenact_trust_region(*args)
    assert ref["exit"] == want, ref["exit"]
    check_tr(kind, got, ref, {})
    if kind != "beyond-all":  # t = 0: nothing moves, both bounds ARE the Lagrangian
        assert ref["t"] == 0.0 and ref["lower_bound"] == ref["upper_bound"] == ref["lagrangian"]
        assert got["lower_bound"] == got["upper_bound"] == got["lagrangian"]
    else:
        c = ref["counts"]
        assert c["moving"] > 10 and c["moving_forever"] == 0 and c["at_bounds"] == c["moving"] == c["finite_thresholds"], c
        again = rr.trust_region(*args[:-1], 1e9)  # (beyond all of them the radius no longer matters)
        assert (again["lower_bound"], again["upper_bound"]) == (ref["lower_bound"], ref["upper_bound"])
    if kind == "obj==0":
        assert not np.any(rr.elements(p, x, y, ax, aty, 2.0, 0.7)["obj"] != 0.0) and np.abs(y).max() > 0 and np.abs(p["c"]).max() > 0


def test_a_broken_branch_leaves_the_bounds():
    """what the GPU test is for, on the host: the re-enactment with lo and hi swapped in the y == 0 subgradient, and with the first
    workgroup's share of the primal elements dropped, is outside the bounds"""
    p, slots, dr, dc = host_slots("300x257", False)
    xh, yh, x, y, ax, aty = slots["CURRENT"]
    lrx, lry = slots["LAST_RESTART"][:2]
    args = (p, xh, yh, lrx, lry, dr, dc, ax, aty, 2.0, 0.7, 0.5, 0.5, 1.5, 0.5)
    ref = rr.trust_region(*args)
    q = dict(p, lo=np.where((y == 0.0) & np.isfinite(p["lo"]) & np.isinf(p["hi"]), -INF, p["lo"]),
             hi=np.where((y == 0.0) & np.isfinite(p["lo"]) & np.isinf(p["hi"]), p["lo"], p["hi"]))
    swapped = reenact_trust_region(q, *args[1:])
    assert max(rr.ratio(swapped[k], ref[k], ref["bound"][k]) for k in ("lower_bound", "upper_bound")) > 1.0
    xs = xh.copy()
    xs[:8] = lrx[:8]
    dropped = reenact_trust_region(p, xs, *args[2:])
    assert rr.ratio(dropped["primal_distance2"], ref["primal_distance2"], ref["bound"]["primal_distance2"]) > 1.0


def test_exact_rationals_agree_with_long_double():
    p, slots, dr, dc = host_slots("37x53", False)
    xh, yh, x, y, ax, aty = slots["AVERAGE"]
    lrx, lry = slots["LAST_RESTART"][:2]
    for radius in (-1.0, 0.5, 1e7):
        a = rr.trust_region(p, xh, yh, lrx, lry, dr, dc, ax, aty, 2.0, 0.7, 0.5, 0.5, 1.5, radius, exact=True)
        b = rr.trust_region(p, xh, yh, lrx, lry, dr, dc, ax, aty, 2.0, 0.7, 0.5, 0.5, 1.5, radius, exact=False)
        assert a["exit"] == b["exit"]
        for k in rr.TR_KEYS:
            assert rr.ratio(a[k], b[k], a["bound"][k]) <= 1.0 / 64, (k, a[k], b[k])
            assert a["bound"][k] == pytest.approx(b["bound"][k], rel=1e-4), k  # (the spread is a difference of two long doubles 1e-13 apart)
    a, b = (rr.infeasibility(p, x, y, ax, aty, exact=e) for e in (True, False))
    for k in rr.INFEAS_KEYS:
        assert a[k] == pytest.approx(b[k], rel=1e-15), k
