"""CPU: the restatement of one adaptive PDHG attempt (tests/attempt_reference.py) against numbers worked out by hand and against the C
oracle, and the scenario of tests/test_attempt_layouts_gpu.py (tests/attempt_scenario.py) on a plain float64 stand-in for the device,
on every LP and seed the GPU test uses: the stand-in stays inside every derived bound, and the scenario has the properties the GPU
test relies on (accepted steps from both sides of the ping-pong pairs, attempts with and without a pending average, a forced rejection
with step / limit >= 2, no natural decision within 1e-6 of a tie).  The last section runs the same scenario on W stand-in RANKS behind
the assembly of tests/sharded_ranks.py, for the cases of tests/test_sharded_attempts_gpu.py: the assembly reads no stale entry (whatever
a rank does not own is NaN there) and the LPs keep the scenario's properties in the sharded order of summation."""
import numpy as np
import pytest

import attempt_reference as ar
import attempt_scenario as sc
import eval_reference as er
from cuopt_amd import synthetic
import resident_lps as rl
import sharded_ranks as sr
from eval_lps import SEEDS, WIDE_N, edge_lp
from oracle import orcbind

INF = np.inf
# (long_col, dense, seed[, columns]): what the GPU test builds
LPS = [(4500, False, SEEDS[0]), (2400, False, SEEDS[0]), (4500, True, SEEDS[1]), (2400, True, SEEDS[1]), (2400, False, SEEDS[0], WIDE_N)]
LP_IDS = ["col4500", "col2400", "dense-col4500", "dense-col2400", "col2400-60000-columns"]
SP_EXACT = dict(reduction_exponent=1.0, growth_exponent=2.0, primal_distance_smoothing=0.5, dual_distance_smoothing=0.5)  # (k + 2)^-1, ^-2: exact


def step_params(mode=1):
    h, H = orcbind.hyper_preset(mode), orcbind.H
    return {k: float(h[H["ORC_H_" + k.upper()]]) for k in ("reduction_exponent", "growth_exponent", "primal_distance_smoothing", "dual_distance_smoothing")}


def scaling_of(p):
    """Ruiz 10 + Pock-Chambolle alpha 1: what pdlpdev_scaling_compute(1, 10, 1, 1.0) gives (test_kernels_gpu: bit for bit)"""
    h, H = orcbind.hyper_preset(1), orcbind.H
    h[H["ORC_H_DO_RUIZ"]], h[H["ORC_H_RUIZ_ITERATIONS"]], h[H["ORC_H_DO_POCK_CHAMBOLLE"]], h[H["ORC_H_ALPHA_POCK_CHAMBOLLE"]] = 1, 10, 1, 1.0
    return orcbind.compute_scaling(p["m"], p["n"], p["offsets"], p["indices"], p["values"], h)


def ctl_of(**over):
    c = dict(step_size=0.0, primal_weight=1.0, tau=0.0, sigma=0.0, sum_weights=0.0, last_interaction=0.0, last_movement=0.0, last_dx2=0.0,
             last_dy2=0.0, k=0, cur=0, pending_avg=0, steps_taken=0, attempts=0, target_steps=1 << 30, error=0, its_since_restart=0)
    c.update(over)
    return c


def arrays(**kw):
    return {k: np.array(v, dtype=np.float64) for k, v in kw.items()}


def stages(S, prob, ctl, st, sp, exact):
    """the attempt stage by stage, each from the reference's own output of the stage in front -> (x', xbar, y', A^T y', sums, decision)"""
    p = ar.primal(prob, ctl, st)
    d = ar.dual(S, prob, ctl, st, p["xbar"], exact)
    a = ar.aty_product(S, prob, d["y"], exact)
    s = ar.step_sums(st, p["xn"], d["y"], a["aty"], exact)
    dec = ar.decision(ctl, float(s["dy2"][0]), float(s["inter"][0]), float(s["dx2"][0]), sp)
    return p, d, a, s, dec


@pytest.mark.parametrize("exact", [False, True], ids=["longdouble", "fractions"])
def test_accepted_attempt_by_hand(exact):
    """A = [1 2; 0 1], c = (-1, -2), 0 <= x, x_1 <= 1, row 0: <= 1, row 1: = 2; from x = y = 0 with step 1/2 at weight 2
    (tau = 1/4, sigma = 1).  Every number is a dyadic rational except the limit 9/11.
       x' = (1/4, 1/2), xbar = (1/2, 1), A xbar = (5/2, 1)
       row 0: next = -5/2, up = -3/2 < 0, low = -inf: y' = -3/2          row 1: next = -1, low = up = 1, min(up, 0) = 0: y' = 1
       A^T y' = (-3/2, -2); dx = (1/4, 1/2), dy = (-3/2, 1): dx2 = 5/16, dy2 = 13/4, interaction = -3/8 - 1 = -11/8
       movement = (1/2) 2 (5/16) + (1/4) (13/4) = 9/8, limit = 9/11 >= 1/2: accepted, margin 11/18
       k = 1: s1 = (1 - 1/2) 9/11, s2 = (1 + 1/4) 1/2 = 5/8: the new step is s1"""
    exact = exact or not er.LONGDOUBLE_IS_EXTENDED
    S = ar.Structure(2, 2, [0, 2, 3], [0, 1, 1])
    prob = arrays(A_VALUES=[1, 2, 1], C=[-1, -2], LB=[0, 0], UB=[INF, 1], LO=[-INF, 2], HI=[1, 2])
    st = arrays(X=[0, 0], Y=[0, 0], ATY=[0, 0], SUM_X=[1, 1], SUM_Y=[2, 2])
    ctl = ctl_of(step_size=0.5, primal_weight=2.0, tau=0.25, sigma=1.0)
    p, d, a, s, dec = stages(S, prob, ctl, st, SP_EXACT, exact)
    np.testing.assert_array_equal(p["xn"], [0.25, 0.5])
    np.testing.assert_array_equal(p["xbar"], [0.5, 1.0])
    np.testing.assert_array_equal(p["sumx"], [1, 1])  # (nothing pending: untouched)
    np.testing.assert_array_equal(d["y"], [-1.5, 1.0])
    np.testing.assert_array_equal(d["sumy"], [2, 2])
    assert not d["branch_tie"].any()
    # bounds: sigma (L + 16) u S + 8 u (|y| + sigma |v| + sigma |b|), S = |v| = (5/2, 1), b = (1, 2), L = (2, 1)
    np.testing.assert_allclose(d["bound"], [(18 * 2.5 + 8 * 3.5) * er.U, (17 * 1.0 + 8 * 3.0) * er.U], rtol=1e-15)
    np.testing.assert_array_equal(a["aty"], [-1.5, -2.0])
    np.testing.assert_allclose(a["bound"], [17 * 1.5 * er.U, 18 * 4.0 * er.U], rtol=1e-15)  # |a y'| sums: 3/2 and 3 + 1
    assert (float(s["dx2"][0]), float(s["dy2"][0]), float(s["inter"][0])) == (0.3125, 3.25, -1.375)
    assert s["inter"][1] == 18 * er.U * 1.375 and s["dx2"][1] == 18 * er.U * 0.3125 and s["dy2"][1] == 18 * er.U * 3.25
    c = dec["ctl"]
    assert dec["accepted"] and c["last_movement"] == 1.125 and dec["limit"] == 1.125 / 1.375 and dec["margin"] == pytest.approx(11 / 18, rel=1e-15)
    assert c["step_size"] == 0.5 * (1.125 / 1.375) and c["tau"] == c["step_size"] / 2.0 and c["sigma"] == c["step_size"] * 2.0
    assert (c["k"], c["attempts"], c["steps_taken"], c["its_since_restart"], c["cur"], c["pending_avg"], c["error"]) == (1, 1, 1, 1, 1, 1, 0)
    assert c["sum_weights"] == c["step_size"]
    # ... and check_attempt accepts exactly this as a device's answer, and names a stage when one number is off
    before = dict(st, ctl=ctl, X_OTHER=np.zeros(2), Y_OTHER=np.zeros(2), ATY_OTHER=np.zeros(2))
    after = dict(ctl=dict(c, target_steps=1), X=p["xn"], Y=d["y"], ATY=a["aty"], X_OTHER=st["X"], Y_OTHER=st["Y"], ATY_OTHER=st["ATY"],
                 SUM_X=st["SUM_X"], SUM_Y=st["SUM_Y"], XBAR=p["xbar"])
    before["ctl"]["target_steps"] = 1
    r = ar.check_attempt(S, prob, SP_EXACT, before, after, exact=exact)
    assert r["accepted"] and r["ratios"] == dict(y=0.0, aty=0.0, dy2=0.0, dx2=0.0, inter=0.0)
    for key, value, stage in (("Y", [-1.5, 1.0 + 2.0 ** -40], "y'"), ("ATY", [-1.5 + 2.0 ** -40, -2.0], "A^T y'"), ("SUM_Y", [2, 2.5], "SUM_Y"),
                              ("XBAR", [0.5, np.nextafter(1.0, 2.0)], "xbar")):
        with pytest.raises(AssertionError, match=stage.replace("^", r"\^")):
            ar.check_attempt(S, prob, SP_EXACT, before, dict(after, **{key: np.array(value)}), exact=exact)
    for key, value, stage in (("last_dy2", 3.25 * (1 + 2.0 ** -40), "dy2"), ("sum_weights", 0.5, "sum_weights"), ("pending_avg", 0, "pending_avg")):
        with pytest.raises(AssertionError, match=stage):
            ar.check_attempt(S, prob, SP_EXACT, before, dict(after, ctl=dict(after["ctl"], **{key: value})), exact=exact)


@pytest.mark.parametrize("exact", [False, True], ids=["longdouble", "fractions"])
def test_rejected_attempt_by_hand(exact):
    """A = [1 0 2; 0 1 0], c = (-1, 0, 0), x >= 0, x_2 <= 0, row 0: = 3, row 1: free; from x = (0, 1, 0), y = 0 on side 1 of the
    ping-pong pairs with step 2 at weight 1 (tau = sigma = 2), k = 2, an average pending.
       x' = (2, 1, 0), xbar = (4, 1, 0), A xbar = (4, 1)
       row 0: next = -8, low = up = -2: y' = -2                            row 1: free, min(+inf, 0) = 0: y' = 0
       A^T y' = (-2, 0, -4); dx = (2, 0, 0), dy = (-2, 0): dx2 = dy2 = 4, interaction = -4, movement = 2 + 2 = 4, limit = 1 < 2:
       REJECTED with margin 2.  k = 3: s1 = (1 - 1/4) 1 = 3/4, s2 = (1 + 1/16) 2: the new step is 3/4.
       The pending average is consumed all the same: SUM_X + 2 x = (1, 4, 3), SUM_Y + 2 y = (4, 5); pending_avg = 0 afterwards."""
    exact = exact or not er.LONGDOUBLE_IS_EXTENDED
    S = ar.Structure(2, 3, [0, 2, 3], [0, 2, 1])
    prob = arrays(A_VALUES=[1, 2, 1], C=[-1, 0, 0], LB=[0, 0, 0], UB=[INF, INF, 0], LO=[3, -INF], HI=[3, INF])
    st = arrays(X=[0, 1, 0], Y=[0, 0], ATY=[0, 0, 0], SUM_X=[1, 2, 3], SUM_Y=[4, 5])
    ctl = ctl_of(step_size=2.0, primal_weight=1.0, tau=2.0, sigma=2.0, sum_weights=10.0, k=2, cur=1, pending_avg=1, steps_taken=7, attempts=9,
                 its_since_restart=3)
    p, d, a, s, dec = stages(S, prob, ctl, st, SP_EXACT, exact)
    np.testing.assert_array_equal(p["xn"], [2, 1, 0])
    np.testing.assert_array_equal(p["xbar"], [4, 1, 0])
    np.testing.assert_array_equal(p["sumx"], [1, 4, 3])
    np.testing.assert_array_equal(d["y"], [-2, 0])
    np.testing.assert_array_equal(d["sumy"], [4, 5])
    assert d["bound"][1] == (17 * 2.0 + 8 * 2.0) * er.U  # (the free row: sigma |v| = 2 twice, no bound term)
    np.testing.assert_array_equal(a["aty"], [-2, 0, -4])
    assert (float(s["dx2"][0]), float(s["dy2"][0]), float(s["inter"][0])) == (4.0, 4.0, -4.0)
    c = dec["ctl"]
    assert not dec["accepted"] and (c["last_movement"], dec["limit"], dec["margin"]) == (4.0, 1.0, 2.0)
    assert (c["step_size"], c["tau"], c["sigma"]) == (0.75, 0.75, 0.75)
    assert (c["k"], c["attempts"], c["steps_taken"], c["its_since_restart"], c["cur"], c["pending_avg"], c["error"]) == (3, 10, 7, 3, 1, 0, 0)
    assert c["sum_weights"] == 10.0
    before = dict(st, ctl=ctl, X_OTHER=np.zeros(3), Y_OTHER=np.zeros(2), ATY_OTHER=np.zeros(3))
    after = dict(st, ctl=c, X_OTHER=p["xn"], Y_OTHER=d["y"], ATY_OTHER=a["aty"], SUM_X=p["sumx"], SUM_Y=d["sumy"], XBAR=p["xbar"])
    r = ar.check_attempt(S, prob, SP_EXACT, before, after, exact=exact)
    assert not r["accepted"] and r["margin"] == 2.0 and r["pending_before"] == 1 and r["cur_before"] == 1
    with pytest.raises(AssertionError, match="pending_avg"):  # (left set behind a rejection: the iterate would be averaged twice)
        ar.check_attempt(S, prob, SP_EXACT, before, dict(after, ctl=dict(c, pending_avg=1)), exact=exact)
    with pytest.raises(AssertionError, match="SUM_X"):
        ar.check_attempt(S, prob, SP_EXACT, before, dict(after, SUM_X=st["SUM_X"]), exact=exact)
    with pytest.raises(AssertionError, match="changed its own input"):
        ar.check_attempt(S, prob, SP_EXACT, before, dict(after, X=p["xn"]), exact=exact)


def test_scalar_branches_of_the_decision():
    """movement 0: the step error, k and the step untouched, the buffers flip and the weight sum grows by the step;
    interaction 0: accepted whatever the step, which grows by its full factor"""
    ctl = ctl_of(step_size=0.5, primal_weight=2.0, tau=0.25, sigma=1.0, k=3, sum_weights=1.0)
    d = ar.decision(ctl, 0.0, 0.0, 0.0, SP_EXACT)
    assert d["accepted"] and d["ctl"] == dict(ctl, error=1, cur=1, pending_avg=1, sum_weights=1.5, steps_taken=1, its_since_restart=1, attempts=1)
    d = ar.decision(ctl, 4.0, 0.0, 0.0, SP_EXACT)
    assert d["accepted"] and d["limit"] == INF and d["margin"] == 0.0 and d["ctl"]["k"] == 4 and d["ctl"]["step_size"] == (1.0 + 1.0 / 25.0) * 0.5
    assert ar.decision(ctl, float("nan"), 1.0, 1.0, SP_EXACT)["ctl"]["error"] == 1


def small_mixed_lp(seed=3):
    """300 x 200 with every kind of row and column bound, rows of 0 .. 12 entries"""
    p, x, y = sc.tiny_lp("dual-only", seed=seed, m=300, n=200, density=0.03)
    rng = np.random.default_rng(seed + 100)
    kind_r, kind_c = rng.integers(0, 5, size=300), rng.integers(0, 4, size=200)
    b = p["lo"]
    p["lo"] = np.choose(kind_r, [np.full(300, -INF), b, b, np.full(300, -INF), b - 1.0])
    p["hi"] = np.choose(kind_r, [b, np.full(300, INF), b, np.full(300, INF), b + 1.0])
    p["lb"] = np.choose(kind_c, [np.full(200, -INF), np.zeros(200), np.zeros(200), np.full(200, -INF)])
    p["ub"] = np.choose(kind_c, [np.full(200, INF), np.full(200, INF), np.full(200, 2.0), np.full(200, 2.0)])
    p["c"] = rng.standard_normal(200)
    return p, x, rng.standard_normal(300)


@pytest.mark.parametrize("which", ["synthetic", "mixed"])
def test_fixed_steps_match_the_oracle_bit_for_bit(which):
    """x and y behind orc_pdhg_fixed_steps: the element-wise expressions of the reference around row sums taken left to right in
    float64 (rowsums_f64: the oracle's order) give the oracle's bits; the extended sums stay within their own bounds of them"""
    if which == "synthetic":
        p = synthetic.generate(400, 300, 6, seed=3)
        rng = np.random.default_rng(2)
        x0, y0 = np.abs(rng.standard_normal(p["n"])), rng.standard_normal(p["m"])
    else:
        p, x0, y0 = small_mixed_lp()
    m, n = p["m"], p["n"]
    S = ar.Structure(m, n, p["offsets"], p["indices"])
    to, ti, tv = orcbind.transpose(m, n, p["offsets"], p["indices"], p["values"])
    np.testing.assert_array_equal(tv, np.asarray(p["values"])[S.order])  # (the reference's own transposition)
    np.testing.assert_array_equal(to, S.t_off)
    prob = arrays(A_VALUES=p["values"], C=p["c"], LB=p["lb"], UB=p["ub"], LO=p["lo"], HI=p["hi"])
    step, w = 0.05, 1.3
    ctl = ctl_of(step_size=step, primal_weight=w, tau=step / w, sigma=step * w)
    P, off, idx, val = orcbind._p, np.ascontiguousarray(p["offsets"], np.int32), np.ascontiguousarray(p["indices"], np.int32), np.ascontiguousarray(p["values"])
    x, y = x0.copy(), y0.copy()
    aty = ar.rowsums_f64(tv, y, to, ti)
    for it in range(1, 4):
        xo, yo = x0.copy(), y0.copy()
        orcbind.lib().orc_pdhg_fixed_steps(m, n, P(off), P(idx), P(val), P(to), P(ti), P(tv), P(prob["C"]), P(prob["LO"]), P(prob["HI"]), P(prob["LB"]),
                                           P(prob["UB"]), step / w, step * w, it, P(xo), P(yo))
        st = dict(X=x, Y=y, ATY=aty, SUM_X=np.zeros(n), SUM_Y=np.zeros(m))
        pr = ar.primal(prob, ctl, st)
        yn = ar.dual_f64(prob, ctl, st, ar.rowsums_f64(val, pr["xbar"], off, idx))
        assert ar.bits_equal(pr["xn"], xo) and ar.bits_equal(yn, yo), it
        d = ar.dual(S, prob, ctl, st, pr["xbar"])
        assert er.worst_ratio(ar.abs_err(d, yo), d["bound"]) <= 1.0
        x, y, aty = pr["xn"], yn, ar.rowsums_f64(tv, yn, to, ti)
        a = ar.aty_product(S, prob, y)
        assert er.worst_ratio(ar.abs_err(a, aty), a["bound"]) <= 1.0
    assert np.abs(y - y0).max() > 1e-3 and np.abs(x - x0).max() > 1e-3


def test_forty_iterations_follow_the_oracle():
    """the reference replays the first 40 iterations of the oracle's solve with its OWN (extended) sums: the same accepted and
    attempted counts, the same final step size (the sums differ in their last bits: rel 1e-9, as test_solve_gpu compares the device).
    The preset's min_iteration_restart = 10 makes each of the first ten iterations a major one, with restarts and new primal weights
    the attempt's restatement knows nothing of: it is 0 here, so that the 40 iterations are 40 steps of the loop and nothing else."""
    p = synthetic.generate(800, 400, 5, seed=2)  # (two of the 40 steps take a second attempt)
    h = orcbind.hyper_preset(1)
    h[orcbind.H["ORC_H_MIN_ITERATION_RESTART"]] = 0
    o = orcbind.solve(p, hyper=h, tol=0.0, iteration_limit=40)
    assert o["status"] == "IterationLimit" and int(o["steps_taken"]) == 40 and o["num_restarts"] == 0
    dr, dc = orcbind.compute_scaling(p["m"], p["n"], p["offsets"], p["indices"], p["values"], h)
    S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
    prob = dict(A_VALUES=p["values"] * dr[S.rows] * dc[S.idx], C=p["c"] * dc, LB=p["lb"] / dc, UB=p["ub"] / dc, LO=p["lo"] * dr, HI=p["hi"] * dr)
    step, w = o["initial_step_size"], o["initial_primal_weight"]
    assert step == 1.0 / np.abs(prob["A_VALUES"]).max()
    ctl = ctl_of(step_size=step, primal_weight=w, tau=step / w, sigma=step * w)
    x = np.minimum(np.maximum(np.zeros(p["n"]), prob["LB"]), prob["UB"])
    st = dict(X=x, Y=np.zeros(p["m"]), ATY=np.zeros(p["n"]), SUM_X=np.zeros(p["n"]), SUM_Y=np.zeros(p["m"]))
    sp, margins = step_params(1), []
    while ctl["steps_taken"] < 40 and ctl["attempts"] < 400:
        pr, d, a, s, dec = stages(S, prob, ctl, st, sp, None)
        margins.append(dec["margin"])
        if dec["accepted"]:
            st = dict(X=pr["xn"], Y=d["y"], ATY=a["aty"], SUM_X=pr["sumx"], SUM_Y=d["sumy"])
        else:
            st = dict(st, SUM_X=pr["sumx"], SUM_Y=d["sumy"])
        ctl = dec["ctl"]
    assert min(abs(mg - 1.0) for mg in margins) >= 1e-9, "a decision too close to a tie to be compared: take another seed"
    assert (ctl["steps_taken"], ctl["attempts"]) == (int(o["steps_taken"]), int(o["attempted_steps"]))
    assert ctl["attempts"] > ctl["steps_taken"], "no rejection among them: the comparison would not see the rejection rule"
    assert ctl["step_size"] == pytest.approx(o["final_step_size"], rel=1e-9)
    assert ctl["primal_weight"] == o["final_primal_weight"]


# ---- the GPU test's scenario on the float64 stand-in ------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=LPS, ids=LP_IDS)
def lp(request):
    p, x, y = edge_lp(*request.param)
    return p, x, y, scaling_of(p)


def test_scenario_on_the_stand_in(lp, request):
    """every bound holds for plain float64 sums, and the scenario has the properties the GPU test asserts on the device"""
    p, x0, y0, (dr, dc) = lp
    dev, S, prob = sc.stand_in(p, x0, y0, dr, dc, step_params(1))
    worst = sc.run_scenario(dev, S, prob, dev.sp, dr, dc, request.node.callspec.id)
    print(worst.line(request.node.callspec.id))
    assert max(worst.values()) <= 1.0 and min(worst[k] for k in ("y", "aty", "dy2", "dx2", "inter", "dist")) > 0.0, worst


def test_uniform_bounds_variants_on_the_stand_in():
    p, x0, y0 = edge_lp(4500, False, SEEDS[0])
    dr, dc = scaling_of(p)
    for name, q in sc.uniform_bounds_variants(p).items():
        dev, S, prob = sc.stand_in(q, x0, y0, dr, dc, step_params(1))
        worst = sc.Worst()
        for i in range(3):
            sc.assert_decided(sc.one_attempt(dev, S, prob, dev.sp, "%s %d" % (name, i), worst)[0], name)
        print(worst.line("uniform-" + name))


@pytest.mark.parametrize("kind", ["fixed-point", "dual-only"])
def test_scalar_branch_lps_on_the_stand_in(kind):
    p, x0, y0 = sc.tiny_lp(kind)
    ones_m, ones_n = np.ones(p["m"]), np.ones(p["n"])
    dev, S, prob = sc.stand_in(p, x0, y0, ones_m, ones_n, step_params(1))
    r, before, after = sc.one_attempt(dev, S, prob, dev.sp, kind)
    sc.assert_scalar_branch(kind, r, before, after, dev.sp)


# ---- the resident small-LP tests' LPs and cases on the stand-in ----------------------------------------------------------------------
EVALUATED = list(rl.SCENARIO) + list(rl.FULL)


@pytest.fixture(scope="module", params=list(rl.ALL))
def resident_lp(request):
    p, x, y = rl.lp(request.param)
    return request.param, p, x, y, scaling_of(p)


def resident_stand_in(lp):
    name, p, x0, y0, (dr, dc) = lp
    return sc.stand_in(p, x0, y0, dr, dc, step_params(1), resident=True)


def test_resident_lps_hold_what_they_promise(resident_lp):
    from cuopt_amd import capi
    name, p, x, y, _ = resident_lp
    m, n, nnz = p["m"], p["n"], len(p["values"])
    want_m, want_n, entries, tier = rl.ALL[name][:4]
    assert (m, n) == (want_m, want_n) and (entries is None or nnz == entries) and capi.resident_tier(m, n, nnz) == tier
    rlen, clen = np.diff(p["offsets"]), np.bincount(p["indices"], minlength=n)
    assert all((np.diff(p["indices"][a:b]) > 0).all() for a, b in zip(p["offsets"][:-1], p["offsets"][1:]))  # ascending, no duplicate
    if name in rl.SCENARIO or name in rl.FULL:
        assert set(rl.ROW_LENGTHS + rl.LONG_ROWS) <= set(rlen.tolist()) and clen.max() == clen[p["long_col"]] == rl.LONG_COL
        assert (rlen == 0).sum() >= rl.EMPTY and (clen[p["empty_cols"]] == 0).all() and len(p["empty_cols"]) >= rl.EMPTY
        zero_cost = (p["c"][p["empty_cols"]] == 0).sum()
        assert zero_cost == (rl.EMPTY if name in rl.FULL else rl.EMPTY // 2)
    if name in rl.FULL:  # every lane, every slot
        T, Q, U = ((256, 2, 8), (512, 2, 16), (512, 4, 8))[tier]
        assert m == n == Q * T and (nnz == U * T or (tier == 2 and nnz == 4096))
    if name == "t1-full":
        assert 8 * nnz == 65536  # k_major_small's dynamic LDS at the most it asks the runtime for
    if name == "t1":
        assert nnz > 4096
    if name == "past-n":
        assert capi.resident_tier(m, n - 1, nnz) == 0 and nnz <= 2048
    if name == "past-nnz":
        assert capi.resident_tier(m, n, nnz - 1) == 0
    if name == "rows-only":
        assert capi.resident_tier(m - 1, n, nnz) < 2 and n < 64
    if name == "cols-only":
        assert capi.resident_tier(m, n - 1, nnz) < 2 and m < 64
    if name == "spanning":
        assert rlen[rl.SPANNING_ROW] == n and clen[rl.SPANNING_COL] == m
    if min(m, n) >= 5:
        lo, hi, lb, ub = (p[k] for k in ("lo", "hi", "lb", "ub"))
        row_kinds = [np.isinf(lo) & np.isfinite(hi), np.isfinite(lo) & np.isinf(hi), lo == hi, np.isinf(lo) & np.isinf(hi), np.isfinite(lo) & np.isfinite(hi) & (lo < hi)]
        col_kinds = [np.isinf(lb) & np.isinf(ub), np.isinf(lb) & (ub == 5.0), (lb == 0.0) & np.isinf(ub), (lb == 1.5) & (ub == 1.5), (lb == 0.0) & (ub == 5.0)]
        assert all(m // 5 <= k.sum() <= -(-m // 5) for k in row_kinds) and all(n // 5 <= k.sum() <= -(-n // 5) for k in col_kinds)
        assert (x[col_kinds[3]] == 1.5).all()


def test_resident_attempts_on_the_stand_in(resident_lp, request):
    """the scenario (t0, t1, t2) or the eight natural attempts (every other LP) by the resident rules: y' and A^T y' bit for bit, the
    three sums and the restart's distances inside their bounds, and the properties the GPU test asserts on the device"""
    name, p, x0, y0, (dr, dc) = resident_lp
    dev, S, prob = resident_stand_in(resident_lp)
    if name in rl.SCENARIO:
        worst = sc.run_scenario(dev, S, prob, dev.sp, dr, dc, name, resident=True)
        assert min(worst[k] for k in ("dy2", "dx2", "inter", "dist")) > 0.0, worst
    else:
        worst = sc.Worst()
        seen = sc.edge_attempts(dev, S, prob, dev.sp, name, worst)
        assert not name.startswith("minimal") or len(seen) >= 1
    print(worst.line("stand-in " + name))
    assert max(worst.values()) <= 1.0 and worst["y"] == worst["aty"] == 0.0, worst


def test_the_resident_rules_name_a_stage():
    """check_attempt(resident=True) accepts the stand-in's own attempt and names the stage when one bit is off"""
    lp = ("t0",) + rl.lp("t0") + (scaling_of(rl.lp("t0")[0]),)
    dev, S, prob = resident_stand_in(lp)
    for _ in range(3):  # (the third has an average pending)
        before = sc.snapshot(dev)
        dev.attempt()
        after = sc.snapshot(dev)
    assert before["ctl"]["pending_avg"] == 1 and after["ctl"]["cur"] != before["ctl"]["cur"]
    ar.check_attempt(S, prob, dev.sp, before, after, resident=True)
    for key, stage in (("X", "x'"), ("Y", "y'"), ("ATY", "A^T y'"), ("SUM_X", "SUM_X"), ("SUM_Y", "SUM_Y")):
        off = after[key].copy()
        j = int(np.argmax(off != 0.0))
        off[j] = np.nextafter(off[j], np.inf)
        with pytest.raises(AssertionError, match=stage.replace("^", r"\^")):
            ar.check_attempt(S, prob, dev.sp, before, dict(after, **{key: off}), resident=True)
    with pytest.raises(AssertionError, match="dy2"):
        ar.check_attempt(S, prob, dev.sp, before, dict(after, ctl=dict(after["ctl"], last_dy2=after["ctl"]["last_dy2"] * (1 + 2.0 ** -40))), resident=True)
    rejected = dict(before, ctl=dict(after["ctl"], cur=before["ctl"]["cur"]), SUM_X=after["SUM_X"], SUM_Y=after["SUM_Y"])
    with pytest.raises(AssertionError, match="accepted|steps_taken|cur"):  # (the sums say accepted: a kept iterate is no answer)
        ar.check_attempt(S, prob, dev.sp, before, rejected, resident=True)


@pytest.mark.parametrize("start", sc.STARTS)
@pytest.mark.parametrize("name", EVALUATED)
def test_composition_case_on_the_stand_in(name, start):
    """the starts, the forced rejection in front of the run and the rejection inside it exist on these LPs (the equality itself is
    trivial on the host)"""
    p, x0, y0 = rl.lp(name)
    dr, dc = scaling_of(p)
    sp = step_params(1)
    a, b = sc.check_composition(lambda: sc.stand_in(p, x0, y0, dr, dc, sp, resident=True), sp, name, start)
    print("COMPOSITION stand-in %s from %s: %d attempts / %d steps, run %d / %d" % (name, start, *a, *b))


@pytest.mark.parametrize("name", EVALUATED)
def test_evaluated_iterates_hold_hardly_a_tie(name):
    """the condition of the GPU test's evaluation case, on the reference alone: at the iterates k_major_small evaluates (behind 3
    steps, then one more accepted step per combination) at most 0.5 % of the columns sit on a reduced-cost tie"""
    p, x0, y0 = rl.lp(name)
    dr, dc = scaling_of(p)
    dev, S, prob = sc.stand_in(p, x0, y0, dr, dc, step_params(1), resident=True)
    dev.run(3)
    worst = 0.0
    for mode, rule, eps in sc.EVAL_COMBOS:
        c = dev.ctl()
        assert c["pending_avg"] == 1 and c["error"] == 0
        dev.flush()
        dev.make_average(mode)
        for xs, ys in ((dev.get("X"), dev.get("Y")), (dev.get("AVG_X"), dev.get("AVG_Y"))):
            ref = er.evaluate(p, xs * dc, ys * dr, rule_finite=rule, eps_p=eps, eps_d=eps)
            worst = max(worst, float(ref["near_tie"].mean()))
            assert ref["near_tie"].mean() <= 0.005, (name, mode, rule, eps)
            assert ref["g_is_zero"].any()
        dev.run(c["steps_taken"] + 1)
    assert dev.ctl()["cur"] == 1 and dev.ctl()["steps_taken"] == 3 + len(sc.EVAL_COMBOS)
    print("TIES %s worst share %.4f" % (name, worst))


# ---- the sharded GPU test's cases on W stand-in ranks (tests/sharded_ranks.py) --------------------------------------------------------
FLOWS = ("allreduce", "rsag", "owner")
# world -> (rows per block, slice, last slice) of the 6000 x 6000 LP with the 4500-entry column, as the GPU test's docstring quotes them
BLOCKS = {2: ((2979, 3021), 3008, 2992), 3: ((1924, 1955, 2121), 2000, 2000), 4: ((1501, 1478, 1442, 1579), 1504, 1488)}
# the LPs behind the ids of the layout cases at world 4 (test_eval_layouts_gpu.VARIANTS): panel-*, jag-8 | pb | dense-stream, dense-panel-longtail
WORLD4 = [(0, "allreduce"), (0, "rsag"), (0, "owner"), (1, "allreduce"), (1, "owner"), (2, "allreduce"), (2, "owner")]


@pytest.fixture(scope="module")
def sharded_lps():
    out = []
    for spec in LPS[:3]:
        p, x, y = edge_lp(*spec)
        out.append((p, x, y, scaling_of(p)))
    return out


def test_row_blocks_and_slices_of_the_sharded_cases(sharded_lps):
    from cuopt_amd import capi
    p = sharded_lps[0][0]
    for world, (rows, width, last) in BLOCKS.items():
        assert tuple(np.diff(capi.partition_rows(p["m"], p["offsets"], world))) == rows
        sl = sr.slices_of(p["n"], world, "owner")
        assert all(s == (r * width, width) for r, s in enumerate(sl[:-1])) and sl[-1] == ((world - 1) * width, last), sl
    rows = np.diff(capi.partition_rows(p["m"], p["offsets"], 8))
    assert (rows.min(), rows.max()) == (649, 796) and sr.slices_of(p["n"], 8, "rsag")[-1] == (7 * 752, 736)
    assert sr.slices_of(p["n"], 8, "allreduce") == [(0, 6000)] * 8
    assert sr.slices_of(60, 8, "owner") == [(0, 16), (16, 16), (32, 16), (48, 12)] + [(60, 0)] * 4  # (the 40 x 60 LPs: four empty slices)


def _sharded_scenario(lp, world, flow, name):
    p, x0, y0, (dr, dc) = lp
    dev, S, prob = sr.stand_in(p, x0, y0, dr, dc, step_params(1), world, flow)
    worst = sc.run_scenario(dev, S, prob, dev.sp, dr, dc, name)
    print(worst.line(name))
    assert max(worst.values()) <= 1.0 and min(worst[k] for k in ("y", "aty", "dy2", "dx2", "inter", "dist")) > 0.0, worst


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("flow", FLOWS)
def test_sharded_scenario_on_the_stand_in_ranks(sharded_lps, flow, world):
    _sharded_scenario(sharded_lps[0], world, flow, "stand-in ranks %s world %d" % (flow, world))


@pytest.mark.parametrize("which,flow", WORLD4, ids=["%s-%s" % (LP_IDS[w], f) for w, f in WORLD4])
def test_sharded_scenario_of_the_layout_cases_on_the_stand_in_ranks(sharded_lps, which, flow):
    _sharded_scenario(sharded_lps[which], 4, flow, "stand-in ranks %s %s world 4" % (LP_IDS[which], flow))


def test_band_lp_of_the_transport_cases():
    """the smallest band LP on which every rank takes the halo exchange at world 4 (the rule restated on the host; the GPU test asserts
    wire_bytes()), and the scenario's properties on it under the owner-computes dataflow"""
    m, band = sr.smallest_band(4)
    assert (m, band) == sr.BAND_LP
    p, x0, y0 = sr.band_lp(m, band)
    use, worst, full = sr.halo_rule(p, 4)
    assert use and not sr.halo_rule(sr.band_lp(m // 2, band)[0], 4)[0], (worst, full)
    lo, hi = p["lo"], p["hi"]
    assert (np.isfinite(lo) & (lo == hi)).sum() == m // 5 or abs((np.isfinite(lo) & (lo == hi)).sum() - m / 5) <= 1
    print("BAND m=%d band=%d: a rank receives at most %d entries per attempt, the all-gathers bring %d" % (m, band, worst, full))
    _sharded_scenario((p, x0, y0, scaling_of(p)), 4, "owner", "stand-in ranks band world 4")


@pytest.mark.parametrize("flow", FLOWS)
@pytest.mark.parametrize("kind", ["fixed-point", "dual-only"])
def test_scalar_branch_lps_on_the_stand_in_ranks(kind, flow):
    """40 x 60 at world 8: slices of 16 columns, so rank 3 holds 12 and ranks 4 .. 7 none"""
    p, x0, y0 = sc.tiny_lp(kind)
    dev, S, prob = sr.stand_in(p, x0, y0, np.ones(p["m"]), np.ones(p["n"]), step_params(1), 8, flow)
    assert flow == "allreduce" or [s[1] for s in dev.slices] == [16, 16, 16, 12, 0, 0, 0, 0]
    r, before, after = sc.one_attempt(dev, S, prob, dev.sp, "%s %s" % (kind, flow))
    sc.assert_scalar_branch(kind, r, before, after, dev.sp)


def test_the_assembly_sees_a_stale_entry(sharded_lps):
    """what the stand-in ranks prove rests on this: a value taken from a rank that does not own it fails the check, at the stage"""
    p, x0, y0, (dr, dc) = sharded_lps[0]
    dev, S, prob = sr.stand_in(p, x0, y0, dr, dc, step_params(1), 4, "owner")
    before = sc.snapshot(dev)
    dev.attempt()
    after = sc.snapshot(dev, xbar=True)
    ar.check_attempt(S, prob, dev.sp, before, after, "owner")
    ranks = dev.b.ranks
    assert all(np.isnan(k.v["XBAR"][:k.c0]).all() and np.isnan(k.v["XBAR"][k.c0 + k.nc:]).all() for k in ranks[1:3])
    dev.slices = [dev.slices[0], (dev.slices[1][0] + 1, dev.slices[1][1]), *dev.slices[2:]]  # (rank 1's slice taken one column late)
    dev._cache.clear()
    with pytest.raises(AssertionError, match="changed its own input|xbar"):
        ar.check_attempt(S, prob, dev.sp, before, sc.snapshot(dev, xbar=True), "owner, a slice off by one")
    swapped = dict(after, ctl=dict(after["ctl"], last_dx2=after["ctl"]["last_interaction"], last_interaction=after["ctl"]["last_dx2"]))
    with pytest.raises(AssertionError):  # (two entries of the 3-scalar pack swapped)
        ar.check_attempt(S, prob, dev.sp, before, swapped, "owner, swapped sums")
