"""GPU: the resident reflected-Halpern code -- resident_halpern_body, major_small_halpern_body and halpern_restart_finish_workgroup
(cuopt_amd/csrc/resident_halpern_bodies.hpp) through their three sets of wrapper kernels -- against the stage-by-stage references, with
CUOPT_AMD_SMALL unset: the path every LP of MIP-relaxation size takes by itself in mode 4 with halpern_resident.

The context is prepared as tests/test_halpern_step_layouts_gpu.py prepares it (Ruiz 10 + Pock-Chambolle, set_halpern, eta = STEP_SAFETY /
sigma_max, omega from the norms, halpern_restart(-1)); in Halpern mode run(steps_taken + 1) is ONE launch of the loop kernel that makes
one step.  The rules are halpern_step_reference.check_step(resident=True): every row and column is added up by its owner left to right
from products rounded once, so x', y', x^{k+1}, y^{k+1} and A^T y^{k+1} are BIT FOR BIT the float64 restatement (A^T from the device's
own AT_VALUES); the three sums go through a fixed tree and keep their derived bounds; the decision follows from the device's own sums.
The LPs are tests/resident_lps.py's, at the exact edges of the three tiers.

1. the scenario of tests/halpern_step_scenario.py on one LP per tier;
2. three checked steps, a smoothed restart and two more checked steps on every LP at the edge of a tier;
3. a launch is the composition of its steps: 12 steps in one launch leave what 12 single-step launches leave, bit for bit, from
   cur = 0, from cur = 1 and behind a restart whose anchor is not the start -- the registers carried from step to step against what a
   launch re-reads, the store of z^k on the last step, and a launch without a step, which must not touch the average slots;
4. the two scalar branches of the decision, which in the loop every lane takes on its own copy of both blocks;
5. k_major_small_halpern against tests/eval_reference.py with the checks and tolerances of tests/test_eval_layouts_gpu.py (the kernel is
   a statement-for-statement copy of k_major_small's pass over the average, which tests/test_resident_attempts_gpu.py pins), and its
   ray pass against tests/halpern_ray_reference.py;
6. the same bodies through the K-workgroup batch and the device-decided bursts, on all 13 LPs in ONE batch: every member bit for bit
   its own solve.

tests/test_halpern_step_reference.py runs 1 - 3 on a float64 stand-in, shows that stand-ins wrong in one place fail at that stage, and
asserts what these cases need of the LPs; the id lists of 5 are its constants."""
import numpy as np
import pytest

import attempt_reference as ar
import attempt_scenario as asc
import eval_reference as er
import halpern_ray_reference as R
import halpern_step_reference as hr
import halpern_step_scenario as sc
import resident_lps as rl
from cuopt_amd import capi
from test_eval_layouts_gpu import _check_scalars, _check_vectors, _iterate
from test_halpern_step_layouts_gpu import prepared
from test_halpern_step_reference import EVALUATED, overflow_lp
from test_small_batch_gpu import same

pytestmark = pytest.mark.gpu
COMPOSED_LPS = list(rl.SCENARIO) + list(rl.FULL) + ["rows-only", "cols-only", "minimal-1x2"]
ON = dict(mode=4, halpern_resident=1, halpern_batch=1, tol=0.0)
BUDGET = {name: 400 for name in rl.ALL}  # iteration_limit per id: every solve must restart within it (the restatement: at its first major iteration)
EVERYTHING = hr.AFTER_RESIDENT
FIGURES = R.KEYS


@pytest.fixture(autouse=True)
def resident_by_itself(monkeypatch):
    monkeypatch.delenv("CUOPT_AMD_SMALL", raising=False)


def prepared_resident(p, x0, y0, tier, scale=True):
    """-> (OnDevice over a resident context right before its first step, Structure, the scaled problem with AT_VALUES)"""
    raw = capi.Device(p)
    assert raw.layout()["resident"], raw.layout()
    assert capi.resident_tier(p["m"], p["n"], len(p["values"])) == tier
    dev, S, prob = prepared(raw, p, x0, y0, scale=scale, resident=True)
    np.testing.assert_allclose(prob["AT_VALUES"], prob["A_VALUES"][S.order], rtol=4e-16, atol=0)  # (scaled in the other order: the last bit may differ)
    return dev, S, prob


def prepared_lp(name):
    return prepared_resident(*rl.lp(name), tier=rl.tier_of(name))


def unchanged(held, dev, tag, skip=()):
    sc._same_end(held, sc.snapshot(dev, EVERYTHING), tag, EVERYTHING, skip)


# ---- 1. the scenario, one LP per tier -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rl.SCENARIO))
def test_scenario_per_tier(name):
    dev, S, prob = prepared_lp(name)
    worst = sc.run_scenario(dev, S, prob, name, resident=True)
    dev.dev.close()
    print(worst.line(name))
    assert max(worst.values()) <= 1.0 and min(worst[k] for k in ("dy2", "dx2", "inter", "dist")) > 0.0, worst


# ---- 2. the edges of the tiers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rl.FULL) + list(rl.EDGE))
def test_steps_at_the_edges(name):
    dev, S, prob = prepared_lp(name)
    worst, record = sc.edge_steps(dev, S, prob, name)
    dev.dev.close()
    print(worst.line(name))
    assert max(worst.values()) <= 1.0 and len(record) == 5, worst


# ---- 3. a launch is the composition of its steps -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", sc.STARTS)
@pytest.mark.parametrize("name", COMPOSED_LPS)
def test_a_launch_is_the_composition_of_its_steps(name, start):
    made = []

    def make():
        made.append(prepared_lp(name))
        return made[-1]

    steps = sc.check_composition(make, name, start)
    for m in made:
        m[0].dev.close()
    print("COMPOSITION %s from %s: %d steps in one launch against single steps" % (name, start, steps))


# ---- 4. the scalar branches ------------------------------------------------------------------------------------------------------------------
def test_a_fixed_point_of_the_operator():
    """test_halpern_step_layouts_gpu's assertions: r2 = r = r_first = r2_min = 0 and no error on every step; a step at k = 0
    (w = w0 = 1/2) keeps every bit of the iterate -- from cur = 0, and behind halpern_restart(-1) from cur = 1 -- and the step at k = 1
    behind it still finds r2 = 0 exactly"""
    p, x0, y0 = asc.tiny_lp("fixed-point")
    dev, S, prob = prepared_resident(p, x0, y0, tier=0, scale=False)
    start = sc.snapshot(dev)
    for i, k in enumerate((0, 0, 1)):
        if i == 1:
            assert dev.halpern_restart(-1.0) == (0.0, 0.0)
        r, before, after = sc.one_step(dev, S, prob, "fixed point %d" % i, resident=True)
        assert (r["k_before"], r["cur_before"]) == (k, i & 1), r
        assert (r["r2"], r["dx2"], r["dy2"], r["inter"], r["error"]) == (0.0, 0.0, 0.0, 0.0, 0), r
        assert (after["hal"]["r"], after["hal"]["r_first"], after["hal"]["r2"], after["hal"]["r2_min"]) == (0.0, 0.0, 0.0, 0.0), after["hal"]
        assert after["ctl"]["error"] == 0
        if k == 0:
            assert all(ar.bits_equal(after[key], start[key]) for key in ("X", "Y", "ATY")), "the fixed point moved"
    dev.dev.close()


def test_an_overflow_raises_the_step_error():
    """Y with 1e200 on a "<=" row: y' = 0 there, dy^2 overflows in every lane's copy, r2 = inf raises `error`; hal keeps every field,
    the counters advance all the same, and the next run makes no step and changes no buffer"""
    p, x0, y0 = overflow_lp()
    dev, S, prob = prepared_resident(p, x0, y0, tier=0, scale=False)
    assert prob["LO"][0] == -np.inf and np.isfinite(prob["HI"][0])
    y = dev.get("Y")
    y[0] = 1e200
    dev.put("Y", y)
    before = sc.snapshot(dev)
    assert before["Y"][0] == 1e200
    c = dev.run(1)
    after = sc.snapshot(dev, EVERYTHING)
    assert hr.check_decision(before, after, "overflow")["error"] == 1
    assert after["ctl"]["last_dy2"] == np.inf and after["ctl"]["last_movement"] == np.inf and after["AVG_Y"][0] == 0.0, after["ctl"]
    assert after["hal"] == before["hal"], (before["hal"], after["hal"])
    assert (c.error, c.attempts, c.steps_taken, c.k, c.cur, c.its_since_restart) == (1, 1, 1, 1, 1, 1)
    c = dev.run(2)
    assert (c.error, c.attempts, c.steps_taken) == (1, 1, 1) and dev.hal() == before["hal"]
    unchanged(after, dev, "the run behind the step error", skip=("target_steps",))
    dev.dev.close()


# ---- 5. the evaluation of T(z^k) and its ray pass ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EVALUATED)
def test_major_small_halpern_against_the_reference(name):
    """behind run(3) and behind run(4) (cur = 1 and cur = 0): the eight scalars and the three vectors of the evaluation of the average
    slots against the reference at the downloaded, unscaled AVG_X / AVG_Y, under both reduced-cost rules, with and without the
    l-infinity pass; both returned blocks carry the same bits; the evaluation changes no buffer and neither block"""
    p, x0, y0 = rl.lp(name)
    empty_rows, empty_cols = np.diff(p["offsets"]) == 0, np.bincount(p["indices"], minlength=p["n"]) == 0
    dev, S, prob = prepared_lp(name)
    raw, dr, dc = dev.dev, dev.get("DROW"), dev.get("DCOL")
    worst = {}
    for steps in (3, 4):
        ctl = raw.run(steps)
        assert (ctl.error, ctl.steps_taken, ctl.cur) == (0, steps, steps & 1)
        held = sc.snapshot(dev, EVERYTHING)
        xs, ys = _iterate(raw, "AVG_X", "AVG_Y", dr, dc)
        for rule in (True, False):
            for eps in (1e-4, -1.0):
                tag = "%s steps=%d rule=%d eps=%g" % (name, steps, rule, eps)
                ref = er.evaluate(p, xs, ys, rule_finite=rule, eps_p=eps, eps_d=eps)
                cur, avg = raw.major_eval(3, rule_finite=rule, eps_p=eps, eps_d=eps)
                assert ar.bits_equal(cur, avg), (tag, "current and average are the same point in this mode", cur, avg)
                _check_scalars(avg, ref, eps >= 0, tag)
                for k, v in _check_vectors(raw, "AVERAGE", ref, empty_rows, empty_cols, tag).items():
                    worst[k] = max(worst.get(k, 0.0), v)
                unchanged(held, dev, tag + ": the evaluation changed")
    raw.close()
    print("WORST-EVAL %s ax=%.3f aty=%.3f rc=%.3f" % (name, worst["ax"], worst["aty"], worst["rc"]))


def ray_figures(dev, p, dr, dc, tag):
    """the evaluation's ray pass under both rules against ray_info of the displacement the device holds: T(z^k) in the average slots,
    z^k in the side `cur` does not select"""
    raw = dev.dev
    dx, dy = (dev.get("AVG_X") - dev.get("X_OTHER")) * dc, (dev.get("AVG_Y") - dev.get("Y_OTHER")) * dr
    assert np.any(dx != 0.0) and np.any(dy != 0.0), tag
    for rule in (True, False):
        raw.major_eval(3, rule_finite=rule, eps_p=1e-4, eps_d=1e-4)
        syncs = raw.loop_stats()["loop_syncs"]
        got = raw.halpern_eval_infeasibility(rule_finite=rule)
        assert raw.loop_stats()["loop_syncs"] == syncs, (tag, "the figures are not those the evaluation's own ray pass left")
        ref = R.ray_info(p, dx, dy, finite_bounds_rule=rule)
        print("RAY %s rule=%d %s" % (tag, rule, " ".join("%.6e" % got[k] for k in FIGURES)))
        for k in FIGURES:
            assert got[k] == pytest.approx(ref[k], rel=1e-10, abs=1e-12), (tag, rule, k, got[k], ref[k])


@pytest.mark.parametrize("name", EVALUATED)
def test_ray_pass_against_the_reference(name):
    """with set_halpern_rays: the four figures behind run(3) (a launch of three steps), behind run(4) (a single-step launch, the other
    parity) and behind run(9) -- a launch of five steps, whose z^k only the store on its last step puts where the pass reads it; that
    what the pass reads there IS the z^k of the last step is check_last_step_store's assertion"""
    p, x0, y0 = rl.lp(name)
    dev, S, prob = prepared_lp(name)
    raw, dr, dc = dev.dev, dev.get("DROW"), dev.get("DCOL")
    raw.set_halpern_rays(True)
    for steps in (3, 4, 9):
        ctl = raw.run(steps)
        assert (ctl.error, ctl.steps_taken, ctl.cur) == (0, steps, steps & 1)
        held = sc.snapshot(dev, EVERYTHING)
        hr.check_last_step_store(S, prob, held, "%s steps=%d" % (name, steps))  # (the reference below takes the device's own z^k: this is what ties it to T(z^k))
        ray_figures(dev, p, dr, dc, "%s steps=%d" % (name, steps))
        unchanged(held, dev, "%s steps=%d: the ray pass changed" % (name, steps))
    raw.close()


# ---- 6. the same bodies through the batch and the burst wrappers ----------------------------------------------------------------------------
def solver_of(name, **kw):
    p, x0, y0 = rl.lp(name)
    s = capi.Solver(p, init_x=x0, init_y=y0, iteration_limit=BUDGET[name], **dict(ON, **kw))
    assert s.device.layout()["resident"], (name, s.device.layout())
    return s


@pytest.fixture(scope="module")
def singles():
    """every LP's own solve with the decisions on the host, once for the three batches"""
    out = {}
    for name in rl.ALL:
        s = solver_of(name)
        out[name] = (s.advance(), s.solution())
        s.close()
    return out


def test_every_single_solve_restarts(singles):
    """k_restart_batch + k_halpern_restart_finish_batch and the burst's guarded restart run for every member, on every tier"""
    counts = {name: (r["steps_taken"], r["num_restarts"]) for name, (r, _) in singles.items()}
    print("RESTARTS", counts)
    without = [name for name, (_, restarts) in counts.items() if restarts < 1]
    assert not without, ("no restart within the budget, where the restatement restarts at its first major iteration", without, BUDGET)


@pytest.mark.parametrize("P", [0, 1, 4])
def test_batch_of_every_edge_lp(singles, P):
    """ONE K-workgroup batch of the 13 LPs -- mixed tiers, rows-only and cols-only among them, where a swap of m and n in a member's
    argument record would show -- with the decisions on the host (P = 0) and on the device, P periods per synchronisation: every member
    matches its own solve on every result field but the two timings and on x, y, z"""
    solvers = [solver_of(name) for name in rl.ALL]
    batch = capi.SmallBatch(solvers)
    assert batch.stats()["halpern"] == 1 and batch.stats()["tiers"] == 3
    if P:
        batch.set_halpern_device_major(P)
        assert batch.halpern_device_major() == P
    got = batch.advance()
    if P:
        assert batch.burst_stats()["bursts"] >= 1
    for name, s, r in zip(rl.ALL, solvers, got):
        want, solution = singles[name]
        same(want, r)
        for what, u, v in zip("xyz", solution, s.solution()):
            assert ar.bits_equal(u, v), (name, P, what, hr._first(u, v))
    batch.close()
    for s in solvers:
        s.close()


def test_single_burst_at_the_lds_limit():
    """t1-full has 8192 entries: k_major_small_halpern_burst asks for all 65 536 bytes of LDS the evaluation may ask for.  The single
    solver with halpern_device_major = 4 against the same solver with the option at 0 (halpern_batch off on both: a solver takes only
    one of the two settings)"""
    name = "t1-full"
    assert 8 * len(rl.lp(name)[0]["values"]) == 65536
    got = []
    for P in (4, 0):
        s = solver_of(name, halpern_batch=0, halpern_device_major=P)
        got.append((s.advance(), s.solution()))
        assert (s.device.halpern_burst_stats()["bursts"] >= 1) == (P > 0)
        s.close()
    assert got[1][0]["num_restarts"] >= 1 and got[1][0]["steps_taken"] == BUDGET[name]
    same(got[1][0], got[0][0])
    for what, u, v in zip("xyz", got[1][1], got[0][1]):
        assert ar.bits_equal(u, v), (name, what, hr._first(u, v))
