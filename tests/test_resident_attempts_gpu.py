"""GPU: the resident one-workgroup loop (resident_body) and the one-workgroup head of a major iteration (k_major_small) against the
stage-by-stage references, with CUOPT_AMD_SMALL unset: the path every LP of MIP-relaxation size takes by itself.

One attempt at a time through pdlpdev_debug_attempts, which on this path is one launch of the loop kernel capped at `count` attempts.
The rules are attempt_reference.check_attempt(resident=True): every row and column is added up by its owner left to right from products
rounded once, so x', y', A^T y' and the running sums are BIT FOR BIT the float64 restatement; the three sums of the step rule go
through a fixed tree and keep their derived bounds; the decision and everything behind it follows from the device's own three sums.
A rejected attempt leaves nothing but the control block and the running sums, so it is checked through those and through the iterate
it must not have touched.

1. the scenario of tests/attempt_scenario.py on one LP per tier (tests/resident_lps.py);
2. eight natural attempts on every LP at the edge of a tier (exact lane / slot / LDS counts, one column or nonzero past a tier, lanes
   that own rows and no column, a row as long as n, one nonzero slot);
3. a launch is the composition of its attempts: 12 attempts in one launch, and a run behind a forced rejection, leave what single
   attempts leave, bit for bit, from cur = 0, with an average pending and from cur = 1 -- the registers carried over an acceptance, the
   running sums over a rejection inside the loop, the parity tables red[2] / pw[2];
4. the two scalar branches of the decision;
5. k_major_small: its own flush of a pending average, its three averages, both reduced-cost rules, with and without the l-infinity
   pass, against tests/eval_reference.py with the checks and tolerances of tests/test_eval_layouts_gpu.py.

tests/test_attempt_reference.py runs 1 - 3 on a float64 stand-in and asserts what these cases need of the LPs (the properties of the
scenario, the rejection inside the run, hardly a reduced-cost tie at the evaluated iterates)."""
import numpy as np
import pytest

import attempt_reference as ar
import attempt_scenario as sc
import eval_reference as er
import resident_lps as rl
from cuopt_amd import capi
from test_attempt_layouts_gpu import OnDevice, step_params
from test_eval_layouts_gpu import _check_scalars, _check_vectors, _iterate

pytestmark = pytest.mark.gpu
EVALUATED = list(rl.SCENARIO) + list(rl.FULL)


@pytest.fixture(autouse=True)
def resident_by_itself(monkeypatch):
    monkeypatch.delenv("CUOPT_AMD_SMALL", raising=False)


class Resident(OnDevice):
    """attempt_scenario's interface over a resident capi.Device, with the two calls of the composition case"""

    def get(self, name):
        return self.dev.download(name, self.dev.nnz) if name == "AT_VALUES" else super().get(name)

    def attempts(self, count):
        return self.dev.attempts(count)

    def run(self, target):
        return self.dev.run(target)


def prepared(p, x0, y0, tier=None, scale=True):
    """step 1 of the scenario on a resident context -> (Resident, Structure, the scaled problem as the device holds it, D_r, D_c)"""
    raw = capi.Device(p)
    assert raw.layout()["resident"], raw.layout()
    assert tier is None or capi.resident_tier(p["m"], p["n"], len(p["values"])) == tier
    dev = Resident(raw, step_params(1))
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
    prob = sc.download_problem(dev)
    prob["AT_VALUES"] = dev.get("AT_VALUES")  # (scaled in the other order: an entry may differ from A's in its last bit)
    np.testing.assert_allclose(prob["AT_VALUES"], prob["A_VALUES"][S.order], rtol=4e-16, atol=0)
    return dev, S, prob, dev.get("DROW"), dev.get("DCOL")


def prepared_lp(name):
    return prepared(*rl.lp(name), tier=rl.tier_of(name))


@pytest.mark.parametrize("name", list(rl.SCENARIO))
def test_scenario_per_tier(name):
    dev, S, prob, dr, dc = prepared_lp(name)
    worst = sc.run_scenario(dev, S, prob, dev.sp, dr, dc, name, resident=True)
    dev.dev.close()
    print(worst.line(name))
    assert max(worst.values()) <= 1.0 and min(worst[k] for k in ("dy2", "dx2", "inter", "dist")) > 0.0, worst


@pytest.mark.parametrize("name", list(rl.FULL) + list(rl.EDGE))
def test_natural_attempts_at_the_edges(name):
    dev, S, prob, dr, dc = prepared_lp(name)
    worst = sc.Worst()
    seen = sc.edge_attempts(dev, S, prob, dev.sp, name, worst)
    dev.dev.close()
    print(worst.line(name) + " outcomes " + "".join("E" if r["error"] else "A" if r["accepted"] else "r" for r in seen))
    assert max(worst.values()) <= 1.0 and len(seen) >= 1, worst


@pytest.mark.parametrize("start", sc.STARTS)
@pytest.mark.parametrize("name", EVALUATED)
def test_a_launch_is_the_composition_of_its_attempts(name, start):
    made = []

    def make():
        made.append(prepared_lp(name))
        return made[-1][:3]

    a, b = sc.check_composition(make, step_params(1), name, start)
    for m in made:
        m[0].dev.close()
    print("COMPOSITION %s from %s: %d attempts / %d steps, run %d / %d" % (name, start, *a, *b))


@pytest.mark.parametrize("kind", ["fixed-point", "dual-only"])
def test_scalar_branches(kind):
    p, x0, y0 = sc.tiny_lp(kind)
    dev, S, prob, dr, dc = prepared(p, x0, y0, tier=0, scale=False)
    r, before, after = sc.one_attempt(dev, S, prob, dev.sp, kind, resident=True)
    sc.assert_scalar_branch(kind, r, before, after, dev.sp)
    if kind == "fixed-point":  # (with the error up the launch makes no attempt)
        c = dev.attempts(1)
        assert (c.error, c.attempts, c.steps_taken) == (1, 1, 1)
        again = sc.snapshot(dev)
        assert all(ar.bits_equal(again[k], after[k]) for k in sc.CURRENT_SIDE)
    dev.dev.close()


@pytest.mark.parametrize("name", EVALUATED)
def test_major_small_against_the_reference(name):
    p, x0, y0 = rl.lp(name)
    m, n = p["m"], p["n"]
    empty_rows, empty_cols = np.diff(p["offsets"]) == 0, np.bincount(p["indices"], minlength=n) == 0
    dev, S, prob, dr, dc = prepared_lp(name)
    raw = dev.dev
    ctl = raw.run(3)
    assert (ctl.error, ctl.steps_taken, ctl.cur, ctl.pending_avg) == (0, 3, 1, 1), (ctl.error, ctl.steps_taken, ctl.cur, ctl.pending_avg)
    worst = {}
    for mode, rule, eps in sc.EVAL_COMBOS:
        refs = {}
        for pending in (1, 0):  # (the first evaluation flushes the pending average itself; the second finds nothing pending)
            tag = "%s mode=%d rule=%d eps=%g pending=%d" % (name, mode, rule, eps, pending)
            st = sc.snapshot(dev)
            assert st["ctl"]["pending_avg"] == pending and st["ctl"]["sum_weights"] > 0.0, (tag, st["ctl"])
            sx, sy = ar.flush(st["ctl"], st)
            ax, ay = ar.make_average(mode, st["ctl"], dict(st, SUM_X=sx, SUM_Y=sy))
            cur, avg = raw.major_eval(mode, rule_finite=rule, eps_p=eps, eps_d=eps)
            after = sc.snapshot(dev)
            assert ar.bits_equal(after["SUM_X"], sx) and ar.bits_equal(after["SUM_Y"], sy), (tag, "the flush inside k_major_small")
            assert after["ctl"] == dict(st["ctl"], pending_avg=0), (tag, after["ctl"], st["ctl"])
            for k in ("X", "Y", "ATY"):
                assert ar.bits_equal(after[k], st[k]), (tag, "the evaluation changed", k)
            assert ar.bits_equal(dev.get("AVG_X"), ax) and ar.bits_equal(dev.get("AVG_Y"), ay), (tag, "the average")
            if mode == 2:
                assert np.abs(ax - st["X"]).max() > 0.0 and np.abs(ay - st["Y"]).max() > 0.0, (tag, "the average is the iterate")
            for slot, ev, xname, yname in (("CURRENT", cur, "X", "Y"), ("AVERAGE", avg, "AVG_X", "AVG_Y")):
                if slot not in refs:  # (the same iterate and average behind the flush: one reference for both evaluations)
                    xs, ys = _iterate(raw, xname, yname, dr, dc)
                    refs[slot] = er.evaluate(p, xs, ys, rule_finite=rule, eps_p=eps, eps_d=eps)
                _check_scalars(ev, refs[slot], eps >= 0, tag + " " + slot)
                for k, v in _check_vectors(raw, slot, refs[slot], empty_rows, empty_cols, tag + " " + slot).items():
                    worst[k] = max(worst.get(k, 0.0), v)
        ctl = raw.run(st["ctl"]["steps_taken"] + 1)  # the next combination: another iterate, the other side, an average pending
        assert ctl.error == 0 and ctl.pending_avg == 1
    raw.close()
    print("WORST-EVAL %s ax=%.3f aty=%.3f rc=%.3f" % (name, worst["ax"], worst["aty"], worst["rc"]))
