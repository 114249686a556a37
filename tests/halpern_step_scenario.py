"""TEST UTILITY: the scenario that tests/test_halpern_step_layouts_gpu.py runs on the device and tests/test_halpern_step_reference.py on a
plain float64 stand-in, checked stage by stage with tests/halpern_step_reference.py.  numpy (and, for the stand-in, scipy) only.

`dev` is anything with ctl() -> control block (dict), hal() -> dict(r, r_first, r2, r2_min, k), get(buffer name) -> array,
run(target) (steps until steps_taken = target), halpern_restart(theta) -> the two distances, put(buffer name, array).

The scenario, on a context right behind halpern_restart(-1) at its start:
  1. three single steps: k = 0, 1, 2 from cur = 0, 1, 0, each checked
  2. one run of RUN_STEPS = 7 steps in one call (graphs of 4 + 2 + 1 on the device; what can be seen of it -- the counters, and that
     it moved -- is asserted here, its bits by the GPU test's split-invariance case)
  3. halpern_restart(THETA), checked: both distances are far above 1e-10, the weight is smoothed
  4. two single steps, checked (k = 0, 1 again, behind the new weight, tau and sigma, from an anchor that is not the start)
  5. halpern_restart(THETA) and another one right behind it: the second finds both distances 0 and leaves the weight untouched
  6. one more single step, so that the last restart has something to measure, and halpern_restart(-1): distances above 1e-10, and the
     weight untouched all the same.

resident=True (tests/test_halpern_resident_steps_gpu.py on the device, the resident stand-in on the host): the same scenario by the
rules of the resident one-workgroup loop -- a snapshot then holds neither XBAR nor the partials, and the problem carries AT_VALUES.
check_composition is that path's further case: a launch is the composition of its steps."""
import numpy as np

import attempt_reference as ar
import halpern_reference as H
import halpern_step_reference as hr

RUN_STEPS = 7
CHECKED_STEPS = 3  # of steps_and_a_restart


def rows_as_equalities(p, rows):
    """p with the rows `rows` turned into equality rows: lo = hi = the finite bound the row had (its lower one; 0.5 on a free row).
    y' of a free row is 0 and y' of an inactive inequality row is clamped to 0 WHATEVER the A product gave for it, so a wrong sum of
    such a row cannot show in any buffer -- and the long rows of tests/eval_lps.edge_lp, which are there for the sake of their sums
    (the cooperative path, a row with a workgroup of its own, a row over many slabs, the dense segments), draw their kind at random
    like every other row: at seed 5 the 2049-nonzero row is free, at seed 6 all four long rows are.  On an equality row
    y' = y - sigma (v - b): the row sum is seen at full weight."""
    rows = np.asarray(sorted(rows), dtype=np.int64)
    lo, hi = np.array(p["lo"], dtype=np.float64), np.array(p["hi"], dtype=np.float64)
    b = np.where(np.isfinite(lo[rows]), lo[rows], np.where(np.isfinite(hi[rows]), hi[rows], 0.5))
    lo[rows], hi[rows] = b, b
    return dict(p, lo=lo, hi=hi)


def steps_and_a_restart(dev, S, prob, tag, steps=CHECKED_STEPS, resident=False, both_halves=True):
    """`steps` single steps (k = 0, 1, ... from cur = 0, 1, ...) and halpern_restart(THETA), each checked -> (Worst, the steps' results).
    Every step moves both halves; both_halves=False asks for one of them only (an LP of ONE row or ONE column, whose single y' or x'
    may rest on a bound for a step)."""
    worst, record = Worst(), []
    for i in range(steps):
        r = one_step(dev, S, prob, "%s step %d" % (tag, i), worst, record, resident)[0]
        assert (r["k_before"], r["cur_before"], r["error"]) == (i, i & 1, 0), (tag, r)
        assert (r["dx2"] > 0.0 and r["dy2"] > 0.0) if both_halves else (r["dx2"] > 0.0 or r["dy2"] > 0.0), (tag, r)
    r, dist = one_restart(dev, H.THETA, tag + " restart", worst)[:2]
    assert r["smoothed"], (tag, dist)
    return worst, record


def snapshot(dev, names=hr.BEFORE):
    out = {k: dev.get(k) for k in names}
    out["ctl"], out["hal"] = dev.ctl(), dev.hal()  # (ctl() first: it is what reads both blocks back)
    return out


def download_problem(dev, resident=False):
    """the scaled problem as the device holds it; resident: with the values of A^T's own CSR, which the one-workgroup loop reads"""
    return {k: dev.get(k) for k in ar.PROBLEM + (("AT_VALUES",) if resident else ())}


class Worst(dict):
    def __init__(self):
        super().__init__({k: 0.0 for k in hr.RATIOS})

    def take(self, ratios):
        for k, v in ratios.items():
            self[k] = max(self[k], v)

    def line(self, name):
        return "WORST %s " % name + " ".join("%s=%.3g" % (k, self[k]) for k in hr.RATIOS)


def one_step(dev, S, prob, tag, worst=None, record=None, resident=False):
    """one step through run(steps_taken + 1), checked fully against the state in front of it -> (result, before, after)"""
    before = snapshot(dev)
    dev.run(before["ctl"]["steps_taken"] + 1)
    after = snapshot(dev, hr.AFTER_RESIDENT if resident else hr.AFTER)
    r = hr.check_step(S, prob, before, after, tag, resident=resident)
    if worst is not None:
        worst.take(r["ratios"])
    if record is not None:
        record.append(r)
    return r, before, after


def one_restart(dev, theta, tag, worst=None):
    before = snapshot(dev)
    dist = dev.halpern_restart(theta)
    after = snapshot(dev)
    r = hr.check_restart(before, after, dist, theta, tag)
    if worst is not None:
        worst.take(r["ratios"])
    return r, dist, before, after


def run_scenario(dev, S, prob, name, record=None, resident=False):
    """steps 1 .. 6 on a prepared context -> Worst"""
    worst = Worst()
    first = snapshot(dev)
    assert (first["hal"]["k"], first["ctl"]["cur"], first["ctl"]["steps_taken"], first["ctl"]["error"]) == (0, 0, 0, 0), (name, first["ctl"], first["hal"])
    for name_, anchor in (("X", "LAST_RESTART_X"), ("Y", "LAST_RESTART_Y"), ("ATY", "LAST_RESTART_ATY")):
        assert ar.bits_equal(first[name_], first[anchor]), (name, "the start is not its own anchor", name_)
    for i in range(3):  # 1.
        r = one_step(dev, S, prob, "%s step %d" % (name, i), worst, record, resident)[0]
        assert (r["k_before"], r["cur_before"], r["error"]) == (i, i & 1, 0), (name, i, r)
    held = snapshot(dev)  # 2.
    dev.run(held["ctl"]["steps_taken"] + RUN_STEPS)
    after = snapshot(dev)
    assert (after["ctl"]["steps_taken"], after["ctl"]["attempts"], after["hal"]["k"], after["ctl"]["error"]) == (3 + RUN_STEPS, 3 + RUN_STEPS, 3 + RUN_STEPS, 0), after
    assert after["ctl"]["cur"] == (3 + RUN_STEPS) & 1 and np.abs(after["X"] - held["X"]).max() > 0.0 and np.abs(after["Y"] - held["Y"]).max() > 0.0, name
    r, dist = one_restart(dev, H.THETA, name + " restart", worst)[:2]  # 3.
    assert r["smoothed"] and min(dist) > 1e-6, (name, "the restart measured nothing", dist)
    for i in range(2):  # 4.
        r = one_step(dev, S, prob, "%s restarted step %d" % (name, i), worst, record, resident)[0]
        assert (r["k_before"], r["error"]) == (i, 0), (name, i, r)
    r, dist = one_restart(dev, H.THETA, name + " second restart", worst)[:2]  # 5.
    assert r["smoothed"], (name, dist)
    r, dist, before, after = one_restart(dev, H.THETA, name + " restart behind a restart", worst)
    assert tuple(dist) == (0.0, 0.0) and not r["smoothed"] and after["ctl"]["primal_weight"] == before["ctl"]["primal_weight"], (name, dist)
    r = one_step(dev, S, prob, name + " last step", worst, record, resident)[0]  # 6.
    assert (r["k_before"], r["error"]) == (0, 0), (name, r)
    r, dist = one_restart(dev, -1.0, name + " restart with theta < 0", worst)[:2]
    assert not r["smoothed"] and min(dist) > 1e-10, (name, dist)
    return worst


# ---- the resident loop's further case: a launch is the composition of its steps -------------------------------------------------------------
LAUNCH_STEPS = 12  # steps of the one launch that is compared with as many single-step launches
STARTS = ("fresh", "cur1", "restarted")  # k = 0, cur = 0 | one step on: cur = 1 | three steps and a smoothed restart: another anchor, k = 0, new tau / sigma
COMPOSED = ("X", "Y", "ATY", "AVG_X", "AVG_Y", "X_OTHER", "Y_OTHER") + hr.ANCHORS  # (ATY_OTHER: not promised behind a multi-step launch)


def edge_steps(dev, S, prob, name):
    """the edge LPs' case: three checked single steps and a smoothed restart, then two more checked steps -> (Worst, the five results).
    Every rule is checked on every LP; that each step moves BOTH halves is a property of the LP, asked of all but the two of one row or
    one column (as attempt_scenario.edge_attempts asks nothing of their sequence)."""
    worst, record = steps_and_a_restart(dev, S, prob, name, resident=True, both_halves=min(S.m, S.n) > 1)
    for i in range(2):
        r = one_step(dev, S, prob, "%s restarted step %d" % (name, i), worst, record, resident=True)[0]
        assert (r["k_before"], r["error"]) == (i, 0), (name, i, r)
    return worst, record


def start_state(dev, start):
    """the prepared context moved to one of STARTS"""
    first = snapshot(dev)
    if start == "cur1":
        dev.run(1)
    elif start == "restarted":
        dev.run(3)
        dist = dev.halpern_restart(H.THETA)
        assert min(dist) > hr.SMALL_DISTANCE, (start, "the restart measured nothing", dist)
    c, h = dev.ctl(), dev.hal()
    want = dict(fresh=(0, 0, 0), cur1=(1, 1, 1), restarted=(1, 3, 0))[start]
    assert (c["cur"], c["steps_taken"], h["k"]) == want and c["error"] == 0, (start, c, h)
    if start == "restarted":
        assert not ar.bits_equal(dev.get("LAST_RESTART_X"), first["X"]) and (c["tau"], c["sigma"]) != (first["ctl"]["tau"], first["ctl"]["sigma"]), start


def _same_end(a, b, tag, names, skip=()):
    for k in a["ctl"]:
        assert k in skip or a["ctl"][k] == b["ctl"][k], (tag, "control block", k, a["ctl"][k], b["ctl"][k])
    for k in hr.HAL_FIELDS:
        assert ar.bits_equal([a["hal"][k]], [b["hal"][k]]), (tag, "hal", k, a["hal"][k], b["hal"][k])
    for k in names:
        assert ar.bits_equal(a[k], b[k]), (tag, k, hr._first(a[k], b[k]))


def check_composition(make, name, start):
    """A launch is the composition of its steps.  make() -> (dev, S, prob) prepared afresh, the same state every time.
    (a) run(steps_taken + LAUNCH_STEPS), ONE launch, leaves X, Y, A^T y, T(z^k) of the last step (AVG_X, AVG_Y), z^k of the last
        step (X_OTHER, Y_OTHER: the last-step store), the three anchors and BOTH blocks -- target_steps included -- bit for bit what
        LAUNCH_STEPS single-step launches leave: the registers a launch carries from step to step are what a launch re-reads.
    (b) behind either, run(steps_taken) -- a launch that finds its target reached -- changes no buffer (AVG_X and AVG_Y in
        particular: it made no step) and no field of either block but target_steps.
    -> the steps of (a)"""
    tag = "%s from %s" % (name, start)
    ends = []
    for single in (False, True):
        dev = make()[0]
        start_state(dev, start)
        base = dev.ctl()["steps_taken"]
        if single:
            for i in range(LAUNCH_STEPS):
                dev.run(base + i + 1)
        else:
            dev.run(base + LAUNCH_STEPS)
        ends.append(snapshot(dev, COMPOSED))
        c = ends[-1]["ctl"]
        assert (c["steps_taken"], c["target_steps"], c["error"], c["cur"]) == (base + LAUNCH_STEPS, base + LAUNCH_STEPS, 0, (base + LAUNCH_STEPS) & 1), (tag, c)
        held = snapshot(dev, hr.AFTER_RESIDENT)
        dev.run(held["ctl"]["steps_taken"])
        _same_end(held, snapshot(dev, hr.AFTER_RESIDENT), tag + ": a launch without a step changed", hr.AFTER_RESIDENT, skip=("target_steps",))
    _same_end(ends[0], ends[1], tag + ": one launch against single steps", COMPOSED)
    return LAUNCH_STEPS


# ---- a plain float64 restatement standing in for the device ------------------------------------------------------------------------------
WRONG = ("w", "anchor", "avg_y", "r_first", "factor2", "row-entry", "xprime")
WRONG_RESIDENT = ("last-store", "at-values", "made")  # (of the resident stand-in only)


class LeftToRightIteration(H.HalpernIteration):
    """halpern_reference.HalpernIteration with the resident loop's products: every row of A and of A^T (its own CSR, its own values)
    added up left to right from products rounded once, the projections as the loop's dmin / dmax select"""

    def __init__(self, S, a_values, at_values, *args, **kw):
        self.S, self.a_values, self.at_values = S, np.asarray(a_values, float), np.asarray(at_values, float)
        super().__init__(*args, **kw)
        self.aty = self.at_product(self.y)
        self._anchor()

    def at_product(self, y):
        return ar.rowsums_f64(self.at_values, y, self.S.t_off, self.S.t_rows)

    def operator(self, x, y, aty):
        tau, sigma = self.eta / self.omega, self.eta * self.omega
        nxt = x - tau * (self.c - aty)
        nxt = np.where(nxt < self.ub, nxt, self.ub)
        xp = np.where(nxt > self.lb, nxt, self.lb)
        v = ar.rowsums_f64(self.a_values, xp - x + xp, self.S.off, self.S.idx)
        nxt = y - sigma * v
        with np.errstate(invalid="ignore"):
            low, up = nxt + sigma * self.lo, nxt + sigma * self.hi
        inner = np.where(up < 0.0, up, 0.0)
        yp = np.where(low > inner, low, inner)
        return xp, yp, self.at_product(yp)


class HostStandIn:
    """The same interface on the host.  halpern_reference.HalpernIteration is the arithmetic (its products: scipy's float64 row sums);
    this class only keeps what the device keeps around it -- the ping-pong pairs, XBAR, T(z^k) in the average slots (x' on the last
    step of a run only), the partials (one per sum), the two blocks.  It stands in for the device where the reference and the
    scenario are tested without one; it is no second reference.

    wrong: one of WRONG -- a stand-in that is subtly wrong in one place, for the tests that the rules name the stage:
      "w" the weights from k + 1; "anchor" the anchor term dropped from A^T y^{k+1}; "avg_y" AVG_Y holds y^{k+1}; "r_first" rewritten on
      every step; "factor2" r2 without the factor 2 on the interaction; "row-entry" (with drop=(row, position)) one entry of a row
      missing in the A product; "xprime" x' not stored on a single step.

    resident: the one-workgroup loop in the device's place -- the products of LeftToRightIteration (prob["AT_VALUES"] for A^T), z^k in
    X_OTHER / Y_OTHER behind the last step of a run; nobody asks it for XBAR or the partials.  Wrong in one resident-specific place
    (WRONG_RESIDENT): "last-store" z^k is not stored on the last step of a multi-step run (the other side keeps what the launch found
    there, or the launch's own start where the step count is odd); "at-values" the A^T product takes A_VALUES in A^T's order where
    prob["AT_VALUES"] differs from it; "made" a run that makes no step rewrites AVG_X from its registers (x' = x there)."""

    def __init__(self, S, prob, eta, omega, x, y, wrong=None, drop=None, resident=False):
        assert wrong is None or wrong in WRONG or (resident and wrong in WRONG_RESIDENT)
        self.S, self.prob, self.wrong, self.resident = S, prob, wrong, resident
        import scipy.sparse as sp
        B = sp.csr_matrix((prob["A_VALUES"], S.idx, S.off), shape=(S.m, S.n))
        values = prob["A_VALUES"].copy()
        if wrong == "row-entry":
            values[S.off[drop[0]] + drop[1]] = 0.0  # (the A product alone: the A^T product keeps the entry)
        if resident:
            at_values = prob["A_VALUES"][S.order] if wrong == "at-values" else prob["AT_VALUES"]
            self.it = LeftToRightIteration(S, values, at_values, B, prob["C"], prob["LB"], prob["UB"], prob["LO"], prob["HI"], eta, omega, x=x, y=y)
        else:
            self.it = H.HalpernIteration(B, prob["C"], prob["LB"], prob["UB"], prob["LO"], prob["HI"], eta, omega, x=x, y=y)
            if wrong == "row-entry":
                self.it.B = sp.csr_matrix((values, S.idx, S.off), shape=(S.m, S.n))
        n, m = S.n, S.m
        self.c = dict(step_size=float(eta), primal_weight=float(omega), tau=float(eta) / float(omega), sigma=float(eta) * float(omega), sum_weights=0.0,
                      last_interaction=0.0, last_movement=0.0, last_dx2=0.0, last_dy2=0.0, k=0, cur=0, pending_avg=0, steps_taken=0, attempts=0,
                      target_steps=0, error=0, its_since_restart=0)
        self.h = dict(r=0.0, r_first=0.0, r2=0.0, r2_min=np.inf, k=0)
        self.other = dict(X=np.zeros(n), Y=np.zeros(m), ATY=np.zeros(n))
        self.v = dict(XBAR=np.zeros(n), SUM_X=np.zeros(n), SUM_Y=np.zeros(m), AVG_X=np.zeros(n), AVG_Y=np.zeros(m), PART_A=np.zeros(1), PART_AT=np.zeros(2))

    def ctl(self):
        return dict(self.c)

    def hal(self):
        return dict(self.h)

    def get(self, name):
        it = self.it
        cur = dict(X=it.x, Y=it.y, ATY=it.aty, LAST_RESTART_X=it.x0, LAST_RESTART_Y=it.y0, LAST_RESTART_ATY=it.aty0)
        if name in cur:
            return cur[name].copy()
        if name.endswith("_OTHER"):
            return self.other[name[:-6]].copy()
        return (self.prob[name] if name in self.prob else self.v[name]).copy()

    def put(self, name, a):
        setattr(self.it, dict(X="x", Y="y")[name], np.array(a, float))

    def run(self, target):
        self.c["target_steps"] = target
        found, start, made = dict(self.other), dict(X=self.it.x, Y=self.it.y), 0
        while self.c["error"] == 0 and self.c["steps_taken"] < target:
            self._step(self.c["steps_taken"] + 1 >= target)
            made += 1
        if self.wrong == "last-store" and made > 1:  # (the final store goes to the side the start came from where `made` is even)
            self.other.update({k: (start if made & 1 else found)[k] for k in ("X", "Y")})
        if self.wrong == "made" and made == 0:
            self.v["AVG_X"] = self.it.x.copy()

    def _step(self, last):
        it, c, h, v, wrong = self.it, self.c, self.h, self.v, self.wrong
        x, y, aty, k = it.x, it.y, it.aty, it.k
        xp, yp, atyp = it.operator(x, y, aty)  # (what step() is about to form again, bit for bit: here for the three sums)
        dx, dy, t = xp - x, yp - y, atyp - aty
        with np.errstate(all="ignore"):
            dy2, inter, dx2 = float(dy @ dy), float(dx @ t), float(dx @ dx)
            r2 = float(it.step())  # THE ARITHMETIC: T(z^k), r2 in PDHG's metric, the combination
        if wrong == "factor2":
            r2 = float((it.omega / it.eta) * (dx @ dx) + (dx @ t) + (dy @ dy) / (it.eta * it.omega))
        if wrong == "w":
            w = (k + 2.0) / (k + 3.0)
            it.x, it.y, it.aty = (w * (2.0 * a - b) + (1.0 - w) * z for a, b, z in ((xp, x, it.x0), (yp, y, it.y0), (atyp, aty, it.aty0)))
        if wrong == "anchor":
            it.aty = ((k + 1.0) / (k + 2.0)) * (2.0 * atyp - aty)
        self.other = dict(X=x, Y=y, ATY=aty)
        v["XBAR"], v["AVG_Y"] = xp - x + xp, (it.y.copy() if wrong == "avg_y" else yp)
        if last and wrong != "xprime":
            v["AVG_X"] = xp
        v["PART_A"], v["PART_AT"] = np.array([dy2]), np.array([inter, dx2])
        c.update(last_interaction=inter, last_movement=r2, last_dx2=dx2, last_dy2=dy2, attempts=c["attempts"] + 1)
        if r2 != r2 or not r2 < hr.OVERFLOW:
            c["error"] = 1
            it.k = k  # (hal keeps every field)
        else:
            r = float(np.sqrt(max(r2, 0.0)))
            h.update(r=r, r2=r2, r_first=(r if k == 0 or wrong == "r_first" else h["r_first"]), r2_min=min(h["r2_min"], r2), k=k + 1)
        c.update(k=c["k"] + 1, cur=c["cur"] ^ 1, steps_taken=c["steps_taken"] + 1, its_since_restart=c["its_since_restart"] + 1)

    def halpern_restart(self, theta):
        it, c = self.it, self.c
        dist = it.restart(theta)
        c.update(primal_weight=it.omega, tau=c["step_size"] / it.omega, sigma=c["step_size"] * it.omega, its_since_restart=0)
        self.h["k"] = 0
        return float(dist[0]), float(dist[1])


def stand_in(p, x0, y0, dr, dc, wrong=None, drop=None, resident=False, at_entry=None):
    """the GPU test's set-up on the host: the LP scaled with (dr, dc) as pdlpdev_scale_problem scales it, eta = STEP_SAFETY / sigma_max
    by the restatement's power iteration, omega = ||c|| / ||b||, the start scaled and projected, A^T y formed, the start its own anchor
    -> (HostStandIn, Structure, the scaled problem).  resident: the resident stand-in; the problem then carries AT_VALUES, A^T's entries
    multiplied by D_c first and D_r second as pdlpdev_scale_problem multiplies them (so some differ from A's in their last bit).
    at_entry: that entry of AT_VALUES is instead one ulp above A's value -- the one difference of the "at-values" case."""
    S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
    prob = dict(A_VALUES=np.asarray(p["values"], float) * dr[S.rows] * dc[S.idx], C=p["c"] * dc, LB=p["lb"] / dc, UB=p["ub"] / dc, LO=p["lo"] * dr,
                HI=p["hi"] * dr)
    if resident:
        prob["AT_VALUES"] = (np.asarray(p["values"], float)[S.order] * dc[S.idx[S.order]]) * dr[S.t_rows]
        if at_entry is not None:
            prob["AT_VALUES"] = prob["A_VALUES"][S.order].copy()
            prob["AT_VALUES"][at_entry] = np.nextafter(prob["AT_VALUES"][at_entry], np.inf)
    import scipy.sparse as sp
    sigma = H.power_iteration(sp.csr_matrix((prob["A_VALUES"], S.idx, S.off), shape=(S.m, S.n)))[0]
    eta = H.STEP_SAFETY / sigma if sigma > 0 else 1.0
    dev = HostStandIn(S, prob, eta, H.initial_weight(prob["C"], prob["LO"], prob["HI"]), np.asarray(x0, float) / dc, np.asarray(y0, float) / dr, wrong, drop,
                      resident)
    return dev, S, prob
