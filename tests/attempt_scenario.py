"""TEST UTILITY: the scenario that tests/test_attempt_layouts_gpu.py runs on the device and tests/test_attempt_reference.py on a plain
float64 stand-in, checked stage by stage with tests/attempt_reference.py.  numpy only.

`dev` is anything with ctl() -> control block, get(buffer name) -> array, attempt() (ONE attempt, no make-up round), flush(),
make_average(mode), restart(which, unscaled) -> the two squared distances, set_step(step, weight), compute_aty(), put(buffer name,
array) -- and, for the resident small-LP path's further cases (edge_attempts, check_composition: tests/test_resident_attempts_gpu.py),
attempts(count) (at most `count` attempts towards steps_taken + count in one go) and run(target) (attempts until `target` steps)."""
import numpy as np

import attempt_reference as ar
from eval_reference import _segment_sums

INF = np.inf
RATIOS = ("y", "aty", "dy2", "dx2", "inter", "dist")
NATURAL_ATTEMPTS = 8
MIN_MARGIN_GAP = 1e-6   # every natural decision has |step / limit - 1| at least this: it is decided, not a near tie
FORCED_FACTOR = 64.0    # the forced rejection multiplies the step by this ...
FORCED_MARGIN = 2.0     # ... and must then have step / limit at least this
FORCED_TARGET = 4.0     # what force_rejection() aims step / limit at


def snapshot(dev, xbar=False):
    out = {k: dev.get(k) for k in ar.STATE + (("XBAR",) if xbar else ())}
    out["ctl"] = ar.ctl_dict(dev.ctl())
    return out


def download_problem(dev):
    return {k: dev.get(k) for k in ar.PROBLEM}


class Worst(dict):
    def __init__(self):
        super().__init__({k: 0.0 for k in RATIOS})

    def take(self, ratios):
        for k, v in ratios.items():
            self[k] = max(self[k], v)

    def line(self, name):
        return "WORST %s " % name + " ".join("%s=%.3g" % (k, self[k]) for k in RATIOS)


def one_attempt(dev, S, prob, sp, tag, worst=None, record=None, resident=False):
    """one attempt through the hook, checked fully against the state in front of it -> (result, before, after); resident: by the rules
    of the resident small-LP path, on which XBAR is never written"""
    before = snapshot(dev)
    dev.attempt()
    after = snapshot(dev, xbar=not resident)
    r = ar.check_attempt(S, prob, sp, before, after, tag, resident=resident)
    if worst is not None:
        worst.take(r["ratios"])
    if record is not None:
        record.append(after)
    return r, before, after


def assert_decided(r, tag):
    assert r["error"] == 0 and abs(r["margin"] - 1.0) >= MIN_MARGIN_GAP, (tag, "a near tie: take another seed", r["margin"])


def natural_attempts(dev, S, prob, sp, tag, worst, record=None, count=NATURAL_ATTEMPTS, resident=False):
    """step 2: `count` single attempts, each checked; both cur parities accepted from, both pending_avg states seen"""
    seen = []
    for i in range(count):
        r = one_attempt(dev, S, prob, sp, "%s attempt %d" % (tag, i), worst, record, resident)[0]
        assert_decided(r, "%s attempt %d" % (tag, i))
        seen.append(r)
    assert {r["cur_before"] for r in seen if r["accepted"]} == {0, 1}, (tag, "accepted from both sides of the ping-pong pairs", seen)
    assert {r["pending_before"] for r in seen} == {0, 1}, (tag, "attempts with and without a pending average", seen)
    return seen


def check_flush(dev, tag):
    st = snapshot(dev)
    sx, sy = ar.flush(st["ctl"], st)
    dev.flush()
    after = snapshot(dev)
    assert ar.bits_equal(after["SUM_X"], sx) and ar.bits_equal(after["SUM_Y"], sy), (tag, "flush_average", st["ctl"]["pending_avg"])
    assert after["ctl"]["pending_avg"] == 0, (tag, "pending_avg behind the flush")
    for k in ("X", "Y", "ATY"):
        assert ar.bits_equal(after[k], st[k]), (tag, "the flush changed", k)
    return after


def check_restart(dev, which, unscaled, dr, dc, tag, worst):
    st = snapshot(dev)
    lrx, lry = dev.get("LAST_RESTART_X"), dev.get("LAST_RESTART_Y")
    cx, cy = (dev.get("AVG_X"), dev.get("AVG_Y")) if which == ar.AVERAGE else (st["X"], st["Y"])
    dist = dev.restart(which, unscaled)
    ref, exact = ar.restart(which, unscaled, cx, cy, lrx, lry, dc, dr)
    assert float(ref[0][0]) > 0.0 and float(ref[1][0]) > 0.0, (tag, "the restart moved nothing")
    ratio = max(ar.scalar_ratio(ref[0], dist[0], exact), ar.scalar_ratio(ref[1], dist[1], exact))
    worst.take(dict(dist=ratio))
    assert ratio <= 1.0, (tag, "dist2 outside its bound", ratio, list(dist), [float(v[0]) for v in ref])
    after = snapshot(dev)
    for got, want, what in ((after["X"], cx, "X"), (after["Y"], cy, "Y"), (dev.get("LAST_RESTART_X"), cx, "anchor x"),
                            (dev.get("LAST_RESTART_Y"), cy, "anchor y"), (after["SUM_X"], np.zeros_like(cx), "SUM_X"),
                            (after["SUM_Y"], np.zeros_like(cy), "SUM_Y")):
        assert ar.bits_equal(got, want), (tag, "restart", what)
    want = dict(st["ctl"], sum_weights=0.0, its_since_restart=0, pending_avg=0)
    assert after["ctl"] == want, (tag, "the control block behind the restart", after["ctl"], want)
    return after


def force_rejection(dev, S, prob, sp, held, name, recoverable=False):
    """set_step(64 step, w) alone does not force a rejection with step / limit >= 2 on any LP: the limit of a consistent state grows
    with the step (for dy = -2 sigma A dx the limit is |dx|^2 / (4 step |A dx|^2) + step), so step / limit tends to 1 from either side
    -- 1.005, 1.022, 1.014, 0.994 (accepted!) and 1.003 on the five LPs here, at most 1.8 over a grid of steps and weights.  What
    rejects far from a tie is a STALE A^T y.  So, behind set_step(64 step, w), the dual iterate is moved off the A^T y the device
    holds: Y + beta z through the upload hook, z = +-(A dx) on the equality rows (where the projection is the identity, so that dy and
    the movement stay what they were) and 0 elsewhere, dx the primal move this attempt is going to make (k_primal never reads y).  The
    interaction moves by beta (A dx).z, and beta is sized with the reference so that step / limit becomes FORCED_TARGET.  The attempt
    kernels are functions of the buffers they are handed; the reference is handed the same ones.  -> the Y to put back afterwards

    recoverable: for a whole RUN behind the displacement, in the middle of which nobody can put Y back.  While Y sits off the A^T y
    the device holds, the interaction keeps the term beta z.(A dx), which shrinks only like the step while the movement shrinks like its
    square: with z = A dx, step / limit tends to a constant far above 1 as the rejections shorten the step (10 ... 1e5 on the resident
    tests' LPs) and nothing is accepted until the movement underflows.  So z is taken orthogonal, on the equality rows, to A d, d the
    direction every SHORT primal move has (-(c - A^T y) on the columns that do not push into a bound they sit on): the term is there at
    the long step, which is rejected at step / limit = 4 all the same, and gone once the step is short, where an attempt is accepted
    and forms A^T y afresh."""
    dev.set_step(FORCED_FACTOR * held["ctl"]["step_size"], held["ctl"]["primal_weight"])
    st = snapshot(dev)
    c = st["ctl"]
    assert c["step_size"] == FORCED_FACTOR * held["ctl"]["step_size"] and c["tau"] == c["step_size"] / c["primal_weight"], c
    p = ar.primal(prob, c, st)
    d = ar.dual(S, prob, c, st, p["xbar"])
    a = ar.aty_product(S, prob, d["y"])
    s = ar.step_sums(st, p["xn"], d["y"], a["aty"])
    dec = ar.decision(c, float(s["dy2"][0]), float(s["inter"][0]), float(s["dx2"][0]), sp)
    inter0, movement = float(s["inter"][0]), dec["ctl"]["last_movement"]
    adx = _segment_sums(prob["A_VALUES"] * (p["xn"] - st["X"])[S.idx], S.off, np.zeros(S.m))
    z = np.where(np.isfinite(prob["LO"]) & (prob["LO"] == prob["HI"]), adx, 0.0)
    if recoverable:
        gradient = prob["C"] - st["ATY"]
        short = np.where(((st["X"] <= prob["LB"]) & (gradient > 0.0)) | ((st["X"] >= prob["UB"]) & (gradient < 0.0)), 0.0, -gradient)
        ad = np.where(z != 0.0, _segment_sums(prob["A_VALUES"] * short[S.idx], S.off, np.zeros(S.m)), 0.0)
        z = z - (float(np.sum(z * ad)) / float(np.sum(ad * ad))) * ad
    gain = float(np.sum(z * adx))
    assert gain > 0.0 and movement > 0.0, (name, "no equality row moves", gain, movement)
    beta = (FORCED_TARGET * movement / c["step_size"] - abs(inter0)) / gain
    assert beta > 0.0, (name, "64 x step rejects at the target margin by itself", dec["margin"])
    dev.put("Y", st["Y"] + (-beta if inter0 < 0.0 else beta) * z)
    return st["Y"]


def run_scenario(dev, S, prob, sp, dr, dc, name, resident=False):
    """steps 2 .. 5 on a context prepared by step 1 -> Worst"""
    worst = Worst()
    natural_attempts(dev, S, prob, sp, name, worst, resident=resident)
    # 3. a forced rejection: no average pending, a step 64 times too long and the dual iterate moved off its A^T y (force_rejection)
    held = check_flush(dev, name + " flush")
    y_kept = force_rejection(dev, S, prob, sp, held, name)
    held = snapshot(dev)
    r, before, after = one_attempt(dev, S, prob, sp, name + " forced rejection", worst, resident=resident)
    assert not r["accepted"] and r["margin"] >= FORCED_MARGIN, (name, "the forced rejection", r)
    assert (after["ctl"]["cur"], after["ctl"]["steps_taken"], after["ctl"]["pending_avg"]) == (held["ctl"]["cur"], held["ctl"]["steps_taken"], 0), after["ctl"]
    for k in ("X", "Y", "ATY", "SUM_X", "SUM_Y"):
        assert ar.bits_equal(after[k], held[k]), (name, "the rejected attempt changed", k)
    dev.put("Y", y_kept)
    for i in range(6):  # (the step behind a rejection at margin 4 is still several times the one the iteration had reached)
        r, before, after = one_attempt(dev, S, prob, sp, "%s behind the rejection %d" % (name, i), worst, resident=resident)
        assert_decided(r, "%s behind the rejection %d" % (name, i))
        assert r["pending_before"] == 0 and ar.bits_equal(after["SUM_X"], held["SUM_X"]) and ar.bits_equal(after["SUM_Y"], held["SUM_Y"]), (name, "sums behind the rejection")
        if r["accepted"]:  # (an accepted step is what steps 4 and 5 average and restart from)
            break
    assert r["accepted"], (name, "no accepted step behind the forced rejection", r)
    # 4. the flush with an average pending, the three averages
    assert snapshot(dev)["ctl"]["pending_avg"] == 1
    st = check_flush(dev, name + " flush, pending")
    assert st["ctl"]["sum_weights"] > 0.0
    for mode in (0, 1, 2):
        dev.make_average(mode)
        ax, ay = ar.make_average(mode, st["ctl"], st)
        assert ar.bits_equal(dev.get("AVG_X"), ax) and ar.bits_equal(dev.get("AVG_Y"), ay), (name, "make_average", mode)
    assert np.abs(ax - st["X"]).max() > 0.0 and np.abs(ay - st["Y"]).max() > 0.0, (name, "the average is the iterate")
    # 5. restart to the average (scaled distances), two attempts, restart to the current iterate (unscaled distances)
    check_restart(dev, ar.AVERAGE, 0, dr, dc, name + " restart to the average", worst)
    dev.compute_aty()
    st = snapshot(dev)
    a = ar.aty_product(S, prob, st["Y"])
    assert ar.worst_ratio(ar.abs_err(a, st["ATY"]), a["bound"]) <= 1.0, (name, "A^T y behind the restart")
    for i in range(2):
        assert_decided(one_attempt(dev, S, prob, sp, "%s restarted attempt %d" % (name, i), worst, resident=resident)[0], name + " restarted")
    check_restart(dev, ar.CURRENT, 1, dr, dc, name + " restart to the current iterate", worst)
    return worst


# ---- the resident small-LP path's further cases ------------------------------------------------------------------------------------------
CURRENT_SIDE = ("X", "Y", "ATY", "SUM_X", "SUM_Y")
LAUNCH_ATTEMPTS = 12  # attempts of the one launch that is compared with as many single ones
RUN_STEPS = 4         # accepted steps of the run behind the forced rejection
STARTS = ("fresh", "pending", "cur1")  # cur = 0 and nothing pending; two steps on: an average pending; one step and a flush on: cur = 1
EVAL_COMBOS = [(mode, rule, eps) for mode in (0, 1, 2) for rule in (True, False) for eps in (1e-4, -1.0)]


def edge_attempts(dev, S, prob, sp, name, worst, resident=True):
    """NATURAL_ATTEMPTS single attempts, each checked.  On the LPs of one row or one column only what is defined is asserted: an attempt
    that ends in the step error (no movement) is checked like any other, the attempts behind it must leave the control block's
    (error, attempts, steps_taken) and the iterate alone, and no property of the sequence is asked for."""
    if not name.startswith("minimal"):
        return natural_attempts(dev, S, prob, sp, name, worst, resident=resident)
    seen = []
    for i in range(NATURAL_ATTEMPTS):
        if seen and seen[-1]["error"]:
            before = snapshot(dev)
            dev.attempt()
            after = snapshot(dev)
            assert all(after["ctl"][k] == before["ctl"][k] for k in ("error", "attempts", "steps_taken", "cur", "pending_avg", "step_size")), (name, i, after["ctl"])
            assert all(ar.bits_equal(after[k], before[k]) for k in CURRENT_SIDE), (name, i, "an attempt behind the step error wrote")
            continue
        r = one_attempt(dev, S, prob, sp, "%s attempt %d" % (name, i), worst, resident=resident)[0]
        if not r["error"]:
            assert abs(r["margin"] - 1.0) >= MIN_MARGIN_GAP, (name, i, "a near tie: take another seed", r["margin"])
        seen.append(r)
    return seen


def start_state(dev, start):
    """the prepared context moved to one of STARTS"""
    if start == "pending":
        dev.run(2)
    elif start == "cur1":
        dev.run(1)
        dev.flush()
    c = dev.ctl()
    want = dict(fresh=(0, 0, 0), pending=(0, 1, 2), cur1=(1, 0, 1))[start]
    assert (c["cur"], c["pending_avg"], c["steps_taken"]) == want and c["error"] == 0, (start, c)


def _same(a, b, tag, skip=()):
    for k in a["ctl"]:
        assert k in skip or a["ctl"][k] == b["ctl"][k], (tag, "control block", k, a["ctl"][k], b["ctl"][k])
    for k in CURRENT_SIDE:
        assert ar.bits_equal(a[k], b[k]), (tag, k, int(np.argmax(a[k] != b[k])))


def check_composition(make, sp, name, start):
    """A launch is the composition of its attempts.  make() -> (dev, S, prob) prepared afresh, the same state every time.
    (a) attempts(LAUNCH_ATTEMPTS) in one go leaves the current side and the control block bit for bit what as many attempts(1) leave
        (target_steps apart: it is what each call was asked for, steps_taken + count at ITS start);
    (b) behind the scenario's forced rejection (set_step(64 step) and the moved Y in front of both), run(steps_taken + RUN_STEPS) leaves
        them what attempts(1) repeated until that many steps leaves -- target_steps included -- and the run held a rejection.
        (force_rejection(recoverable=True): a displacement of Y that a run gets past by itself.)
    -> (attempts, accepted steps) of (a) and of (b)"""
    tag = "%s from %s" % (name, start)
    ends = []
    for single in (False, True):
        dev = make()[0]
        start_state(dev, start)
        first = dev.ctl()
        if single:
            for _ in range(LAUNCH_ATTEMPTS):
                dev.attempts(1)
        else:
            dev.attempts(LAUNCH_ATTEMPTS)
        ends.append(snapshot(dev))
    _same(ends[0], ends[1], tag + ": one launch against single attempts", skip=("target_steps",))
    c = ends[0]["ctl"]
    counts_a = (c["attempts"] - first["attempts"], c["steps_taken"] - first["steps_taken"])
    assert counts_a[0] == LAUNCH_ATTEMPTS and c["error"] == 0, (tag, c)
    ends = []
    for single in (False, True):
        dev, S, prob = make()
        start_state(dev, start)
        force_rejection(dev, S, prob, sp, snapshot(dev), tag, recoverable=True)
        first = dev.ctl()
        target = first["steps_taken"] + RUN_STEPS
        if single:
            for _ in range(64 * RUN_STEPS):
                if dev.ctl()["steps_taken"] >= target:
                    break
                dev.attempts(1)
        else:
            dev.run(target)
        ends.append(snapshot(dev))
    _same(ends[0], ends[1], tag + ": run against single attempts")
    c = ends[0]["ctl"]
    counts_b = (c["attempts"] - first["attempts"], c["steps_taken"] - first["steps_taken"])
    assert c["error"] == 0 and counts_b[1] == RUN_STEPS and counts_b[0] > counts_b[1], (tag, "the run held no rejection", counts_b)
    return counts_a, counts_b


# ---- a plain float64 restatement standing in for the device ------------------------------------------------------------------------
class HostStandIn:
    """The same interface on the host: float64 throughout, numpy's own summation order.  It stands in for the device where the
    reference and the scenario are tested without one; it is no second reference."""

    def __init__(self, S, prob, sp, x, y, resident=False):
        self.S, self.prob, self.sp, self.resident = S, prob, sp, resident  # resident: rows and columns left to right, as the one-workgroup loop
        self.c = dict(step_size=0.0, primal_weight=1.0, tau=0.0, sigma=0.0, sum_weights=0.0, last_interaction=0.0, last_movement=0.0, last_dx2=0.0,
                      last_dy2=0.0, k=0, cur=0, pending_avg=0, steps_taken=0, attempts=0, target_steps=0, error=0, its_since_restart=0)
        n, m = S.n, S.m
        self.x, self.y, self.aty = [np.array(x, float), np.zeros(n)], [np.array(y, float), np.zeros(m)], [np.zeros(n), np.zeros(n)]
        self.v = dict(XBAR=np.zeros(n), SUM_X=np.zeros(n), SUM_Y=np.zeros(m), AVG_X=np.zeros(n), AVG_Y=np.zeros(m), LAST_RESTART_X=np.zeros(n),
                      LAST_RESTART_Y=np.zeros(m))

    def ctl(self):
        return dict(self.c)

    def get(self, name):
        cur = self.c["cur"]
        pairs = dict(X=self.x, Y=self.y, ATY=self.aty)
        if name in pairs:
            return pairs[name][cur].copy()
        if name.endswith("_OTHER"):
            return pairs[name[:-6]][cur ^ 1].copy()
        return (self.prob[name] if name in self.prob else self.v[name]).copy()

    def put(self, name, a):
        {"X": self.x, "Y": self.y, "ATY": self.aty}[name][self.c["cur"]] = np.array(a, float)

    def set_step(self, step, weight):
        c = self.c
        if step >= 0.0:
            c["step_size"] = step
        c.update(primal_weight=weight, tau=c["step_size"] / weight, sigma=c["step_size"] * weight)

    def _at(self, y):
        S = self.S
        if self.resident:
            return ar.rowsums_f64(self.prob["A_VALUES"][S.order], y, S.t_off, S.t_rows)
        return _segment_sums(self.prob["A_VALUES"][S.order] * y[S.t_rows], S.t_off, np.zeros(S.n))

    def compute_aty(self):
        self.aty[self.c["cur"]] = self._at(self.y[self.c["cur"]])

    def attempt(self):
        self.attempts(1)

    def attempts(self, count):
        self.c["target_steps"] = self.c["steps_taken"] + count
        for _ in range(count):
            self._attempt()

    def run(self, target):
        self.c["target_steps"] = target
        while self.c["error"] == 0 and self.c["steps_taken"] < target:
            self._attempt()

    def _attempt(self):
        c, P, S, v = self.c, self.prob, self.S, self.v
        if c["error"] or c["steps_taken"] >= c["target_steps"]:
            return
        cur = c["cur"]
        x, y, aty = self.x[cur], self.y[cur], self.aty[cur]
        nxt = x - c["tau"] * (P["C"] - aty)
        nxt = np.where(nxt < P["UB"], nxt, P["UB"])
        nxt = np.where(nxt > P["LB"], nxt, P["LB"])
        v["XBAR"] = nxt - x + nxt
        if self.resident:
            ax = ar.rowsums_f64(P["A_VALUES"], v["XBAR"], S.off, S.idx)
        else:
            ax = _segment_sums(P["A_VALUES"] * v["XBAR"][S.idx], S.off, np.zeros(S.m))
        ny = y - c["sigma"] * ax
        with np.errstate(invalid="ignore"):
            low, up = ny + c["sigma"] * P["LO"], ny + c["sigma"] * P["HI"]
        inner = np.where(up < 0.0, up, 0.0)
        ny = np.where(low > inner, low, inner)
        if c["pending_avg"]:
            v["SUM_X"], v["SUM_Y"] = v["SUM_X"] + c["step_size"] * x, v["SUM_Y"] + c["step_size"] * y
        naty = self._at(ny)
        dx, dy = nxt - x, ny - y
        self.c = ar.decision(c, float(np.sum(dy * dy)), float(np.sum((naty - aty) * dx)), float(np.sum(dx * dx)), self.sp)["ctl"]
        if not self.resident or self.c["cur"] != cur:  # (the resident loop's rejected trial iterate never leaves its registers)
            self.x[cur ^ 1], self.y[cur ^ 1], self.aty[cur ^ 1] = nxt, ny, naty

    def flush(self):
        c, v, cur = self.c, self.v, self.c["cur"]
        if c["pending_avg"]:
            v["SUM_X"], v["SUM_Y"] = v["SUM_X"] + c["step_size"] * self.x[cur], v["SUM_Y"] + c["step_size"] * self.y[cur]
        c["pending_avg"] = 0

    def make_average(self, mode):
        v, cur = self.v, self.c["cur"]
        if mode == 0:
            v["AVG_X"], v["AVG_Y"] = self.x[cur].copy(), self.y[cur].copy()
        elif mode == 1:
            v["AVG_X"], v["AVG_Y"] = np.zeros(self.S.n), np.zeros(self.S.m)
        else:
            v["AVG_X"], v["AVG_Y"] = v["SUM_X"] / self.c["sum_weights"], v["SUM_Y"] / self.c["sum_weights"]

    def restart(self, which, unscaled):
        v, cur, dist = self.v, self.c["cur"], []
        for pair, avg, anchor, d in ((self.x, "AVG_X", "LAST_RESTART_X", self.dc), (self.y, "AVG_Y", "LAST_RESTART_Y", self.dr)):
            cand = v[avg].copy() if which == ar.AVERAGE else pair[cur].copy()
            diff = v[anchor] - cand
            if unscaled:
                diff = diff * d
            dist.append(float(np.sum(diff * diff)))
            pair[cur], v[anchor] = cand, cand.copy()
        v["SUM_X"], v["SUM_Y"] = np.zeros(self.S.n), np.zeros(self.S.m)
        self.c.update(sum_weights=0.0, its_since_restart=0, pending_avg=0)
        return np.array(dist)


def stand_in(p, x0, y0, dr, dc, sp, resident=False):
    """step 1 on the host: the LP scaled with (dr, dc) as pdlpdev_scale_problem scales it, the start scaled and projected, the step
    1 / max|A| at weight 1, A^T y formed -> (HostStandIn, Structure, the scaled problem)"""
    S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
    prob = dict(A_VALUES=np.asarray(p["values"], float) * dr[S.rows] * dc[S.idx], C=p["c"] * dc, LB=p["lb"] / dc, UB=p["ub"] / dc, LO=p["lo"] * dr,
                HI=p["hi"] * dr)
    x = np.asarray(x0, float) / dc
    dev = HostStandIn(S, prob, sp, np.minimum(np.maximum(x, prob["LB"]), prob["UB"]), np.asarray(y0, float) / dr, resident)
    dev.dr, dev.dc = dr, dc
    dev.set_step(1.0 / np.abs(prob["A_VALUES"]).max(), 1.0)
    dev.compute_aty()
    return dev, S, prob


# ---- the further cases' LPs ----------------------------------------------------------------------------------------------------------
def uniform_bounds_variants(p):
    """the LP with all lb = 0 and ub = inf (k_primal reads neither array), with only lb uniform, with only ub uniform"""
    n = p["n"]
    return {"both": dict(p, lb=np.zeros(n), ub=np.full(n, INF)), "lb-only": dict(p, lb=np.zeros(n), ub=np.where(p["ub"] < INF, p["ub"], 7.0)),
            "ub-only": dict(p, lb=np.where(p["lb"] > -INF, p["lb"], -2.0), ub=np.full(n, INF))}


def tiny_lp(kind, seed=11, m=40, n=60, density=0.15):
    """40 x 60 (the shape of test_random_lps_gpu.random_lp), c = 0 and y0 = 0 so that x' = x:
    kind "fixed-point": free rows -> y' = y too: movement 0, the step error;  kind "dual-only": equality rows off A x0 -> dy != 0 while
    dx = 0: interaction 0, the step grows by its full factor.  -> (p, x0, y0)"""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, n)) < density
    mask[np.arange(m), rng.integers(0, n, size=m)] = True
    rows, cols = np.nonzero(mask)
    off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    val = rng.standard_normal(len(rows))
    x0 = np.abs(rng.standard_normal(n))
    p = dict(m=m, n=n, offsets=off, indices=cols.astype(np.int32), values=val, c=np.zeros(n), lb=np.zeros(n), ub=np.full(n, 10.0))
    if kind == "fixed-point":
        p.update(lo=np.full(m, -INF), hi=np.full(m, INF))
    else:
        b = np.bincount(rows, weights=val * x0[cols], minlength=m) + 1.0 + rng.random(m)
        p.update(lo=b, hi=b.copy())
    return p, x0, np.zeros(m)


def assert_scalar_branch(kind, r, before, after, sp):
    """what the two scalar branches of apply_step_decision must leave behind ONE attempt on tiny_lp(kind)"""
    cb, ca = before["ctl"], after["ctl"]
    if kind == "fixed-point":
        assert ca["last_movement"] == 0.0 and ca["error"] == 1 and r["error"] == 1, ca
        assert (ca["k"], ca["step_size"], ca["tau"], ca["sigma"]) == (cb["k"], cb["step_size"], cb["tau"], cb["sigma"]), ca
        assert ca["cur"] == cb["cur"] ^ 1 and ca["sum_weights"] == cb["sum_weights"] + cb["step_size"], ca
        assert ar.bits_equal(after["X"], before["X"]) and ar.bits_equal(after["Y"], before["Y"]), "a fixed point moved"
    else:
        assert ca["last_dx2"] == 0.0 and ca["last_dy2"] > 0.0 and ca["last_interaction"] == 0.0, ca
        assert r["accepted"] and ca["error"] == 0 and ca["k"] == cb["k"] + 1, ca
        want = (1.0 + float(ca["k"] + 1) ** -sp["growth_exponent"]) * cb["step_size"]
        assert abs(ca["step_size"] - want) <= ar.STEP_REL * want, (ca["step_size"], want)
