"""TEST UTILITY: one adaptive PDHG attempt, the averaging kernels and the restart restated stage by stage, in the style of
tests/eval_reference.py (whose helpers it uses): numpy only, every sum in np.longdouble (64-bit significand) or in exact rationals
where the platform's long double is no wider than a double.

What it restates is this repository's own device code: k_primal (cuopt_amd/csrc/pdlp_device.hip), DualEpilogue and StepEpilogue
(pdlp_epilogues.hpp), apply_step_decision and restart_block (pdlp_kernels.hpp), k_flush_average (pdlp_device.hip), k_make_average
(pdlp_eval.hip) -- on the SCALED problem as the device holds it (A_VALUES, C, LB, UB, LO, HI downloaded once) and on the state
downloaded IN FRONT of the attempt (the control block, X, Y, ATY, SUM_X, SUM_Y).  Every stage takes the inputs the device itself held
for that stage -- the A product the device's xbar, the A^T product the device's y', the three sums the device's current and trial
vectors, the decision the device's three sums -- so an error never compounds across stages or attempts, and a failure names the
stage.

BIT-EXACT (the library is built with -ffp-contract=off; float64 numpy, the kernel's order of operations):
    x'   = max(min(x - tau (c - aty), ub), lb)          xbar = x' - x + x'
    SUM_X + w x, SUM_Y + w y  when pending_avg was set in front of the attempt (w: the step size held then), untouched otherwise
    the flush, the average (modes 0, 1, 2), the restart's copies
    last_movement = pds w dx2 + (dds / w) dy2, accepted <=> step <= movement / |interaction|, tau = step / w, sigma = step w,
    sum_weights + step -- all from the device's OWN three sums and its own new step.  The new step itself goes through pow():
    libm here, ocml there, compared at rel 1e-14 (the tolerance tests/test_kernels_gpu.py uses for the same pair).

BOUNDED, per element, u = 2^-53, L the row's (column's) length, for ANY summation tree (a lane left to right, a wave's shuffle tree,
long-row partials, the dense segments' share added ahead of the epilogue; Higham, Accuracy and Stability of Numerical Algorithms,
section 4.2):

  the A product.  v^ = fl(sum_k a_ik xbar_k) has |v^ - v| <= (L + 1) u S_i, S_i = sum_k |a_ik xbar_k| (one rounding per product,
  at most L per term for the tree and the dense share).  DualEpilogue then forms, with N = y - sigma v,
      next = fl(y - fl(sigma v^))            |next - N|  <= sigma |v^ - v| + u sigma |v| + u (|y| + sigma |v|)
      low  = fl(next + fl(sigma lo))         |low - Lo|  <= |next - N| + u sigma |lo| + u (|y| + sigma |v| + sigma |lo|)
  (the same for up with hi), first order in u, and y' = max(low, min(up, 0)).  max and min are exact, and for h = max or min
  |h(a^, b^) - h(a, b)| <= the larger error of the two arguments SELECTED (by the computed and by the exact evaluation): so
      |y'_i - ref_i| <= sigma (L_i + 16) u S_i + 8 u (|y_i| + sigma |v_i| + sigma |b_i|)
  with b_i the finite row bound of the selected branch (0 for the branch "0" and for an infinite bound); 2, 3 and 2 roundings on the
  three terms and L + 1 on the first, the rest is spare for the second order.  The projection is 1-Lipschitz in v, so there is no
  tie in v -- but low and up carry INDEPENDENT roundings of sigma lo and sigma hi, so where the exact evaluation is itself within the
  bound of switching branch (|Lo - min(Up, 0)| or |Up| below the bound taken with the larger |bound| of the row: `branch_tie`) the
  device may select the other one, and b_i is the larger of the row's finite |bounds| there.  Elsewhere both select the same branch.

  the A^T product, from the device's own y':  |got_j - (A^T y')_j| <= (L_j + 16) u sum_i |a_ij y'_i|.

  the three sums, from the device's own current and trial vectors (dy = fl(y' - y) is one rounding of the exact difference, its
  square two more, a tree over N terms at most N - 1 per term):
      |dy2 - sum dy_i^2| <= (m + 16) u sum dy_i^2      |dx2 - sum dx_j^2| <= (n + 16) u sum dx_j^2
      |interaction - sum t_j dx_j| <= (n + 16) u sum |t_j dx_j|,  t = A^T y' - A^T y       (absolute: the sum may cancel)
  the restart's squared distances likewise: within (N + 16) u of the sum of the squared terms d_i = (anchor_i - candidate_i) [D_i].

The reference's own error is at most N 2^-64 of the same magnitude sums (1/2048 of a bound).  The bounds are derived, not measured:
a layout that exceeds one is a finding.

THE RESIDENT SMALL-LP PATH (check_attempt(resident=True); resident_body, cuopt_amd/csrc/kernels_resident.hip).  There every row and
column is added up by its owning lane left to right in float64 from products rounded once (lds_row_sum), so MORE is bit for bit:
    x', SUM_X, SUM_Y as above
    y'      = dual_f64(prob, ctl, st, rowsums_f64(A, xbar)), xbar the reference's own (bit-exact from x')
    A^T y'  = rowsums_f64(A^T, y'), A^T in the stable transposition of A (Structure.order) with the values the device holds for it
              (prob["AT_VALUES"]: scaling multiplies A by D_r then D_c and A^T by D_c then D_r, so an entry of the two may differ in
              its last bit; without that key A_VALUES in that order); an empty column is exactly 0
The three sums go through block_sum_fast's fixed tree, which is not left to right: they keep the bounds above, and are taken from the
reference's own trial vectors (which the device's equal bit for bit).  The decision and everything behind it is unchanged.  What can be
looked at differs: an ACCEPTED attempt leaves its trial iterate as the new current side; a REJECTED one writes nothing but the
control block and the running sums (the trial iterate never leaves the registers: the other side is stale and not read), so X, Y and
ATY must be the bits in front of the attempt, SUM_X / SUM_Y too unless an average was pending.  XBAR is never written there.

THE SHARDED PATH (tests/test_sharded_attempts_gpu.py: W ranks' buffers assembled to the global vectors by tests/sharded_ranks.py, then
check_attempt as it stands).  No bound above is widened, because none needs to be:
    the ranks' partial products of a column, added in rank order (the all-reduce, the reduce-scatter), are one more summation tree
    over the same L_j terms, and a rank without an entry in the column contributes an exact 0: (L_j + 16) u sum |a_ij y'_i| holds for
    A^T y' under all three dataflows.  The owner-computes column block sums a whole column on one rank: a tree like any other.
    dy2, dx2, the interaction and the restart's distances are sums of per-rank (per-slice) partials over the same m or n terms.
    An entry of the column block, or of a rank's A^T, is scaled (a D_c) D_r where A_VALUES holds (a D_r) D_c: it may differ in its last
    bit, which is one of the 16 spare roundings per term.
    x', xbar, SUM_X, SUM_Y, the flush, the three averages, the restart's copies and everything derived from the device's own three
    sums are element-wise or scalar work on values every rank holds alike: bit for bit, as on one GPU.
A ratio above 1.0 there is a finding about the kernel concerned, not a reason to touch a bound."""
import math

import numpy as np

from eval_reference import LONGDOUBLE_IS_EXTENDED, U, _down, _finite_part, _lift, _segment_sums, worst_ratio

CTL_FIELDS = ("step_size", "primal_weight", "tau", "sigma", "sum_weights", "last_interaction", "last_movement", "last_dx2", "last_dy2",
              "k", "cur", "pending_avg", "steps_taken", "attempts", "target_steps", "error", "its_since_restart")
STATE = ("X", "Y", "ATY", "X_OTHER", "Y_OTHER", "ATY_OTHER", "SUM_X", "SUM_Y")
PROBLEM = ("A_VALUES", "C", "LB", "UB", "LO", "HI")
STEP_REL = 1e-14  # pow() of libm against ocml
CURRENT, AVERAGE = 0, 1


def ctl_dict(c):
    """a control block (any object with pdlpdev_ctl's fields, or a dict) as a dict of Python numbers"""
    if isinstance(c, dict):
        return dict(c)
    return {f: (float(getattr(c, f)) if i < 9 else int(getattr(c, f))) for i, f in enumerate(CTL_FIELDS)}


class Structure:
    """the sparsity pattern of A, and of A^T as a stable sort by column (rows ascending inside a column)"""

    def __init__(self, m, n, offsets, indices):
        self.m, self.n = int(m), int(n)
        self.off, self.idx = np.asarray(offsets, dtype=np.int64), np.asarray(indices, dtype=np.int64)
        self.rows = np.repeat(np.arange(self.m), np.diff(self.off))
        self.order = np.argsort(self.idx, kind="stable")
        self.t_off = np.concatenate([[0], np.cumsum(np.bincount(self.idx, minlength=self.n))]).astype(np.int64)
        self.t_rows = self.rows[self.order]
        self.len_r, self.len_c = np.diff(self.off), np.diff(self.t_off)


def bits_equal(a, b):
    """the same float64 bits (so -0.0 is not 0.0), element by element"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


def _dmin(a, b):
    return np.where(a < b, a, b)  # a < b ? a : b


def _dmax(a, b):
    return np.where(a > b, a, b)  # a > b ? a : b


def _exact(exact):
    exact = (not LONGDOUBLE_IS_EXTENDED) if exact is None else exact
    assert exact or np.finfo(np.longdouble).eps <= 2.0 ** -63
    return exact


# ---- the stages of one attempt --------------------------------------------------------------------------------------------------
def primal(prob, ctl, st):
    """k_primal in float64: x', xbar and SUM_X behind it"""
    x, tau = st["X"], np.float64(ctl["tau"])
    gradient = prob["C"] - st["ATY"]
    nxt = x - (tau * gradient)
    nxt = _dmax(_dmin(nxt, prob["UB"]), prob["LB"])
    xbar = nxt - x + nxt
    sumx = st["SUM_X"] + np.float64(ctl["step_size"]) * x if ctl["pending_avg"] else st["SUM_X"].copy()
    return dict(xn=nxt, xbar=xbar, sumx=sumx)


def dual(S, prob, ctl, st, xbar, exact=None):
    """DualEpilogue behind A xbar: y' in extended precision (`y`: rounded to double, `_ext`: for abs_err) with its bound per row,
    branch_tie, and SUM_Y behind it (float64, bit-exact)"""
    exact = _exact(exact)
    val, xb, y = _lift(prob["A_VALUES"], exact), _lift(xbar, exact), _lift(st["Y"], exact)
    zm = _lift(np.zeros(S.m), exact)
    sigma = _lift([ctl["sigma"]], exact)[0]
    prod = val * xb[S.idx]
    v, absv = _segment_sums(prod, S.off, zm), _segment_sums(np.abs(prod), S.off, zm)
    (lo_f, lo), (hi_f, hi) = _finite_part(prob["LO"], exact), _finite_part(prob["HI"], exact)
    nxt = y - sigma * v
    low, up = nxt + sigma * lo, nxt + sigma * hi
    inner_is_up = hi_f & (up < 0)                      # dmin(up, 0.0); up = +inf selects 0
    inner = np.where(inner_is_up, up, zm)
    outer_is_low = lo_f & (low > inner)                # dmax(low, inner); low = -inf selects inner
    ref = np.where(outer_is_low, low, inner)
    abs_lo, abs_hi = np.where(lo_f, np.abs(lo), zm), np.where(hi_f, np.abs(hi), zm)
    b_pick = np.where(outer_is_low, abs_lo, np.where(inner_is_up, abs_hi, zm))
    b_max = np.maximum(abs_lo, abs_hi)

    def bound(b):
        return _down(sigma * absv) * (S.len_r + 16) * U + 8 * U * _down(np.abs(y) + sigma * np.abs(v) + sigma * b)
    wide = bound(b_max)
    wide_e = _lift(wide, exact)
    tie = (lo_f & (np.abs(low - inner) <= wide_e)) | (hi_f & (np.abs(up) <= wide_e))
    tie = np.asarray(tie, dtype=bool)
    sumy = st["SUM_Y"] + np.float64(ctl["step_size"]) * st["Y"] if ctl["pending_avg"] else st["SUM_Y"].copy()
    return dict(y=_down(ref), bound=np.where(tie, wide, bound(b_pick)), branch_tie=tie, sumy=sumy, absv=_down(absv), _ext=ref, _exact=exact)


def rowsums_f64(values, vec, off, idx):
    """float64 row sums, every row left to right from 0.0 with one rounding per product: the order of the C oracle's orc_spmv and of a
    lane on the device's short-row paths -- what the bit-for-bit comparisons with the oracle use in place of the extended sums"""
    off, idx = np.asarray(off, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    prod = np.asarray(values, dtype=np.float64) * np.asarray(vec, dtype=np.float64)[idx]
    lens, acc = np.diff(off), np.zeros(len(off) - 1)
    for k in range(int(lens.max()) if len(lens) else 0):
        r = np.nonzero(lens > k)[0]
        acc[r] = acc[r] + prod[off[r] + k]
    return acc


def dual_f64(prob, ctl, st, v):
    """DualEpilogue's element-wise part in float64 from a row sum v = (A xbar)_i GIVEN"""
    sigma = np.float64(ctl["sigma"])
    nxt = st["Y"] - (sigma * v)
    with np.errstate(invalid="ignore"):
        low, up = nxt + sigma * prob["LO"], nxt + sigma * prob["HI"]
    return _dmax(low, _dmin(up, np.float64(0.0)))


def aty_product(S, prob, y_new, exact=None):
    """A^T y' from the device's own y': extended value and bound per column"""
    exact = _exact(exact)
    val, ye = _lift(prob["A_VALUES"], exact), _lift(y_new, exact)
    zn = _lift(np.zeros(S.n), exact)
    prod = val[S.order] * ye[S.t_rows]
    v, absv = _segment_sums(prod, S.t_off, zn), _segment_sums(np.abs(prod), S.t_off, zn)
    return dict(aty=_down(v), bound=(S.len_c + 16) * U * _down(absv), _ext=v, _exact=exact)


def abs_err(ref, got):
    """|got - ref| per element against the extended value of dual() / aty_product()"""
    return _down(np.abs(_lift(got, ref["_exact"]) - ref["_ext"]))


def step_sums(st, x_new, y_new, aty_new, exact=None):
    """StepEpilogue's and DualEpilogue's reductions from the device's own vectors: (value, bound) of dy2, dx2, interaction"""
    exact = _exact(exact)
    dy = _lift(y_new, exact) - _lift(st["Y"], exact)
    dx = _lift(x_new, exact) - _lift(st["X"], exact)
    t = _lift(aty_new, exact) - _lift(st["ATY"], exact)
    m, n = len(dy), len(dx)
    dy2, dx2, inter, absinter = (dy * dy).sum(), (dx * dx).sum(), (t * dx).sum(), np.abs(t * dx).sum()
    return dict(dy2=(dy2, (m + 16) * U * float(dy2)), dx2=(dx2, (n + 16) * U * float(dx2)), inter=(inter, (n + 16) * U * float(absinter)),
                _exact=exact)


def scalar_ratio(entry, got, exact):
    """|got - value| / bound of one (value, bound) pair of step_sums() / restart(): 0 / 0 is 0, an error above a zero bound infinite"""
    value, bound = entry
    err = float(abs(_lift([got], exact)[0] - value))
    return 0.0 if err == 0.0 else (err / bound if bound > 0.0 else math.inf)


def decision(ctl, dy2, interaction, dx2, sp):
    """apply_step_decision in float64 from the three sums GIVEN: the control block behind the attempt plus `accepted`, `limit` and
    `margin` = step / limit (the decision is accepted <=> margin <= 1; nan on the error path)"""
    c = dict(ctl)
    w, step = ctl["primal_weight"], ctl["step_size"]
    movement = sp["primal_distance_smoothing"] * w * dx2 + (sp["dual_distance_smoothing"] / w) * dy2
    c.update(last_interaction=interaction, last_movement=movement, last_dx2=dx2, last_dy2=dy2, attempts=ctl["attempts"] + 1)
    limit, margin = math.nan, math.nan
    if not (movement > 0.0) or not (movement < 1.0e100) or interaction != interaction:
        c["error"], accepted = 1, True
    else:
        inter = abs(interaction)
        c["k"] = ctl["k"] + 1
        kc = float(c["k"])
        limit = movement / inter if inter > 0.0 else math.inf
        accepted = step <= limit
        margin = step / limit
        s1 = (1.0 - math.pow(kc + 1.0, -sp["reduction_exponent"])) * limit
        s2 = (1.0 + math.pow(kc + 1.0, -sp["growth_exponent"])) * step
        step = s1 if s1 < s2 else s2
        c.update(step_size=step, tau=step / w, sigma=step * w)
    if accepted:
        c.update(cur=ctl["cur"] ^ 1, pending_avg=1, sum_weights=ctl["sum_weights"] + step, steps_taken=ctl["steps_taken"] + 1,
                 its_since_restart=ctl["its_since_restart"] + 1)
    else:
        c["pending_avg"] = 0
    return dict(ctl=c, accepted=accepted, limit=limit, margin=margin)


# ---- the averaging kernels and the restart -----------------------------------------------------------------------------------------
def flush(ctl, st):
    """k_flush_average + k_clear_pending: (SUM_X, SUM_Y) behind them; pending_avg is 0 afterwards"""
    if not ctl["pending_avg"]:
        return st["SUM_X"].copy(), st["SUM_Y"].copy()
    w = np.float64(ctl["step_size"])
    return st["SUM_X"] + w * st["X"], st["SUM_Y"] + w * st["Y"]


def make_average(mode, ctl, st):
    """k_make_average: mode 0 the current iterate, 1 zero, 2 sum / sum_weights"""
    if mode == 0:
        return st["X"].copy(), st["Y"].copy()
    if mode == 1:
        return np.zeros_like(st["X"]), np.zeros_like(st["Y"])
    sw = np.float64(ctl["sum_weights"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return st["SUM_X"] / sw, st["SUM_Y"] / sw


def restart(which, unscaled, cand_x, cand_y, anchor_x, anchor_y, dc, dr, exact=None):
    """restart_block's two squared distances: [(value, bound) primal, (value, bound) dual]; the candidate (the average, or the current
    iterate) is what iterate and anchors hold afterwards, the sums are zero"""
    exact = _exact(exact)
    out = []
    for cand, anchor, d in ((cand_x, anchor_x, dc), (cand_y, anchor_y, dr)):
        diff = _lift(anchor, exact) - _lift(cand, exact)
        if unscaled:
            diff = diff * _lift(d, exact)
        s = (diff * diff).sum() if len(cand) else _lift([0.0], exact)[0]
        out.append((s, (len(cand) + 16) * U * float(s)))
    return out, exact


# ---- one whole attempt checked against the state in front of it --------------------------------------------------------------------
def _check_decision(tag, cb, ca, flipped, sp):
    """(5) the decision, from the device's own three sums"""
    dec = decision(cb, ca["last_dy2"], ca["last_interaction"], ca["last_dx2"], sp)
    want = dec["ctl"]
    assert ca["last_movement"] == want["last_movement"], (tag, "movement", ca["last_movement"], want["last_movement"])
    for k in ("k", "attempts", "steps_taken", "its_since_restart", "cur", "pending_avg", "error"):
        assert ca[k] == want[k], (tag, k, ca[k], want[k], dec["margin"])
    assert flipped == dec["accepted"], (tag, "accepted", dec["margin"])
    assert abs(ca["step_size"] - want["step_size"]) <= STEP_REL * abs(want["step_size"]), (tag, "step_size", ca["step_size"], want["step_size"])
    assert ca["primal_weight"] == cb["primal_weight"], (tag, "primal_weight")
    if want["error"] == 0:  # (the error path leaves step, tau and sigma alone)
        assert ca["tau"] == ca["step_size"] / cb["primal_weight"] and ca["sigma"] == ca["step_size"] * cb["primal_weight"], (tag, "tau / sigma")
    else:
        assert (ca["step_size"], ca["tau"], ca["sigma"]) == (cb["step_size"], cb["tau"], cb["sigma"]), (tag, "step on the error path")
    assert ca["sum_weights"] == (cb["sum_weights"] + ca["step_size"] if dec["accepted"] else cb["sum_weights"]), (tag, "sum_weights")
    return dec, want


def _check_sums(tag, s, ca, ratios):
    """(4) the three sums against (value, bound) of step_sums()"""
    ratios.update(dy2=scalar_ratio(s["dy2"], ca["last_dy2"], s["_exact"]), dx2=scalar_ratio(s["dx2"], ca["last_dx2"], s["_exact"]),
                  inter=scalar_ratio(s["inter"], ca["last_interaction"], s["_exact"]))
    for k in ("dy2", "dx2", "inter"):
        assert ratios[k] <= 1.0, (tag, k + " outside its bound", ratios[k], float(s[k][0]), ca["last_" + ("interaction" if k == "inter" else k)])


def _first(a, b):
    return int(np.argmax(np.asarray(a).view(np.int64) != np.asarray(b).view(np.int64)))


def check_attempt(S, prob, sp, before, after, tag="", exact=None, resident=False):
    """Every rule of the module's docstring for ONE attempt.  before / after: dict(ctl=control block, X, Y, ATY, X_OTHER, Y_OTHER,
    ATY_OTHER, SUM_X, SUM_Y[, XBAR in `after`]) as downloaded in front of and behind it (X: the CURRENT side at that moment).
    resident: the rules of the resident small-LP path (neither the _OTHER buffers nor XBAR are read).
    Raises AssertionError naming the stage; returns dict(accepted, error, margin, limit, pending_before, cur_before, ratios:
    y, aty, dy2, dx2, inter)."""
    if resident:
        return _check_resident_attempt(S, prob, sp, before, after, tag, exact)
    cb, ca = ctl_dict(before["ctl"]), ctl_dict(after["ctl"])
    assert cb["error"] == 0 and cb["steps_taken"] < ca["target_steps"], (tag, "the attempt was a no-op by its guard", cb, ca)
    flipped = ca["cur"] != cb["cur"]
    trial = {k: after[k if flipped else k + "_OTHER"] for k in ("X", "Y", "ATY")}
    kept = {k: after[k + "_OTHER" if flipped else k] for k in ("X", "Y", "ATY")}
    for k in ("X", "Y", "ATY"):  # the iterate the attempt started from is read, never written
        assert bits_equal(kept[k], before[k]), (tag, "the attempt changed its own input", k)
    # (1) k_primal
    p = primal(prob, cb, before)
    assert bits_equal(trial["X"], p["xn"]), (tag, "x'", int(np.argmax(trial["X"] != p["xn"])))
    assert bits_equal(after["XBAR"], p["xbar"]), (tag, "xbar", int(np.argmax(after["XBAR"] != p["xbar"])))
    assert bits_equal(after["SUM_X"], p["sumx"]), (tag, "SUM_X", cb["pending_avg"], int(np.argmax(after["SUM_X"] != p["sumx"])))
    # (2) the A product with DualEpilogue, from the device's own xbar
    d = dual(S, prob, cb, before, after["XBAR"], exact)
    assert np.isfinite(trial["Y"]).all(), (tag, "y'")
    ry = worst_ratio(abs_err(d, trial["Y"]), d["bound"])
    assert ry <= 1.0, (tag, "y' outside its bound", ry, int(np.argmax(abs_err(d, trial["Y"]) / np.maximum(d["bound"], 1e-300))))
    assert bits_equal(after["SUM_Y"], d["sumy"]), (tag, "SUM_Y", cb["pending_avg"], int(np.argmax(after["SUM_Y"] != d["sumy"])))
    # (3) the A^T product with StepEpilogue, from the device's own y'
    a = aty_product(S, prob, trial["Y"], exact)
    assert np.isfinite(trial["ATY"]).all(), (tag, "A^T y'")
    ra = worst_ratio(abs_err(a, trial["ATY"]), a["bound"])
    assert ra <= 1.0, (tag, "A^T y' outside its bound", ra, int(np.argmax(abs_err(a, trial["ATY"]) / np.maximum(a["bound"], 1e-300))))
    assert (trial["ATY"][S.len_c == 0] == 0.0).all(), (tag, "A^T y' of the empty columns")
    # (4) the three sums, from the device's own vectors
    ratios = dict(y=ry, aty=ra)
    _check_sums(tag, step_sums(before, trial["X"], trial["Y"], trial["ATY"], exact), ca, ratios)
    # (5) the decision, from the device's own three sums
    dec, want = _check_decision(tag, cb, ca, flipped, sp)
    return dict(accepted=dec["accepted"], error=want["error"], margin=dec["margin"], limit=dec["limit"], pending_before=cb["pending_avg"],
                cur_before=cb["cur"], ratios=ratios)


def resident_trial(S, prob, ctl, st):
    """the trial iterate of the resident path in float64, every row and column left to right: dict(xn, xbar, sumx, y, sumy, aty)"""
    p = primal(prob, ctl, st)
    y = dual_f64(prob, ctl, st, rowsums_f64(prob["A_VALUES"], p["xbar"], S.off, S.idx))
    sumy = st["SUM_Y"] + np.float64(ctl["step_size"]) * st["Y"] if ctl["pending_avg"] else st["SUM_Y"].copy()
    at_values = prob["AT_VALUES"] if "AT_VALUES" in prob else prob["A_VALUES"][S.order]
    return dict(p, y=y, sumy=sumy, aty=rowsums_f64(at_values, y, S.t_off, S.t_rows))


def _check_resident_attempt(S, prob, sp, before, after, tag, exact):
    cb, ca = ctl_dict(before["ctl"]), ctl_dict(after["ctl"])
    assert cb["error"] == 0 and cb["steps_taken"] < ca["target_steps"], (tag, "the attempt was a no-op by its guard", cb, ca)
    flipped = ca["cur"] != cb["cur"]
    t = resident_trial(S, prob, cb, before)
    assert np.isfinite(t["y"]).all() and np.isfinite(t["aty"]).all(), (tag, "the reference's own trial iterate")
    # (1) - (3): the running sums always; the trial iterate where it is the new current side, the untouched iterate where it is not
    assert bits_equal(after["SUM_X"], t["sumx"]), (tag, "SUM_X", cb["pending_avg"], _first(after["SUM_X"], t["sumx"]))
    assert bits_equal(after["SUM_Y"], t["sumy"]), (tag, "SUM_Y", cb["pending_avg"], _first(after["SUM_Y"], t["sumy"]))
    if flipped:
        assert bits_equal(after["X"], t["xn"]), (tag, "x'", _first(after["X"], t["xn"]))
        assert bits_equal(after["Y"], t["y"]), (tag, "y'", _first(after["Y"], t["y"]))
        assert bits_equal(after["ATY"], t["aty"]), (tag, "A^T y'", _first(after["ATY"], t["aty"]))
        assert (after["ATY"][S.len_c == 0] == 0.0).all(), (tag, "A^T y' of the empty columns")
    else:
        for k in ("X", "Y", "ATY"):
            assert bits_equal(after[k], before[k]), (tag, "the rejected attempt changed", k, _first(after[k], before[k]))
    # (4) the three sums, from the reference's own trial vectors
    ratios = dict(y=0.0, aty=0.0)
    _check_sums(tag, step_sums(before, t["xn"], t["y"], t["aty"], exact), ca, ratios)
    # (5) the decision, from the device's own three sums
    dec, want = _check_decision(tag, cb, ca, flipped, sp)
    return dict(accepted=dec["accepted"], error=want["error"], margin=dec["margin"], limit=dec["limit"], pending_before=cb["pending_avg"],
                cur_before=cb["cur"], ratios=ratios)
