"""TEST UTILITY: one step of the restarted reflected-Halpern mode and its restart restated stage by stage, in the style of
tests/attempt_reference.py (whose helpers it uses): numpy only, every sum in np.longdouble (64-bit significand) or in exact rationals
where the platform's long double is no wider than a double.

What it restates is this repository's own device code: k_primal (cuopt_amd/csrc/pdlp_device.hip), HalpernWeights, HalpernDualEpilogue
and HalpernStepEpilogue (pdlp_epilogues.hpp), halpern_decision_workgroup (halpern_decision.hpp), restart_block (pdlp_kernels.hpp)
and k_halpern_restart_ctl (pdlp_device.hip) -- on the SCALED problem as the device holds it and on the state downloaded IN FRONT of
the step.  Every stage takes what the device itself held for that stage -- the A product the device's xbar, the A^T product the
device's y', the three sums the device's vectors, the decision the device's three sums -- so an error never compounds across stages or
steps, and a failure names the stage and the element.

check_step is only ever called behind a run of ONE step (target_steps = steps_taken + 1 in front of it: asserted), where the step is
the last of its run and stores x'.

The weights are formed in float64 as HalpernWeights forms them, with k = hal.k in front of the step:
    w = (k + 1.0) / (k + 2.0),  w0 = 1.0 - w,  combine(t, z, z0) = w * (2.0 * t - z) + w0 * z0          (in that order)

BIT FOR BIT (the library is built with -ffp-contract=off; float64 numpy, the kernel's order of operations):
    x' (AVG_X) = attempt_reference.primal()'s xn, XBAR its xbar
    the new X = combine(x', X, anchor X);  the new Y = combine(AVG_Y, Y, anchor Y), AVG_Y the device's OWN y'
    on an empty row AVG_Y = dual_f64 at v = 0; on an empty column the new ATY = combine(0.0, ATY, anchor ATY)
    the side the step started from (now _OTHER), the three anchors, SUM_X and SUM_Y keep their bits
    from the device's own three sums in the control block, w_p = primal_weight, eta = step_size:
        r2 = ((w_p / eta) * dx2 + 2.0 * inter) + dy2 / (eta * w_p) = last_movement = hal.r2;  hal.r = sqrt(max(r2, 0)) (sqrt is
        correctly rounded on both sides); hal.r_first is written only when k was 0; hal.r2_min = min(previous, r2);
        hal.k, ctl.k, attempts, steps_taken, its_since_restart grow by 1 and cur flips; step_size, primal_weight, tau, sigma,
        sum_weights, pending_avg and error are unchanged.  A NaN, or r2 >= 1e100: error = 1, hal keeps EVERY field (k too), the
        counters of the control block advance all the same (halpern_decision.hpp writes them behind the branch).

BOUNDED, per element, u = 2^-53, for ANY summation tree (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2):

  y' (AVG_Y).  The arithmetic in front of the store to yp is DualEpilogue's, so the bound per row is attempt_reference.dual()'s, from
  the device's own XBAR, branch ties widened as there; no row is left out.

  A^T y^{k+1}.  v = A^T y' is never stored; it is seen through the new ATY.  With (v_ref, bound_v) = aty_product(S, prob, AVG_Y),
  a = ATY and a0 = the anchor's ATY in front of the step, and the device's v^ = v + e, |e| <= bound_v:
      d  = fl(2 v^ - a)          2 v^ is exact; |d - (2 v - a)| <= 2 |e| + u (2 |v| + |a|)
      p  = fl(w d), q = fl(w0 a0), ATY_new = fl(p + q)
      |ATY_new - (w (2 v - a) + w0 a0)| <= 2 w bound_v + 4 u (w (2 |v| + |a|) + w0 |a0|)
  to first order: four roundings (d, p, q, the sum), of which 3 fall on the first term and 2 on the second, rounded up to 4 on
  both.  w >= 1/2, so an error in v is never damped below itself: 2 w >= 1.

  dy2, dx2: attempt_reference.step_sums on the device's AVG_Y and x': within (m + 16) u and (n + 16) u of the sums of squares.

  the interaction.  The device adds t^_j dx_j, t^ = fl(v^ - a), dx = fl(x' - x) (exact difference rounded once, as step_sums takes it):
      |inter - sum t_j dx_j| <= (n + 16) u sum |t_j dx_j| + sum |dx_j| bound_v_j,     t = v_ref - a
  (the first term: one rounding each for t^, dx, the product, and at most n - 1 for the tree; the second: v^'s own error).

  the partials.  k_halpern_decision adds the partials of the two products (PART_A: nb_A of dy2; PART_AT: nb_At of the interaction,
  then nb_At of dx2) in a tree of its own: each of the three sums in the control block lies within (nb + 16) u sum |partial| of the
  extended sum of the downloaded partials.

THE RESTART (check_restart; pdlpdev_halpern_restart(theta)):
    the anchors equal the current X, Y and ATY bit for bit, which the restart does not touch; hal.k = 0, its_since_restart = 0, every
    other field of hal and of the control block but the weight, tau and sigma is untouched.
    The two RETURNED distances are sqrt of restart_block's two sums: dist^2, squared in extended precision, lies within
    attempt_reference.restart()'s bound (N + 16) u of the sum of squares of the scaled differences -- the correctly rounded sqrt and
    its squaring are 2 of the 16 spare roundings, 3 + (N - 1) are taken by the differences, squares and the tree.
    theta < 0 or a distance <= 1e-10: the weight, tau and sigma keep their bits.  Otherwise, from the device's OWN two returned
    distances and its previous weight, in np.longdouble,
        w_ref = exp(theta ln(dy / dx) + (1 - theta) ln w),      |w_new - w_ref| <= u (8 + 6 (|theta ln(dy / dx)| + |(1 - theta) ln w|)) w_ref
    The exponent E = A + B has absolute error at most about u (|A| + |B|) from 1-ulp logarithms (relative u on each ln, the division
    correctly rounded in front of one), u (|A| + |B|) more from the two products, u |E| <= u (|A| + |B|) from the sum: 3 of the 6 on
    the device's side and 3 on the reference's where long double is no wider than a double; exp turns an absolute error of the
    exponent into a relative one of the result and adds its own ulp on each side, (1 - theta) is one rounding, the division one: 8.
    ASSUMPTION: log and exp of the device's math library, and of the host's for long double, are accurate to 1 ulp.  The
    toolchain this project builds with installs no document that states the accuracy of its double-precision log and exp (the device
    library's own table, OCML.md of ROCm-Device-Libs, is where it would stand), so the figure is an assumption of this test and is
    named as one: a ratio a little above 1 on the weight alone would question the assumption before it questions the kernel.
    tau = step_size / w_new and sigma = step_size * w_new, bit for bit from the device's own new weight.

The reference's own error is at most N 2^-64 of the same magnitude sums (1/2048 of a bound).  The bounds are derived, not measured:
a layout that exceeds one is a finding about the kernel concerned, not a reason to touch a bound.

THE RESIDENT ONE-WORKGROUP LOOP (check_step(resident=True); resident_halpern_body, cuopt_amd/csrc/resident_halpern_bodies.hpp, through
any of its three wrapper kernels).  There the owning lane of every row and of every column adds it up left to right in float64 from
products rounded once (prod[] = val * vec[col], then lds_row_sum), so MORE is bit for bit than in the layouts, and nothing of a step
is seen through a bound but its three sums.  `prob` carries AT_VALUES, the values the device holds for A^T's own CSR: scaling
multiplies A by D_r then D_c and A^T by D_c then D_r, so an entry of the two may differ in its last bit, and the loop reads A^T's.
  NOT READ: XBAR (the loop keeps xbar in LDS and never stores it) and PART_A / PART_AT (one workgroup: there are no partials; the
  `part` ratio is 0).
  (0) what the step must not change.  X_OTHER and Y_OTHER hold the bits of X and Y in front of the step: on the LAST step of a launch
      the loop stores z^k into the side `cur` selects at that moment, which the step's flip makes the other one (the ray pass of the
      evaluation reads it there).  The three anchors (read once into registers, never written), SUM_X and SUM_Y keep their bits.
      ATY_OTHER holds the bits of ATY in front of the step BEHIND A SINGLE-STEP LAUNCH ONLY: that launch read that side and never
      writes it.  Behind a multi-step launch ATY_OTHER is NOT PROMISED: the loop stores no A^T y^k (nothing reads it), so that side
      holds whatever an earlier launch left.  check_step is only ever called behind a single-step launch (asserted), so it asserts all
      three; halpern_step_scenario.check_composition, which looks behind a launch of 12 steps, leaves ATY_OTHER out.
      check_last_step_store asserts the store behind a launch of any length from one state alone: AVG_Y is, bit for bit, stage (2)
      applied to (X_OTHER, Y_OTHER) and AVG_X -- so what the ray pass reads as z^k is the point whose image the average slots hold.
  (1) the primal half.  AVG_X = attempt_reference.primal()'s xn bit for bit (every launch that made a step stores the x' of its last
      one); xbar is taken from primal() -- it is bit-exact from x', x -- and the new X = combine(k, xn, X, anchor X) bit for bit.
  (2) the dual half.  AVG_Y = dual_f64(prob, ctl, before, rowsums_f64(A_VALUES, xbar, off, idx)) BIT FOR BIT on every row, which on
      an empty row is dual_f64 at v = +0.0; the new Y = combine(k, AVG_Y, Y, anchor Y).
  (3) the A^T product.  v = rowsums_f64(AT_VALUES, AVG_Y, t_off, t_rows) over A^T's own CSR (the stable transposition of A:
      Structure.order), from the device's own AVG_Y; the new ATY = combine(k, v, ATY, anchor ATY) BIT FOR BIT -- on an empty column
      combine(k, +0.0, ATY, anchor ATY).
  (4) the three sums go through block_sum_fast's fixed tree, which is not left to right: they stay bounded.  Every lane adds its own
      terms in registers, then the tree: any order of n (m) terms.  dy2 and dx2 keep step_sums' bounds, (m + 16) u and (n + 16) u of
      the sums of squares (dy = fl(y' - y) is one rounding of the exact difference, its square two more, the tree at most N - 1 per
      term).  The interaction: the device adds fl(t^_j dx^_j) with t^ = fl(v_j - a_j) and dx^ = fl(x'_j - x_j), v the SAME float64
      number the reference holds (stage 3 is bit for bit).  One rounding each for t^, dx^ and the product and at most n - 1 for the
      tree give, to first order,
          |inter - sum t_j dx_j| <= (n + 2) u sum |t_j dx_j| <= (n + 16) u sum |t_j dx_j|,        t = v - a exactly.
      The layouts' second term, sum |dx_j| bound_v_j, carries the error of the device's v^ against the extended product; here
      v^ = v, so the carried term is 0.
  (5) the decision: check_decision unchanged -- r2, r, r_first, r2_min, the counters and the error branch from the device's own three
      sums.  In the loop every lane repeats it on its own copy of both blocks; lane 0's copy is what the launch stores.
check_restart applies as it stands: the restart of a resident context is pdlpdev_halpern_restart's, and a batch's
halpern_restart_finish_workgroup is compared bit for bit with it through whole solves."""
import math

import numpy as np

import attempt_reference as ar
from attempt_reference import Structure, abs_err, aty_product, bits_equal, dual, dual_f64, primal, restart, scalar_ratio, step_sums  # noqa: F401
from eval_reference import U, _down, _lift, worst_ratio

HAL_FIELDS = ("r", "r_first", "r2", "r2_min", "k")
ANCHORS = ("LAST_RESTART_X", "LAST_RESTART_Y", "LAST_RESTART_ATY")
BEFORE = ("X", "Y", "ATY", "SUM_X", "SUM_Y") + ANCHORS
AFTER = BEFORE + ("XBAR", "AVG_X", "AVG_Y", "X_OTHER", "Y_OTHER", "ATY_OTHER", "PART_A", "PART_AT")
AFTER_RESIDENT = BEFORE + ("AVG_X", "AVG_Y", "X_OTHER", "Y_OTHER", "ATY_OTHER")  # the resident loop: no XBAR, no partials
RATIOS = ("y", "aty", "dy2", "dx2", "inter", "part", "dist", "weight")
UNCHANGED = ("step_size", "primal_weight", "tau", "sigma", "sum_weights", "pending_avg")
OVERFLOW = 1.0e100
SMALL_DISTANCE = 1.0e-10


def hal_dict(h):
    return {k: (int(h[k]) if k == "k" else float(h[k])) for k in HAL_FIELDS}


def weights(k):
    """HalpernWeights: (w, w0) in float64 from hal.k in front of the step"""
    k = np.float64(k)
    w = (k + np.float64(1.0)) / (k + np.float64(2.0))
    return w, np.float64(1.0) - w


def combine(k, t, z, z0):
    w, w0 = weights(k)
    return w * (np.float64(2.0) * t - z) + w0 * z0


def r2_of(ctl, dy2, inter, dx2):
    """halpern_decision_workgroup's r^2 in float64 from three sums GIVEN (Python floats are IEEE doubles, one rounding per operation)"""
    eta, w = float(ctl["step_size"]), float(ctl["primal_weight"])
    with np.errstate(all="ignore"):
        return float(np.float64(w / eta) * np.float64(dx2) + np.float64(2.0) * np.float64(inter) + np.float64(dy2) / np.float64(eta * w))


def _first(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return int(np.argmax(a.view(np.int64) != b.view(np.int64))) if a.shape == b.shape else -1


def _same_bits(tag, stage, got, want):
    assert bits_equal(got, want), (tag, stage, _first(got, want))


def _worst(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return int(np.argmax(np.where(err == 0.0, 0.0, err / bound)))


# ---- the stages of one step ------------------------------------------------------------------------------------------------------------
def check_vectors(S, prob, before, after, tag="", exact=None):
    """stages (0) - (3): what the step left in its buffers -> dict(ratios: y, aty; compared: rows and columns looked at; aty: the
    extended A^T y' and its bound, for the sums)"""
    cb, k = ar.ctl_dict(before["ctl"]), hal_dict(before["hal"])["k"]
    assert cb["pending_avg"] == 0, (tag, "an average pending in Halpern mode", cb)
    # (0) what the step reads and never writes
    for name in ("X", "Y", "ATY"):
        _same_bits(tag, "the step changed its own input " + name, after[name + "_OTHER"], before[name])
    for name in ANCHORS + ("SUM_X", "SUM_Y"):
        _same_bits(tag, "the step changed " + name, after[name], before[name])
    # (1) k_primal, and HalpernStepEpilogue's primal half
    p = primal(prob, cb, before)
    _same_bits(tag, "x' (AVG_X)", after["AVG_X"], p["xn"])
    _same_bits(tag, "xbar", after["XBAR"], p["xbar"])
    _same_bits(tag, "x^{k+1}", after["X"], combine(k, p["xn"], before["X"], before["LAST_RESTART_X"]))
    # (2) the A product with HalpernDualEpilogue, from the device's own xbar
    d = dual(S, prob, cb, before, after["XBAR"], exact)
    yp = after["AVG_Y"]
    assert yp.shape == (S.m,) and np.isfinite(yp).all(), (tag, "y' (AVG_Y) is not finite")
    err_y = abs_err(d, yp)
    ry = worst_ratio(err_y, d["bound"])
    assert ry <= 1.0, (tag, "y' (AVG_Y) outside its bound", ry, _worst(err_y, d["bound"]))
    empty_r = S.len_r == 0
    want = dual_f64(prob, cb, before, np.zeros(S.m))
    _same_bits(tag, "y' (AVG_Y) of the empty rows", yp[empty_r], want[empty_r])
    _same_bits(tag, "y^{k+1}", after["Y"], combine(k, yp, before["Y"], before["LAST_RESTART_Y"]))
    # (3) the A^T product with HalpernStepEpilogue, from the device's own y': v is seen through the new ATY
    a = aty_product(S, prob, yp, exact)
    ex = a["_exact"]
    w, w0 = weights(k)
    we, w0e = _lift([w], ex)[0], _lift([w0], ex)[0]
    old, anchor = before["ATY"], before["LAST_RESTART_ATY"]
    want_e = we * (2 * a["_ext"] - _lift(old, ex)) + w0e * _lift(anchor, ex)
    bound = 2.0 * w * a["bound"] + 4.0 * U * (w * (2.0 * np.abs(a["aty"]) + np.abs(old)) + w0 * np.abs(anchor))
    got = after["ATY"]
    assert got.shape == (S.n,) and np.isfinite(got).all(), (tag, "A^T y^{k+1} is not finite")
    err = _down(np.abs(_lift(got, ex) - want_e))
    ra = worst_ratio(err, bound)
    assert ra <= 1.0, (tag, "A^T y^{k+1} outside its bound", ra, _worst(err, bound))
    empty_c = S.len_c == 0
    _same_bits(tag, "A^T y^{k+1} of the empty columns", got[empty_c], combine(k, np.zeros(S.n), old, anchor)[empty_c])
    return dict(ratios=dict(y=ry, aty=ra), compared=dict(y=int(len(err_y)), aty=int(len(err))), xn=p["xn"], yp=yp, a=a)


def check_sums(S, before, after, vec, tag="", exact=None):
    """stage (4): the three sums of the control block against the device's own vectors, and against the downloaded partials
    -> dict(ratios: dy2, dx2, inter, part; values; inter_bound_rel: the interaction's bound over sum |t_j dx_j|)"""
    ca = ar.ctl_dict(after["ctl"])
    a, ex = vec["a"], vec["a"]["_exact"]
    s = step_sums(before, vec["xn"], vec["yp"], a["aty"], ex)
    dx = _lift(vec["xn"], ex) - _lift(before["X"], ex)
    t = a["_ext"] - _lift(before["ATY"], ex)
    inter, absinter = (t * dx).sum(), np.abs(t * dx).sum()
    carried = float((np.abs(dx) * _lift(a["bound"], ex)).sum())
    inter_bound = (S.n + 16) * U * float(absinter) + carried
    ratios = dict(dy2=scalar_ratio(s["dy2"], ca["last_dy2"], ex), dx2=scalar_ratio(s["dx2"], ca["last_dx2"], ex),
                  inter=scalar_ratio((inter, inter_bound), ca["last_interaction"], ex))
    for key, field, value in (("dy2", "last_dy2", s["dy2"][0]), ("dx2", "last_dx2", s["dx2"][0]), ("inter", "last_interaction", inter)):
        assert ratios[key] <= 1.0, (tag, key + " outside its bound", ratios[key], float(value), ca[field])
    # the partials: PART_A holds nb_A of dy2, PART_AT nb_At of the interaction and then nb_At of dx2
    pa, pt = np.asarray(after["PART_A"], dtype=np.float64), np.asarray(after["PART_AT"], dtype=np.float64)
    assert len(pa) >= 1 and len(pt) >= 2 and len(pt) % 2 == 0, (tag, "the partials", len(pa), len(pt))
    nb = len(pt) // 2
    worst = 0.0
    for name, field, part in (("dy2", "last_dy2", pa), ("interaction", "last_interaction", pt[:nb]), ("dx2", "last_dx2", pt[nb:])):
        pe = _lift(part, ex)
        entry = (pe.sum(), (len(part) + 16) * U * float(np.abs(pe).sum()))
        r = scalar_ratio(entry, ca[field], ex)
        assert r <= 1.0, (tag, "the partials of %s do not add up to the control block's sum" % name, r, float(entry[0]), ca[field])
        worst = max(worst, r)
    ratios["part"] = worst
    return dict(ratios=ratios, dy2=float(s["dy2"][0]), dx2=float(s["dx2"][0]), inter=float(inter), absinter=float(absinter),
                inter_bound_rel=(inter_bound / float(absinter) if float(absinter) > 0.0 else math.inf))


def check_resident_vectors(S, prob, before, after, tag=""):
    """stages (0) - (3) by the rules of the resident loop: every buffer bit for bit -> dict(xn, yp, v: the float64 A^T y')"""
    cb, k = ar.ctl_dict(before["ctl"]), hal_dict(before["hal"])["k"]
    assert cb["pending_avg"] == 0, (tag, "an average pending in Halpern mode", cb)
    # (0) what the step reads and never writes; z^k where the last step of a launch stores it
    for name in ("X", "Y", "ATY"):
        _same_bits(tag, "the step changed its own input " + name, after[name + "_OTHER"], before[name])
    for name in ANCHORS + ("SUM_X", "SUM_Y"):
        _same_bits(tag, "the step changed " + name, after[name], before[name])
    # (1) the primal half
    p = primal(prob, cb, before)
    _same_bits(tag, "x' (AVG_X)", after["AVG_X"], p["xn"])
    _same_bits(tag, "x^{k+1}", after["X"], combine(k, p["xn"], before["X"], before["LAST_RESTART_X"]))
    # (2) the dual half: every row left to right from the reference's own xbar (bit-exact from x')
    yp = after["AVG_Y"]
    want = dual_f64(prob, cb, before, ar.rowsums_f64(prob["A_VALUES"], p["xbar"], S.off, S.idx))
    assert yp.shape == (S.m,) and np.isfinite(want).all(), (tag, "the reference's own y'")
    _same_bits(tag, "y' (AVG_Y)", yp, want)
    _same_bits(tag, "y^{k+1}", after["Y"], combine(k, yp, before["Y"], before["LAST_RESTART_Y"]))
    # (3) the A^T product over A^T's own CSR and values, from the device's own y'
    at_values = prob["AT_VALUES"] if "AT_VALUES" in prob else prob["A_VALUES"][S.order]
    v = ar.rowsums_f64(at_values, yp, S.t_off, S.t_rows)
    assert after["ATY"].shape == (S.n,) and np.isfinite(v).all(), (tag, "the reference's own A^T y'")
    _same_bits(tag, "A^T y^{k+1}", after["ATY"], combine(k, v, before["ATY"], before["LAST_RESTART_ATY"]))
    return dict(xn=p["xn"], yp=yp, v=v)


def check_resident_sums(S, before, after, vec, tag="", exact=None):
    """stage (4) by the rules of the resident loop: the three sums against step_sums of x', y' and the float64 v (no carried term,
    no partials) -> what check_sums returns"""
    ca = ar.ctl_dict(after["ctl"])
    s = step_sums(before, vec["xn"], vec["yp"], vec["v"], exact)
    ex = s["_exact"]
    ratios = dict(dy2=scalar_ratio(s["dy2"], ca["last_dy2"], ex), dx2=scalar_ratio(s["dx2"], ca["last_dx2"], ex),
                  inter=scalar_ratio(s["inter"], ca["last_interaction"], ex), part=0.0)
    for key, field in (("dy2", "last_dy2"), ("dx2", "last_dx2"), ("inter", "last_interaction")):
        assert ratios[key] <= 1.0, (tag, key + " outside its bound", ratios[key], float(s[key][0]), ca[field])
    absinter = s["inter"][1] / ((S.n + 16) * U)
    return dict(ratios=ratios, dy2=float(s["dy2"][0]), dx2=float(s["dx2"][0]), inter=float(s["inter"][0]), absinter=float(absinter),
                inter_bound_rel=(S.n + 16) * U)  # (no carried term: the bound is that share of sum |t_j dx_j| whatever the step)


def check_last_step_store(S, prob, after, tag=""):
    """Behind a launch of ANY number of steps on the resident path: X_OTHER / Y_OTHER hold the z^k whose image T(z^k) the average
    slots hold -- y' = dual_f64 at Y_OTHER of the row sums of A (2 x' - x^k), bit for bit as stage (2) forms it.  A launch that left
    its last z^k in registers fails here: the side then holds the iterate of an earlier launch.  (tau and sigma are those of the last
    step: nothing but a restart moves them.)"""
    xn, xk = after["AVG_X"], after["X_OTHER"]
    want = dual_f64(prob, ar.ctl_dict(after["ctl"]), dict(Y=after["Y_OTHER"]), ar.rowsums_f64(prob["A_VALUES"], xn - xk + xn, S.off, S.idx))
    _same_bits(tag, "z^k (X_OTHER, Y_OTHER) is not the point whose image the average slots hold", after["AVG_Y"], want)


def check_decision(before, after, tag=""):
    """stage (5): halpern_decision_workgroup from the device's OWN three sums -> dict(r2, error)"""
    cb, ca = ar.ctl_dict(before["ctl"]), ar.ctl_dict(after["ctl"])
    hb, ha = hal_dict(before["hal"]), hal_dict(after["hal"])
    r2 = r2_of(cb, ca["last_dy2"], ca["last_interaction"], ca["last_dx2"])
    assert ca["last_movement"] == r2 or (r2 != r2 and ca["last_movement"] != ca["last_movement"]), (tag, "r2 (last_movement)", ca["last_movement"], r2)
    for key in ("k", "attempts", "steps_taken", "its_since_restart"):
        assert ca[key] == cb[key] + 1, (tag, "the counter " + key, cb[key], ca[key])
    assert ca["cur"] == cb["cur"] ^ 1, (tag, "cur did not flip", cb["cur"], ca["cur"])
    for key in UNCHANGED:
        assert ca[key] == cb[key], (tag, "the step changed " + key, cb[key], ca[key])
    error = int(r2 != r2 or not r2 < OVERFLOW)
    assert ca["error"] == error, (tag, "error", ca["error"], r2)
    if error:
        assert ha == hb or (ha["k"] == hb["k"] and all(bits_equal([ha[f]], [hb[f]]) for f in HAL_FIELDS[:4])), (tag, "hal behind the step error", hb, ha)
        return dict(r2=r2, error=1)
    assert ha["r2"] == r2, (tag, "hal.r2", ha["r2"], r2)
    assert ha["r"] == math.sqrt(max(r2, 0.0)), (tag, "hal.r", ha["r"], math.sqrt(max(r2, 0.0)))
    want_first = ha["r"] if hb["k"] == 0 else hb["r_first"]
    assert ha["r_first"] == want_first, (tag, "r_first", ha["r_first"], want_first, hb["k"])
    assert ha["r2_min"] == (hb["r2_min"] if hb["r2_min"] < r2 else r2), (tag, "r2_min", ha["r2_min"], hb["r2_min"], r2)
    assert ha["k"] == hb["k"] + 1, (tag, "hal.k", hb["k"], ha["k"])
    return dict(r2=r2, error=0)


def check_step(S, prob, before, after, tag="", exact=None, resident=False):
    """Every rule of the module's docstring for ONE step behind a single-step run.  before: dict(ctl, hal, X, Y, ATY, SUM_X, SUM_Y,
    LAST_RESTART_X/Y/ATY) as downloaded in front of it; after: the same plus XBAR, AVG_X, AVG_Y, X_OTHER, Y_OTHER, ATY_OTHER,
    PART_A, PART_AT (X: the CURRENT side at that moment).  resident: the rules of the resident one-workgroup loop -- `after` needs
    neither XBAR nor the partials (AFTER_RESIDENT), `prob` carries AT_VALUES.  Raises AssertionError naming the stage; returns
    dict(ratios: y, aty, dy2, dx2, inter, part; compared; dy2, dx2, inter, absinter, inter_bound_rel, r2, error, k_before,
    cur_before)."""
    cb, ca = ar.ctl_dict(before["ctl"]), ar.ctl_dict(after["ctl"])
    assert cb["error"] == 0 and ca["target_steps"] == cb["steps_taken"] + 1, (tag, "not one step behind a single-step run", cb, ca)
    if resident:
        vec = check_resident_vectors(S, prob, before, after, tag)
        vec.update(ratios=dict(y=0.0, aty=0.0), compared=dict(y=S.m, aty=S.n))  # (bit for bit on every row and column)
        sums = check_resident_sums(S, before, after, vec, tag, exact)
    else:
        vec = check_vectors(S, prob, before, after, tag, exact)
        sums = check_sums(S, before, after, vec, tag, exact)
    dec = check_decision(before, after, tag)
    out = dict(sums, **dec)
    out.update(ratios=dict(vec["ratios"], **sums["ratios"]), compared=vec["compared"], k_before=hal_dict(before["hal"])["k"], cur_before=cb["cur"])
    return out


# ---- the restart ---------------------------------------------------------------------------------------------------------------------------
def weight_reference(theta, dist, w_prev):
    """(w_ref as a long double, the allowed relative error) of k_halpern_restart_ctl's smoothed weight"""
    L = np.longdouble
    dx, dy = L(dist[0]), L(dist[1])
    first, second = L(theta) * np.log(dy / dx), (L(1.0) - L(theta)) * np.log(L(w_prev))
    return np.exp(first + second), U * (8.0 + 6.0 * (abs(float(first)) + abs(float(second))))


def check_restart(before, after, dist, theta, tag="", exact=None):
    """pdlpdev_halpern_restart(theta).  before / after: dict(ctl, hal, X, Y, ATY, LAST_RESTART_X/Y/ATY); dist: the two returned
    distances -> dict(ratios: dist, weight; smoothed)"""
    cb, ca = ar.ctl_dict(before["ctl"]), ar.ctl_dict(after["ctl"])
    hb, ha = hal_dict(before["hal"]), hal_dict(after["hal"])
    for name in ("X", "Y", "ATY"):
        _same_bits(tag, "the restart changed the iterate " + name, after[name], before[name])
        _same_bits(tag, "the anchor LAST_RESTART_" + name, after["LAST_RESTART_" + name], after[name])
    assert ha["k"] == 0 and ca["its_since_restart"] == 0, (tag, "hal.k / its_since_restart behind the restart", ha["k"], ca["its_since_restart"])
    assert all(ha[f] == hb[f] for f in HAL_FIELDS[:4]), (tag, "the restart changed hal", hb, ha)
    for key in cb:
        assert key in ("primal_weight", "tau", "sigma", "its_since_restart") or ca[key] == cb[key], (tag, "the restart changed " + key, cb[key], ca[key])
    ref, ex = restart(ar.CURRENT, 0, before["X"], before["Y"], before["LAST_RESTART_X"], before["LAST_RESTART_Y"], None, None, exact)
    ratios = []
    for (value, bound), got in zip(ref, dist):
        g = _lift([got], ex)[0]
        err = float(abs(g * g - value))
        ratios.append(0.0 if err == 0.0 else (err / bound if bound > 0.0 else math.inf))
    assert max(ratios) <= 1.0, (tag, "dist outside its bound", ratios, list(dist), [math.sqrt(float(v[0])) for v in ref])
    smoothed = theta >= 0.0 and dist[0] > SMALL_DISTANCE and dist[1] > SMALL_DISTANCE
    rw = 0.0
    if not smoothed:
        for key in ("primal_weight", "tau", "sigma"):
            assert ca[key] == cb[key], (tag, "the restart changed %s without smoothing" % key, cb[key], ca[key])
    else:
        w_ref, rel = weight_reference(theta, dist, cb["primal_weight"])
        rw = float(abs(np.longdouble(ca["primal_weight"]) - w_ref) / w_ref) / rel
        assert rw <= 1.0, (tag, "primal_weight outside its bound", rw, ca["primal_weight"], float(w_ref))
        assert ca["tau"] == ca["step_size"] / ca["primal_weight"] and ca["sigma"] == ca["step_size"] * ca["primal_weight"], (tag, "tau / sigma behind the restart")
    return dict(ratios=dict(dist=max(ratios), weight=rw), smoothed=smoothed)
