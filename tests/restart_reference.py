"""TEST UTILITY: the infeasibility information and the trust-region bounds (Methodical1) restated in extended precision, with a DERIVED
error bound per figure.  numpy only; in the manner of tests/eval_reference.py, whose _lift, _segment_sums, U and np.longdouble / Fraction
switch it reuses.

What it restates is this repository's own device code (cuopt_amd/csrc/pdlp_eval.hip): k_infeas_rows, k_infeas_cols and
compute_remaining_stats behind pdlpdev_eval_infeasibility; tr_element, k_tr_stats, k_tr_pass, k_tr_final and the host loop of
pdlpdev_trust_region_bounds.  Both functions work on the UNSCALED problem and are handed the device's OWN products A x and A^T y
(AX_U_*, ATY_U_*, downloaded), so that every element-wise decision -- g == 0, the two reduced-cost rules, zero_if_is_finite, the
subgradient's branch, blocked / free / moving, the threshold -- is taken on the doubles the device took it on: the decisions are formed in
float64 with the device's expressions (the device layer is built with -ffp-contract=off, and none of them has the shape of a fused
multiply-add anyway), there are no near ties to leave out.

The sums.  A sum of L terms whose terms carry at most 5 roundings of their own (the unscaled iterate, a difference, a product, the
final combination, a division by a scale) and which is added up in ANY order -- a lane's grid-stride loop, the workgroup's tree,
k_finalize, the communicator's tree over the ranks -- is within

    (L + 16) u  sum |terms|,   u = 2^-53

of the exact sum of the exact terms (gamma_L of Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: at most L - 1
additions touch a term in any tree; 5 rounded up to 16; L^2 u^2 is below 1e-9 of the bound at L <= 10^6).  The reference's own error is
L 2^-64 of the same sum.  Partial sums that are exactly zero (the workgroups of a rank that leaves the primal part to rank 0) add nothing.

infeasibility().  The two maxima are order independent and every operand is a double the device holds or forms in one rounding:
max_primal_ray_infeasibility and max_dual_ray_infeasibility are formed here in float64 by compute_remaining_stats' expressions and must
come out BIT FOR BIT.  primal_ray_linear_objective = (sum c_j x_j) / ||x||_inf over L = n terms; dual_ray_linear_objective =
(sum B(y_i) + sum B(rc_j)) / max(||y||_inf, ||rc||_inf) over L = m + n terms: the bound above divided by the same scale (the division, the
reciprocal and the addition of the two halves are three of the 16).

trust_region().  The elements are tr_element's, in float64.  primal_distance2, dual_distance2 and lagrangian are sums: the bound above,
with L = n, m and 2 n + m (the Lagrangian's three dot products hold 2 n + m terms; its two final combinations are two of the 16).
distance = sqrt(a pd2 + b dd2), a = pds w, b = dds / w:  |sqrt(s') - sqrt(s)| <= |s' - s| / sqrt(s), and s' - s is a bound_pd2 + b bound_dd2
plus 8 u s for the five roundings of the expression.

t* is NOT found the device's way (a monotone fixed point on the partition) but from the sorted finite thresholds and the one quadratic:
R^2(t) = sum_{thr <= t} w (bound - center)^2 + t^2 sum_{thr > t} w dir^2 is continuous and non-decreasing; the segment of R^2(t) = T^2 is
found on the cumulative sums, t = sqrt((T^2 - low) / high) inside it; T^2 beyond R^2 of the largest finite threshold with nothing moving
freely: t = that threshold ("everything that moves is at its bound"); T == 0 or ||objective|| == 0: t = 0.

lower_bound = lagrangian + sum_{k < n} grad_k (clamp(center_k + t dir_k) - center_k), upper_bound the same over k >= n.  Both are monotone
in t (every term of the first is <= 0 and falls with t, of the second >= 0 and grows), and t is monotone in T.  The device's low(t), high(t)
are sums of N = n + m non-negative terms: relative error at most (N + 16) u each, so the t it stops at is the exact t* of a radius within
T (1 +- eps), eps = (n + m + 32) u (this also covers T = the device's own distance where radius < 0, whose relative error is below
(max(n, m) + 24) u).  Hence

    bound = max |f(T (1 +- 4 eps)) - f(T)|  +  (L + 16) u sum |grad_k (z_k(t) - center_k)|  +  bound_lagrangian.

ASSUMED, not derived (returned as assumed_cancellation and asserted by the tests per case, on the host's own numbers): z_k(t) - center_k
is formed as fl(center + t dir) - center, which costs u |center_k| per moving element whatever t, i.e. u sum |center_k grad_k| in the
final sum.  On the primal side that is below u (sum |c x| + sum |x A^T y|), which the Lagrangian's bound holds 2 n + m + 16 times while
its own error needs max(n, m) + 3 of them.  On the dual side u sum |y_i (sub_i - (A x)_i)| is NOT bounded by the Lagrangian's terms in
general (A x can be large where y sub is small); the bound closes where it is at most (n + 13) u sum |Lagrangian's terms|, the share of
bound_lagrangian its own error does not need.  The same cancellation inside low(t) is second order (clipped elements sit ON the bound:
fl(bound - center) is one rounding)."""
import fractions
import math

import numpy as np

from eval_reference import LONGDOUBLE_IS_EXTENDED, U, _bound_value_product, _finite_part, _lift

INF = np.inf
INFEAS_KEYS = ("max_primal_ray_infeasibility", "primal_ray_linear_objective", "max_dual_ray_infeasibility", "dual_ray_linear_objective")
TR_KEYS = ("primal_distance2", "dual_distance2", "distance", "lagrangian", "lower_bound", "upper_bound")


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _sum(v, exact):
    """sum of a lifted vector (0 for an empty one, in the lifted type)"""
    if len(v) == 0:
        return fractions.Fraction(0) if exact else np.longdouble(0)
    return v.sum()


def _sqrt(v, exact):
    if not exact:
        return np.sqrt(v)
    if v <= 0:
        return fractions.Fraction(0)
    r = fractions.Fraction(math.sqrt(float(v)))
    for _ in range(2):  # (Newton from 53 correct bits: beyond 200)
        r = (r + v / r) / 2
    return r


def _max0(a):
    return float(a.max()) if len(a) else 0.0


def infeasibility(p, x, y, ax, aty, rule_finite=True, exact=None):
    """The four figures of compute_remaining_stats for the ray estimate (x, y) -- the unscaled iterate as the device forms it,
    fl(xhat D_c), fl(yhat D_r) -- with the device's products ax, aty -> dict of the four INFEAS_KEYS (float), `bound` (a bound for each of
    the two sum-based ones) and `counts` (the branches taken)."""
    if exact is None:
        exact = not LONGDOUBLE_IS_EXTENDED
    x, y, ax, aty = _f64(x), _f64(y), _f64(ax), _f64(aty)
    lo, hi, lb, ub, c = (_f64(p[k]) for k in ("lo", "hi", "lb", "ub", "c"))
    m, n = len(y), len(x)
    # ---- rows: float64, the device's expressions
    flo, fhi = np.isfinite(lo), np.isfinite(hi)
    hl, hu = np.where(flo, 0.0, lo), np.where(fhi, 0.0, hi)  # zero_if_is_finite
    viol_rows = np.where(ax < hl, hl - ax, np.where(ax > hu, ax - hu, 0.0))
    r0, r1 = _max0(np.abs(viol_rows)), _max0(np.abs(y))
    # ---- columns
    g = -1.0 * aty
    bv = np.where(g > 0.0, lb, ub)
    with np.errstate(invalid="ignore"):
        take = np.isfinite(bv) if rule_finite else (np.abs(x - bv) <= np.abs(x))
    rc = np.where(g == 0.0, g, np.where(take, g, 0.0))
    viol = np.zeros(n)
    viol = np.where(np.isfinite(lb), np.maximum(viol, -x), viol)
    viol = np.where(np.isfinite(ub), np.maximum(viol, x), viol)
    c0, c1, c2, c3 = _max0(np.abs(g - rc)), _max0(np.abs(rc)), _max0(np.abs(x)), _max0(viol)
    # ---- the three sums, extended
    zm, zn = _lift(np.zeros(m), exact), _lift(np.zeros(n), exact)
    t_y = _bound_value_product(_lift(y, exact), _finite_part(lo, exact), _finite_part(hi, exact), zm)
    t_rc = _bound_value_product(_lift(rc, exact), _finite_part(lb, exact), _finite_part(ub, exact), zn)
    t_cx = _lift(c, exact) * _lift(x, exact)
    dual_sum, dual_abs = _sum(t_y, exact) + _sum(t_rc, exact), _sum(np.abs(t_y), exact) + _sum(np.abs(t_rc), exact)
    cx, cx_abs = _sum(t_cx, exact), _sum(np.abs(t_cx), exact)
    # ---- compute_remaining_stats
    scaling = max(r1, c1)
    out = dict.fromkeys(INFEAS_KEYS, 0.0)
    bound = dict(primal_ray_linear_objective=0.0, dual_ray_linear_objective=0.0)
    if scaling != 0.0:
        s = _lift([scaling], exact)[0]
        out["max_dual_ray_infeasibility"] = c0 / scaling
        out["dual_ray_linear_objective"] = float(dual_sum / s)
        bound["dual_ray_linear_objective"] = (m + n + 16) * U * float(dual_abs / s)
    if c2 > 0.0:
        s = _lift([c2], exact)[0]
        out["max_primal_ray_infeasibility"] = max(r0, c3) / c2
        out["primal_ray_linear_objective"] = float(cx / s)
        bound["primal_ray_linear_objective"] = (n + 16) * U * float(cx_abs / s)
    nz = g != 0.0
    counts = dict(g_zero=int((~nz).sum()), rc_taken=int((nz & take).sum()), rc_dropped=int((nz & ~take).sum()),
                  rows_lo_finite_violated=int((flo & (ax < 0.0)).sum()), rows_hi_finite_violated=int((fhi & (ax > 0.0)).sum()),
                  rows_free=int((~flo & ~fhi).sum()))
    out.update(bound=bound, counts=counts)
    return out


def elements(p, x, y, ax, aty, wp, wd):
    """tr_element for all n + m virtual elements, in float64 with the device's expressions -> dict of arrays (center, obj, lb, ub, w, dir,
    thr, grad, sub) and `counts` (the branches taken)"""
    x, y, ax, aty = _f64(x), _f64(y), _f64(ax), _f64(aty)
    lo, hi, lb, ub, c = (_f64(p[k]) for k in ("lo", "hi", "lb", "ub", "c"))
    m, n = len(y), len(x)
    flo, fhi = np.isfinite(lo), np.isfinite(hi)
    clipped = np.where(ax < lo, lo, np.where(ax > hi, hi, ax))
    sub = np.where(y < 0.0, hi, np.where(y > 0.0, lo, np.where(~fhi & ~flo, 0.0, np.where(~fhi, lo, np.where(~flo, hi, clipped)))))
    with np.errstate(invalid="ignore"):
        gy = sub - ax
    gx = c - aty
    center = np.concatenate([x, y])
    grad = np.concatenate([gx, gy])
    obj = np.concatenate([gx, -gy])
    low = np.concatenate([lb, np.where(fhi, -INF, 0.0)])
    upp = np.concatenate([ub, np.where(flo, INF, 0.0)])
    w = np.concatenate([np.full(n, float(wp)), np.full(m, float(wd))])
    blocked = ((center >= upp) & (obj <= 0.0)) | ((center <= low) & (obj >= 0.0))
    free = ~blocked & (obj == 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(blocked | free, 0.0, -obj / w)
        thr = np.where(d > 0.0, (upp - center) / d, np.where(d < 0.0, (low - center) / d, 0.0))
    thr = np.where(free, INF, thr)
    zy, eq = y == 0.0, flo & fhi & (lo == hi)
    counts = dict(col_on_lb_g_pos=int(((x <= lb) & (gx > 0.0)).sum()), col_on_ub_g_neg=int(((x >= ub) & (gx < 0.0)).sum()),
                  col_on_lb_g_neg=int(((x <= lb) & (gx < 0.0)).sum()), g_zero=int((gx == 0.0).sum()),
                  col_free=int((~np.isfinite(lb) & ~np.isfinite(ub)).sum()), col_fixed=int((lb == ub).sum()),
                  y_neg=int((y < 0.0).sum()), y_pos=int((y > 0.0).sum()), y0_free=int((zy & ~flo & ~fhi).sum()),
                  y0_lo_only=int((zy & flo & ~fhi).sum()), y0_hi_only=int((zy & ~flo & fhi).sum()), y0_both=int((zy & flo & fhi).sum()),
                  y0_both_below=int((zy & flo & fhi & (ax < lo)).sum()), y0_both_above=int((zy & flo & fhi & (ax > hi)).sum()),
                  rows_equality=int(eq.sum()), blocked=int(blocked.sum()), moving=int((d != 0.0).sum()),
                  moving_forever=int(((d != 0.0) & ~np.isfinite(thr)).sum()))
    return dict(center=center, obj=obj, lb=low, ub=upp, w=w, dir=d, thr=thr, grad=grad, sub=sub, n=n, m=m, counts=counts)


class _Search:
    """the moving elements sorted by threshold, with the cumulative sums of R^2(t)"""

    def __init__(self, e, exact):
        self.exact, self.n = exact, e["n"]
        mv = np.nonzero(e["dir"] != 0.0)[0]
        order = mv[np.argsort(e["thr"][mv], kind="stable")]
        self.idx = order
        self.thr64 = e["thr"][order]
        self.nf = int(np.isfinite(self.thr64).sum())
        L = lambda a: _lift(a, exact)  # noqa: E731
        self.center, self.dir, self.w, self.grad = L(e["center"][order]), L(e["dir"][order]), L(e["w"][order]), L(e["grad"][order])
        d64 = e["dir"][order]
        self.to64 = np.where(d64 > 0.0, e["ub"][order], e["lb"][order])  # the bound an element runs into (infinite behind nf)
        self.lo_f, self.hi_f = _finite_part(e["lb"][order], exact), _finite_part(e["ub"][order], exact)
        zero = _lift([0.0], exact)
        step = L(np.where(np.isfinite(self.to64), self.to64, 0.0)) - self.center
        clipped = (self.w * step * step)[:self.nf]
        moving = self.w * self.dir * self.dir
        # low[j]: the first j elements at their bounds; high[j]: elements j .. moving freely (suffix sums: no cancellation)
        self.low = np.concatenate([zero, np.cumsum(clipped)]) if self.nf else zero.copy()
        self.high = np.concatenate([np.cumsum(moving[::-1])[::-1], zero]) if len(order) else zero.copy()
        self.thr = L(self.thr64[:self.nf])
        self.r2 = self.low[:self.nf] + self.thr * self.thr * self.high[:self.nf]  # R^2 at breakpoint j, non-decreasing
        self.max_thr = self.thr[-1] if self.nf else zero[0]

    def t_of(self, T):
        """-> (t, j = elements at their bounds, exit)"""
        T2 = T * T
        if len(self.idx) == 0:
            return self.max_thr, 0, "nothing-moves"
        j = int(np.searchsorted(np.maximum.accumulate(self.r2), T2, side="left")) if self.nf else 0
        if j == self.nf and self.nf == len(self.idx):
            return self.max_thr, j, "beyond-all"
        t = _sqrt(max(T2 - self.low[j], 0 * T2) / self.high[j], self.exact)
        if j > 0 and t < self.thr[j - 1]:  # (a threshold is a rounded quotient: t stays inside the segment its partition belongs to)
            t = self.thr[j - 1]
        return t, j, "inside-first" if j == 0 else "across"

    def sums(self, t):
        """(sum over the primal elements, over the dual ones, the same of the absolute terms) of grad (clamp(center + t dir) - center)"""
        if len(self.idx) == 0:
            z = _lift([0.0], self.exact)[0]
            return z, z, z, z
        z = self.center + t * self.dir
        z = np.where(self.lo_f[0] & (z < self.lo_f[1]), self.lo_f[1], z)
        z = np.where(self.hi_f[0] & (z > self.hi_f[1]), self.hi_f[1], z)
        term = (z - self.center) * self.grad
        pr = self.idx < self.n
        return _sum(term[pr], self.exact), _sum(term[~pr], self.exact), _sum(np.abs(term[pr]), self.exact), _sum(np.abs(term[~pr]), self.exact)


def trust_region(p, xhat, yhat, lrx, lry, dr, dc, ax, aty, wp, wd, pds=0.5, dds=0.5, primal_weight=1.0, radius=-1.0, exact=None):
    """pdlpdev_trust_region_bounds at the point (xhat, yhat) with the anchors (lrx, lry), all four as the device holds them: with D_r,
    D_c given the element is fl(xhat D_c) and the distance fl(fl(lrx - xhat) D_c) (scaled_iterates = 0), with dr = dc = None the vectors
    are taken as they are (scaled_iterates = 1).  ax, aty: the device's products for that point.
    -> dict of the six TR_KEYS (float), `bound` (one per figure), `t`, `exit`, `counts`, `assumed_cancellation` (see the module's text)."""
    if exact is None:
        exact = not LONGDOUBLE_IS_EXTENDED
    xhat, yhat, lrx, lry = _f64(xhat), _f64(yhat), _f64(lrx), _f64(lry)
    n, m = len(xhat), len(yhat)
    if dc is None:
        x, y, dx, dy = xhat, yhat, lrx - xhat, lry - yhat
    else:
        dr, dc = _f64(dr), _f64(dc)
        x, y, dx, dy = xhat * dc, yhat * dr, (lrx - xhat) * dc, (lry - yhat) * dr
    e = elements(p, x, y, ax, aty, wp, wd)
    L = lambda a: _lift(a, exact)  # noqa: E731
    one = lambda v: _lift([float(v)], exact)[0]  # noqa: E731
    # ---- pass 0
    pd2, dd2 = _sum(L(dx) * L(dx), exact), _sum(L(dy) * L(dy), exact)
    xe, ye = L(x), L(y)
    t_cx, t_xaty, t_ysub = L(p["c"]) * xe, xe * L(aty), ye * L(np.where(y == 0.0, 0.0, e["sub"]))  # (y == 0: the term is 0 whatever sub)
    lag = (_sum(t_cx, exact) - _sum(t_xaty, exact)) + _sum(t_ysub, exact)
    lag_abs = _sum(np.abs(t_cx), exact) + _sum(np.abs(t_xaty), exact) + _sum(np.abs(t_ysub), exact)
    a, b = one(pds) * one(primal_weight), one(dds) / one(primal_weight)
    s = pd2 * a + dd2 * b
    own = _sqrt(s, exact)
    out = dict(primal_distance2=float(pd2), dual_distance2=float(dd2), distance=float(own), lagrangian=float(lag))
    bound = dict(primal_distance2=(n + 16) * U * float(pd2), dual_distance2=(m + 16) * U * float(dd2),
                 lagrangian=(2 * n + m + 16) * U * float(lag_abs))
    bound["distance"] = 0.0 if own == 0 else float((a * one(bound["primal_distance2"]) + b * one(bound["dual_distance2"]) + 8 * one(U) * s) / own)
    # ---- t* and the two bounds
    T = one(radius) if radius >= 0.0 else own
    obj_is_zero = not np.any(e["obj"] != 0.0)
    srch = _Search(e, exact)
    eps = one((n + m + 32) * U)

    def solve(Tq):
        if Tq == 0 or obj_is_zero:
            t, j, ex = one(0.0), 0, "T==0" if Tq == 0 else "obj==0"
        else:
            t, j, ex = srch.t_of(Tq)
        return (t, j, ex) + srch.sums(t)

    t, j, ex, f_lo, f_up, abs_lo, abs_up = solve(T)
    spread_lo = spread_up = one(0.0)
    for Tq in (T * (1 - 4 * eps), T * (1 + 4 * eps)):
        q = solve(Tq)
        spread_lo, spread_up = max(spread_lo, abs(q[3] - f_lo)), max(spread_up, abs(q[4] - f_up))
    out.update(lower_bound=float(lag + f_lo), upper_bound=float(lag + f_up))
    bound["lower_bound"] = float(spread_lo) + (n + 16) * U * float(abs_lo) + bound["lagrangian"]
    bound["upper_bound"] = float(spread_up) + (m + 16) * U * float(abs_up) + bound["lagrangian"]
    mv = e["dir"][n:] != 0.0
    with np.errstate(invalid="ignore"):
        cancel = U * float(np.abs(e["center"][n:][mv] * e["grad"][n:][mv]).sum())
    counts = dict(e["counts"], at_bounds=j, finite_thresholds=srch.nf)
    out.update(bound=bound, t=float(t), exit=ex, counts=counts, radius=float(T),
               assumed_cancellation=dict(dual=cancel, room=(n + 13) * U * float(lag_abs)))
    return out


def ratio(got, want, bound):
    """|got - want| / bound; 0 / 0 = 0, an error above a zero bound is infinite"""
    err = abs(float(got) - float(want))
    if err == 0.0:
        return 0.0
    return err / bound if bound > 0.0 else INF
