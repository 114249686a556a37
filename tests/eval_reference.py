"""TEST UTILITY: the convergence evaluation restated in extended precision, with a DERIVED error bound per row and column.

What it restates is this repository's own device code: EvalPrimalEpilogue and EvalDualCore (cuopt_amd/csrc/pdlp_epilogues.hpp),
violation, bound_value_product and combine_bounds (pdlp_kernels.hpp), read_eval (pdlp_layouts.hpp) -- on the UNSCALED problem, where
the device works on the scaled one and unscales per element.  numpy only; every sum is taken in np.longdouble (64-bit significand:
asserted), or in exact rationals (fractions.Fraction) where the platform's long double is no wider than a double.

The bounds.  The device forms (A x)_i = (sum_k fl(fl(a_ik D_r,i) D_c,k) xhat_k) / D_r,i in double, whatever its summation tree (a lane
left to right, a wave's shuffle tree, long-row partials, the dense share added ahead of the epilogue), and this reference is handed
x_k = fl(xhat_k D_c,k).  Per term that is at most 5 roundings (two for the scaled value, one for the unscaled iterate, the product, the
final division), every summation tree over L terms adds at most L - 1 more to any term (the standard gamma_L bound, Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2: valid for ANY order), so with u = 2^-53 and the 5 rounded up to 16

    |got_i - (A x)_i| <= (L_i + 16) u  sum_k |a_ik x_k|          =: bound_ax_i
    |got_j - (A^T y)_j| <= (L_j + 16) u  sum_i |a_ij y_i|        =: bound_aty_prod_j
    |got_j - g_j|, g = c - A^T y:  (L_j + 16) u (sum_i |a_ij y_i| + |c_j|)   =: bound_aty_j   (the subtraction is one more rounding)

(second-order terms L^2 u^2 are below 1e-8 of the bound at L <= 5000 and covered by the 11 spare roundings).  The reference's own
error is at most L 2^-64 of the same magnitude sums, 1/2048 of the bound.  The bounds are derived, not measured: a layout that
exceeds one is a finding.

near_tie marks the columns whose reduced-cost DECISION is not determined at that precision: 0 < |g_j| <= bound_aty_j (the sign of g
picks the bound) and, under the rule that is not the finite-bounds one, 0 < ||x_j - bv_j| - |x_j|| <= 16 u |x_j|.  Exact cases
(g_j == 0, x_j == bv_j, x_j == 0) are no ties."""
import fractions

import numpy as np

U = 2.0 ** -53
LONGDOUBLE_IS_EXTENDED = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)
SCALARS = ("CX", "DUAL_SUM", "PRES2", "DRES2", "X2", "Y2", "LINF_PRES_REL", "LINF_DRES_REL")


def _lift(a, exact):
    a = np.asarray(a, dtype=np.float64)
    if not exact:
        return a.astype(np.longdouble)
    out = np.empty(a.shape, dtype=object)
    out[...] = [fractions.Fraction(float(v)) for v in a]
    return out


def _down(a):
    return np.array([float(v) for v in a], dtype=np.float64) if a.dtype == object else a.astype(np.float64)


def _finite_part(b, exact):
    """(mask of the finite entries, the entries lifted with 0 in place of the infinite ones)"""
    b = np.asarray(b, dtype=np.float64)
    f = np.isfinite(b)
    return f, _lift(np.where(f, b, 0.0), exact)


def _segment_sums(v, off, zero):
    """sums of v over [off[i], off[i+1]): reduceat over the non-empty segments (an empty one has no element between two starts)"""
    out = zero.copy()
    ne = np.nonzero(np.diff(off) > 0)[0]
    if len(ne):
        out[ne] = np.add.reduceat(v, off[:-1][ne])
    return out


def _bound_value_product(v, lower, upper, zero):
    """bound_value_product: v > 0 takes the lower bound, v < 0 the upper one; an infinite bound (and v == 0) gives 0"""
    (lf, lv), (uf, uv) = lower, upper
    pos, neg = v > 0, v < 0
    finite = np.where(pos, lf, np.where(neg, uf, True))
    bound = np.where(pos, lv, np.where(neg, uv, zero))
    return np.where(finite, v * bound, zero)


def evaluate(p, x, y, rule_finite=True, eps_p=1e-4, eps_d=1e-4, exact=None):
    """The eight EV scalars of pdlpdev_eval (capi.EV), the vectors ax, aty, rc (rounded to double; abs_err() compares against the
    extended values), absax / absaty, bound_ax / bound_aty / bound_aty_prod and near_tie for the unscaled problem p at (x, y)."""
    if exact is None:
        exact = not LONGDOUBLE_IS_EXTENDED
    assert exact or np.finfo(np.longdouble).eps <= 2.0 ** -63
    m, n = int(p["m"]), int(p["n"])
    off, idx = np.asarray(p["offsets"], dtype=np.int64), np.asarray(p["indices"], dtype=np.int64)
    val = _lift(p["values"], exact)
    xe, ye, ce = _lift(x, exact), _lift(y, exact), _lift(p["c"], exact)
    zm, zn = _lift(np.zeros(m), exact), _lift(np.zeros(n), exact)
    lo, hi, lb, ub = (_finite_part(p[k], exact) for k in ("lo", "hi", "lb", "ub"))
    rows = np.repeat(np.arange(m), np.diff(off))
    # ---- rows (EvalPrimalEpilogue)
    prod = val * xe[idx]
    ax, absax = _segment_sums(prod, off, zm), _segment_sums(np.abs(prod), off, zm)
    below = lo[0] & (ax < lo[1])                      # violation(): value < lower, else value > upper, else 0
    above = ~below & hi[0] & (ax > hi[1])
    rp = np.where(below, lo[1] - ax, np.where(above, ax - hi[1], zm))
    bcomb = np.maximum(np.where(hi[0], np.abs(hi[1]), zm), np.where(lo[0], np.abs(lo[1]), zm))  # combine_bounds
    # ---- columns (EvalDualCore)
    order = np.argsort(idx, kind="stable")
    t_off = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n))]).astype(np.int64)
    prod_t = val[order] * ye[rows[order]]
    aty, absaty = _segment_sums(prod_t, t_off, zn), _segment_sums(np.abs(prod_t), t_off, zn)
    g = ce - aty
    gpos = g > 0
    bv_finite, bv = np.where(gpos, lb[0], ub[0]), np.where(gpos, lb[1], ub[1])  # bound_value_gradient
    dist, absx = np.abs(xe - bv), np.abs(xe)
    take = bv_finite if rule_finite else (bv_finite & (dist <= absx))
    rc = np.where(take, g, zn)                        # (g == 0: rc = g = 0 either way)
    rd = g - rc
    # ---- the eight scalars (read_eval)
    want_linf = eps_p >= 0.0 and eps_d >= 0.0
    out = dict(CX=(ce * xe).sum(), X2=(xe * xe).sum(), Y2=(ye * ye).sum(), PRES2=(rp * rp).sum(), DRES2=(rd * rd).sum(),
               DUAL_SUM=_bound_value_product(ye, lo, hi, zm).sum() + _bound_value_product(rc, lb, ub, zn).sum(),
               LINF_PRES_REL=0.0, LINF_DRES_REL=0.0)
    if want_linf:  # max over the rows, clipped at 0 from below (k_max_partials)
        ep, ed = _lift([eps_p], exact)[0], _lift([eps_d], exact)[0]
        out["LINF_PRES_REL"] = max(0, (rp - ep * bcomb).max()) if m else 0.0
        out["LINF_DRES_REL"] = max(0, (rd - ed * ce).max()) if n else 0.0
    out = {k: float(v) for k, v in out.items()}
    # ---- bounds and ties
    len_r, len_c = np.diff(off), np.diff(t_off)
    absax_d, absaty_d = _down(absax), _down(absaty)
    c_d, x_d = np.asarray(p["c"], dtype=np.float64), np.asarray(x, dtype=np.float64)
    out.update(absax=absax_d, absaty=absaty_d, bound_ax=(len_r + 16) * U * absax_d, bound_aty_prod=(len_c + 16) * U * absaty_d,
               bound_aty=(len_c + 16) * U * (absaty_d + np.abs(c_d)))
    absg = np.abs(g)
    tie = (absg > 0) & (absg <= _lift(out["bound_aty"], exact))
    if not rule_finite:
        gap = np.abs(dist - absx)
        tie = tie | (bv_finite & (gap > 0) & (gap <= _lift(16 * U * np.abs(x_d), exact)))
    out.update(near_tie=np.asarray(tie, dtype=bool), g_is_zero=np.asarray(g == 0, dtype=bool), ax=_down(ax), aty=_down(aty), rc=_down(rc),
               _ext=dict(ax=ax, aty=aty, rc=rc), _exact=exact)
    return out


def abs_err(ref, key, got):
    """|got - ref[key]| per element, the difference taken against the extended value"""
    return _down(np.abs(_lift(got, ref["_exact"]) - ref["_ext"][key]))


def worst_ratio(err, bound, where=None):
    """max err / bound over `where`; an error above a zero bound counts as infinite, 0 / 0 as 0"""
    if where is not None:
        err, bound = err[where], bound[where]
    if len(err) == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(r.max())
