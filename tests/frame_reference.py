"""TEST UTILITY: the frame around the iteration restated -- the scaling, the norms that set the first step, the primal weight and the
termination thresholds, the start, the reset and the read-back -- in the style of tests/eval_reference.py (whose helpers it uses).
numpy only.

What it restates is this repository's own device code: pdlpdev_scaling_compute and pdlpdev_scale_problem (cuopt_amd/csrc/
pdlp_scaling.hip), pdlpdev_init_norms, pdlpdev_weight_norms, pdlpdev_problem_norms, pdlpdev_initial_solution_stats, pdlpdev_set_initial,
pdlpdev_project_primal, pdlpdev_reset and pdlpdev_get_solution (pdlp_device.hip).

BIT FOR BIT (the library is built with -ffp-contract=off; float64 numpy, the kernels' order of operations):

  the scaling.  One pass takes, from the D_r and D_c in front of it,
      v_k = |fl(fl(a_k D_r[i]) D_c[j])|                                       (every norm kernel of A forms this;
                                                                               those of A^T the same product as (a d_row[j]) d_col[r])
      Ruiz:            norm_i = max_k v_k over row i,  norm_j = max over column j      (order independent)
      Pock-Chambolle:  norm_i = ((0 + v_k0) + v_k1) + ...   over row i in CSR order    (alpha = 1: no pow())
                       norm_j = the same over column j, its entries by ascending row   (A^T is the stable transposition of A)
      d <- fl(d / fl(sqrt(norm)))   where norm > 0; an empty row or column keeps its d (1.0 from start to end)
  both sides' norms before either division.  The sums are added with "the k-th entry of every row that has one" for k = 0, 1, ...:
  every row left to right, one vector operation per k, nothing left to a library's reduction order.
      A_VALUES = fl(fl(a D_r[i]) D_c[j])     AT_VALUES = fl(fl(a D_c[j]) D_r[i])    (the two may differ in the last bit)
      C = c D_c    LB = lb / D_c    UB = ub / D_c    LO = lo D_r    HI = hi D_r     (an infinite bound stays infinite: D > 0)

  max|.|;  x0 / D_c, y0 / D_r;  min(max(x, lb), ub) as (x > lb ? x : lb) < ub ? . : ub;  xhat D_c, yhat D_r.

EXACT VALUE AND BOUND (u = 2^-53, gamma_k = k u / (1 - k u); Higham, Accuracy and Stability of Numerical Algorithms, sections 3.1, 4.2):

  a sum of N squares, S = sum v_i^2.  The device rounds each square once and adds the N rounded squares in SOME tree (a lane's
  grid-stride loop, the wave's and the workgroup's trees, k_finalize over the workgroups' partials; a 0.0 a lane starts from or a
  workgroup without an element contributes adds exactly).  A term passes through at most N - 1 additions, so it carries at most N
  factors (1 + delta), |delta| <= u:            |got - S| <= gamma_N S                                     (every term is >= 0)
  combine_bounds(lo, hi) selects |lo|, |hi| or 0.0 and rounds nothing: sum combine_bounds^2 has the same bound.
  a dot product x . a:  one rounding per product, N - 1 additions:  |got - x . a| <= gamma_N sum |x_j a_j|.
  under row sharding with `world` ranks the all-reduce adds the ranks' partial sums in one more tree of at most world - 1 additions:
  gamma_{N + world - 1}, which the tests round up to gamma_{N + world}.
  pdlpdev_problem_norms returns fl(sqrt(got)):  with |got - S| <= g S, g = gamma_N, |sqrt(1 + t) - 1| <= |t| / (2 (1 - |t|)) for |t| < 1
  and one more rounding                         |norm - sqrt(S)| <= (h + u (1 + h)) sqrt(S),  h = g / (2 (1 - g))
  (it follows from the line above and is what norm_of() returns).
  the interaction of pdlpdev_initial_solution_stats from the device's OWN product t^ = A^T y0 has the dot product's bound.  Where the
  product itself is not visible (the sharded call) the bound carries it:  |t^_j - t_j| <= (L_j + 16) u sum_i |a_ij y_i| =: B_j
  (tests/attempt_reference.aty_product, which holds for the ranks' partial products added in rank order as it stands), so
  |got - x . t| <= gamma_n sum |x_j| (|t_j| + B_j) + sum |x_j| B_j.

Every sum of the reference itself is taken in np.longdouble (64-bit significand: its own error is at most N 2^-64 of the same
magnitude, 1/2048 of the bound), or in exact rationals where the platform's long double is no wider than a double.  The bounds are
derived, not measured: a figure outside of one is a finding about the kernel."""
import math

import numpy as np

from attempt_reference import Structure, _dmax, _dmin, _exact
from eval_reference import U, _lift

INF = np.inf


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- the scaling ---------------------------------------------------------------------------------------------------------------------
def rows_left_to_right(v, off):
    """((0.0 + v[off[r]]) + v[off[r] + 1]) + ... per row in float64: the k-th entry of every row that has one, k = 0, 1, ..."""
    off = np.asarray(off, dtype=np.int64)
    lens, acc = np.diff(off), np.zeros(len(off) - 1)
    order = np.argsort(-lens, kind="stable")  # (rows by descending length: the rows that have a k-th entry are a prefix)
    sorted_lens = lens[order]
    for k in range(int(lens.max()) if len(lens) else 0):
        r = order[:np.searchsorted(-sorted_lens, -k, side="left")]  # lens > k
        acc[r] = acc[r] + v[off[r] + k]
    return acc


def rows_max(v, off):
    """max per row, 0.0 for an empty one (v >= 0; the maximum is order independent)"""
    off = np.asarray(off, dtype=np.int64)
    out = np.zeros(len(off) - 1)
    ne = np.nonzero(np.diff(off) > 0)[0]
    if len(ne):
        out[ne] = np.maximum.reduceat(v, off[:-1][ne])
    return out


def _div_sqrt(d, norm):
    pos = norm > 0.0
    out = d.copy()
    out[pos] = d[pos] / np.sqrt(norm[pos])
    return out


def scaling_pass(S, values, dr, dc, pock_chambolle, corrupt=None):
    """one pass of pdlpdev_scaling_compute -> (D_r, D_c) behind it.  corrupt = ("reverse_column", j): that column's Pock-Chambolle sum
    added last entry first (tests/test_frame_reference.py: the comparison must notice)"""
    v = np.abs((values * dr[S.rows]) * dc[S.idx])
    vt = np.abs((values[S.order] * dr[S.t_rows]) * dc[S.idx[S.order]])  # A^T's own kernels: (a d_row[j]) d_col[r] per entry of A^T
    if pock_chambolle:
        if corrupt is not None and corrupt[0] == "reverse_column":
            j = corrupt[1]
            vt = vt.copy()
            vt[S.t_off[j]:S.t_off[j + 1]] = vt[S.t_off[j]:S.t_off[j + 1]][::-1].copy()
        nr, nc = rows_left_to_right(v, S.off), rows_left_to_right(vt, S.t_off)
    else:
        nr, nc = rows_max(v, S.off), rows_max(vt, S.t_off)
    return _div_sqrt(dr, nr), _div_sqrt(dc, nc)


def scaling(p, ruiz_iterations=10, pock_chambolle=True, S=None, corrupt=None):
    """pdlpdev_scaling_compute(do_ruiz, ruiz_iterations, do_pc, alpha = 1.0) -> (D_r, D_c)"""
    S = S or Structure(p["m"], p["n"], p["offsets"], p["indices"])
    values = np.asarray(p["values"], dtype=np.float64)
    dr, dc = np.ones(S.m), np.ones(S.n)
    for _ in range(ruiz_iterations):
        dr, dc = scaling_pass(S, values, dr, dc, False)
    if pock_chambolle:
        dr, dc = scaling_pass(S, values, dr, dc, True, corrupt)
    return dr, dc


def scaled_problem(p, dr, dc, S=None, corrupt=None):
    """pdlpdev_scale_problem -> the nine buffers as the device holds them.  corrupt = "at_in_a_order": A^T multiplied like A"""
    S = S or Structure(p["m"], p["n"], p["offsets"], p["indices"])
    values = np.asarray(p["values"], dtype=np.float64)
    at = values[S.order]
    t_cols = S.idx[S.order]
    at_values = (at * dr[S.t_rows]) * dc[t_cols] if corrupt == "at_in_a_order" else (at * dc[t_cols]) * dr[S.t_rows]
    with np.errstate(invalid="ignore"):
        return dict(DROW=dr, DCOL=dc, A_VALUES=(values * dr[S.rows]) * dc[S.idx], AT_VALUES=at_values, C=p["c"] * dc, LB=p["lb"] / dc, UB=p["ub"] / dc,
                    LO=p["lo"] * dr, HI=p["hi"] * dr)


SCALED = ("DROW", "DCOL", "A_VALUES", "AT_VALUES", "C", "LB", "UB", "LO", "HI")


# ---- the norms -----------------------------------------------------------------------------------------------------------------------
def combine_bounds(lo, hi):
    """combine_bounds (pdlp_kernels.hpp) in float64: max(|hi| if finite, |lo| if finite, 0.0) -- a selection, nothing is rounded"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    val = np.zeros(len(lo))
    val = np.where(np.isfinite(hi), _dmax(val, np.abs(hi)), val)
    return np.where(np.isfinite(lo), _dmax(val, np.abs(lo)), val)


def max_abs(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.abs(v).max()) if len(v) else 0.0


def sum_squares(v, extra=0, exact=None):
    """(S, bound): S = sum v_i^2 in extended precision, bound = gamma_{N + extra} S"""
    exact = _exact(exact)
    e = _lift(v, exact)
    s = (e * e).sum() if len(e) else _lift([0.0], exact)[0]
    return s, gamma(len(e) + extra) * float(s)


def dot(x, a, extra=0, exact=None):
    """(x . a, gamma_{N + extra} sum |x_j a_j|)"""
    exact = _exact(exact)
    prod = _lift(x, exact) * _lift(a, exact)
    zero = _lift([0.0], exact)[0]
    return (prod.sum() if len(prod) else zero), gamma(len(prod) + extra) * float(np.abs(prod).sum() if len(prod) else zero)


def norm_of(entry, count):
    """(sqrt(S), bound) of fl(sqrt(got)) from sum_squares' (S, gamma S) over `count` terms (the derivation: this file's first lines)"""
    s, _ = entry
    g = gamma(count)
    h = g / (2.0 * (1.0 - g))
    root = math.sqrt(float(s)) if not isinstance(s, np.longdouble) else np.sqrt(s)
    return root, (h + U * (1.0 + h)) * float(root)


def ratio(entry, got, exact=None):
    """|got - value| / bound of a (value, bound) pair: 0 / 0 is 0, an error above a zero bound infinite"""
    exact = _exact(exact)
    value, bound = entry
    if exact and isinstance(value, float):  # (norm_of's square root under exact rationals: a double)
        err = abs(float(got) - value)
    else:
        err = float(abs(_lift([got], exact)[0] - value))
    return 0.0 if err == 0.0 else (err / bound if bound > 0.0 else math.inf)


def init_norms(prob, extra=0, corrupt=None):
    """pdlpdev_init_norms on the buffers GIVEN (A_VALUES, C, LO, HI) -> max|A| as a double, (c2, bound), (b2, bound).
    corrupt = "b2_from_lo": sum lo^2 over the finite lo; "hi_ignored": hi dropped where lo is finite"""
    lo, hi = np.asarray(prob["LO"], dtype=np.float64), np.asarray(prob["HI"], dtype=np.float64)
    b = combine_bounds(lo, hi)
    if corrupt == "b2_from_lo":
        b = np.where(np.isfinite(lo), np.abs(lo), 0.0)
    elif corrupt == "hi_ignored":
        b = np.where(np.isfinite(lo), np.abs(lo), b)
    return max_abs(prob["A_VALUES"]), sum_squares(prob["C"]), sum_squares(b, extra)


def problem_norms(c, lo, hi, extra=0):
    """pdlpdev_problem_norms on the caller's c, lo, hi -> (||c||, bound), (||b||, bound)"""
    return norm_of(sum_squares(c), len(c)), norm_of(sum_squares(combine_bounds(lo, hi), extra), len(lo) + extra)


# ---- the element-wise outputs -----------------------------------------------------------------------------------------------------------
def to_scaled_start(x0, y0, dr, dc):
    """pdlpdev_set_initial: (x0 / D_c, y0 / D_r)"""
    return np.asarray(x0, dtype=np.float64) / dc, np.asarray(y0, dtype=np.float64) / dr


def clamp(x, lb, ub):
    """k_clamp: dmin(dmax(x, lb), ub)"""
    return _dmin(_dmax(np.asarray(x, dtype=np.float64), lb), ub)


def unscaled(xhat, yhat, dr, dc, corrupt=None):
    """k_unscale: (xhat D_c, yhat D_r).  corrupt = "y_with_dc": the dual side multiplied by D_c's first entries"""
    d = np.resize(dc, len(dr)) if corrupt == "y_with_dc" else dr
    return xhat * dc, yhat * d


def initial_stats(x, y, aty, extra=0):
    """the five outputs of pdlpdev_initial_solution_stats from the vectors GIVEN (aty: the product the call left):
    (interaction, bound), (x2, bound), (y2, bound), max|x|, max|y|"""
    return dot(x, aty), sum_squares(x), sum_squares(y, extra), max_abs(x), max_abs(y)


def interaction_through_product(x, product):
    """the interaction where the device's own product is not visible (the sharded call): `product` is attempt_reference.aty_product's
    dict, whose bound B holds for the ranks' partial products added in rank order as it stands (that file's section on the sharded path)
    -> (x . t, gamma_n sum |x_j| (|t_j| + B_j) + sum |x_j| B_j)"""
    exact = product["_exact"]
    xe, t = _lift(x, exact), product["_ext"]
    mag = float((np.abs(xe) * np.abs(t)).sum())
    carried = float((np.abs(np.asarray(x, dtype=np.float64)) * product["bound"]).sum())
    return (xe * t).sum(), gamma(len(xe)) * (mag + carried) + carried
