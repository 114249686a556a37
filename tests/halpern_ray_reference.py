"""numpy restatement of infeasibility detection in the restarted reflected-Halpern mode (docs/design/04d_halpern_mode.md,
"Infeasibility detection"; the iteration itself is tests/halpern_reference.py, imported and not edited).

The displacement of one PDHG step, D = T(z^k) - z^k, converges to the infimal displacement vector of the operator, which is the
certificate.  At a major iteration whose T(z^k) is not Optimal, the UNSCALED displacement
    dx_u = D_c (x' - x^k),   dy_u = D_r (y' - y^k)
takes the place of the iterate in the infeasibility information of the averaging modes (infeasibility_information.cu:115-223):

  * `ray_info(p, dx_u, dy_u)`: the four figures, both reduced-cost rules;
  * `verdict(f, tol_p, tol_d)`: PrimalInfeasible iff f[3] > 0 and f[2] / f[3] <= tol_p, else DualInfeasible iff f[1] < 0 and
    f[0] / -f[1] <= tol_d -- whether or not T(z^k) is primal feasible;
  * `detect(p, ...)`: the major iterations of halpern_reference.run with the test behind the Optimal check;
  * `with_contradictory_rows`, `with_ray_column`, `with_row_columns_fixed`: the three constructions of the tests."""
import numpy as np

import halpern_reference as H

KEYS = ("max_primal_ray_infeasibility", "primal_ray_linear_objective", "max_dual_ray_infeasibility", "dual_ray_linear_objective")
INF = float("inf")


def _bound_value_product(v, lower, upper):
    """sum-and term B(v, lower, upper): v times the bound its sign selects, 0 where that bound is infinite"""
    return np.where(v > 0, np.where(np.isfinite(lower), lower, 0.0) * v, np.where(np.isfinite(upper), upper, 0.0) * v)


def ray_info(p, dx_u, dy_u, finite_bounds_rule=True):
    """the four figures of the infeasibility information with (dx_u, dy_u) as the ray estimate -> dict over KEYS"""
    A = H.csr_of(p)
    sgn = -1.0 if p.get("maximize") else 1.0
    c = sgn * np.asarray(p["c"], float)
    lo, hi, lb, ub = (np.asarray(p[k], float) for k in ("lo", "hi", "lb", "ub"))
    x, y = np.asarray(dx_u, float), np.asarray(dy_u, float)
    # rows: violation of A x against the homogeneous bounds (a finite bound becomes 0, an infinite one stays), ||y||_inf, sum B(y)
    ax = A @ x
    hl, hu = np.where(np.isfinite(lo), 0.0, lo), np.where(np.isfinite(hi), 0.0, hi)
    max_primal = float(np.max(np.maximum(np.maximum(hl - ax, ax - hu), 0.0), initial=0.0))
    y_inf = float(np.max(np.abs(y), initial=0.0))
    sum_by = float(_bound_value_product(y, lo, hi).sum())
    # columns: g = -A^T y, the reduced cost by the preset's rule (both use the ray's own x), ||g - rc||_inf, ||rc||_inf, ||x||_inf,
    # the violation of the homogeneous variable bounds, sum B(rc), c . x
    g = -1.0 * (A.T @ y)
    bv = np.where(g > 0, lb, ub)
    if finite_bounds_rule:
        take = np.isfinite(bv)
    else:
        with np.errstate(invalid="ignore"):
            take = np.abs(x - bv) <= np.abs(x)
    rc = np.where((g == 0) | take, g, 0.0)
    max_dual = float(np.max(np.abs(g - rc), initial=0.0))
    rc_inf = float(np.max(np.abs(rc), initial=0.0))
    x_inf = float(np.max(np.abs(x), initial=0.0))
    viol = np.maximum(np.where(np.isfinite(lb), -x, 0.0), np.where(np.isfinite(ub), x, 0.0))
    max_viol = float(np.max(np.maximum(viol, 0.0), initial=0.0))
    sum_brc = float(_bound_value_product(rc, lb, ub).sum())
    cx = float(c @ x)
    # compute_remaining_stats_kernel, infeasibility_information.cu:115-172
    primal_obj = 0.0 if x_inf == 0.0 else cx * (1.0 / x_inf)
    dual_obj = sum_by + sum_brc
    scaling = max(y_inf, rc_inf)
    if scaling != 0.0:
        max_dual /= scaling
        dual_obj /= scaling
    else:
        max_dual, dual_obj = 0.0, 0.0
    if x_inf > 0.0:
        max_primal = max(max_primal, max_viol) / x_inf
    else:
        max_primal, primal_obj = 0.0, 0.0
    return dict(zip(KEYS, (max_primal, primal_obj, max_dual, dual_obj)))


def verdict(f, tol_p=1e-8, tol_d=1e-8):
    """f: dict over KEYS or the four figures in that order -> "PrimalInfeasible", "DualInfeasible" or None"""
    f = [f[k] for k in KEYS] if isinstance(f, dict) else list(f)
    if f[3] > 0.0 and f[2] / f[3] <= tol_p:
        return "PrimalInfeasible"
    if f[1] < 0.0 and f[0] / -f[1] <= tol_d:
        return "DualInfeasible"
    return None


def detect(p, eps=1e-8, tol_p=1e-8, tol_d=1e-8, max_iterations=100000, restarts=True, major=H.MAJOR_ITERATION, finite_bounds_rule=True,
           theta=H.THETA):
    """the mode's major iterations with the ray test behind the Optimal check (restarts as halpern_reference.run makes them)
    -> dict(status, iterations, figures [of the last test], dx, dy [the unscaled displacement of the last test], restarts)"""
    A = H.csr_of(p)
    B, dr, dc, c, lb, ub, lo, hi = H.scaled_problem(p)
    sigma_max, _ = H.power_iteration(B)
    eta = H.STEP_SAFETY / sigma_max if sigma_max > 0 else 1.0
    it = H.HalpernIteration(B, c, lb, ub, lo, hi, eta, H.initial_weight(c, lo, hi))
    total, r_prev, n_restarts = 0, None, 0
    out = dict(status="IterationLimit", figures=None, dx=None, dy=None)
    while total < max_iterations:
        for _ in range(major):
            xk, yk = it.x, it.y  # (step() rebinds both: z^k of the period's last step stays here)
            it.step()
        total += major
        if H.optimal(H.convergence(p, A, it.tx * dc, it.ty * dr), eps):
            out["status"] = "Optimal"
            break
        dx, dy = dc * (it.tx - xk), dr * (it.ty - yk)
        f = ray_info(p, dx, dy, finite_bounds_rule)
        out.update(figures=f, dx=dx, dy=dy)
        v = verdict(f, tol_p, tol_d)
        if v:
            out["status"] = v
            break
        r, r0 = it.r, it.r_first
        do = restarts and (r <= H.SUFFICIENT * r0 or (r <= H.NECESSARY * r0 and r_prev is not None and r > r_prev) or
                           it.k >= H.ARTIFICIAL * total)
        r_prev = r
        if do:
            it.restart(theta)
            r_prev = None
            n_restarts += 1
    out.update(iterations=total, restarts=n_restarts)
    return out


# ---- the three constructions ------------------------------------------------------------------------------------------------------
def _copy(p):
    q = dict(p)
    for k in ("offsets", "indices", "values", "c", "lo", "hi", "lb", "ub"):
        q[k] = np.array(p[k], dtype=np.int32 if k in ("offsets", "indices") else float)
    q.pop("objective_star", None)
    return q


def with_contradictory_rows(p):
    """two appended rows over columns 0..4 with coefficients 1: one >= 10, one <= 5"""
    q = _copy(p)
    cols = np.arange(min(5, int(p["n"])), dtype=np.int32)
    nnz = int(q["offsets"][-1])
    q["indices"] = np.concatenate([q["indices"], cols, cols]).astype(np.int32)
    q["values"] = np.concatenate([q["values"], np.ones(2 * len(cols))])
    q["offsets"] = np.concatenate([q["offsets"], [nnz + len(cols), nnz + 2 * len(cols)]]).astype(np.int32)
    q["lo"] = np.concatenate([q["lo"], [10.0, -INF]])
    q["hi"] = np.concatenate([q["hi"], [INF, 5.0]])
    q["m"] = int(p["m"]) + 2
    return q


def with_ray_column(p):
    """an appended column with min-form cost -1 and bounds [0, inf); its single entry 1 sits in an appended row >= 0"""
    q = _copy(p)
    n, nnz = int(p["n"]), int(q["offsets"][-1])
    q["indices"] = np.concatenate([q["indices"], [n]]).astype(np.int32)
    q["values"] = np.concatenate([q["values"], [1.0]])
    q["offsets"] = np.concatenate([q["offsets"], [nnz + 1]]).astype(np.int32)
    q["c"] = np.concatenate([q["c"], [1.0 if p.get("maximize") else -1.0]])
    q["lb"] = np.concatenate([q["lb"], [0.0]])
    q["ub"] = np.concatenate([q["ub"], [INF]])
    q["lo"] = np.concatenate([q["lo"], [0.0]])
    q["hi"] = np.concatenate([q["hi"], [INF]])
    q["m"], q["n"] = int(p["m"]) + 1, n + 1
    if "var_types" in q:
        q.pop("var_types")
    return q


def row_columns(p, i):
    return np.asarray(p["indices"])[int(p["offsets"][i]):int(p["offsets"][i + 1])]


def with_row_columns_fixed(p, i):
    """ub = 0 on every column of row i, whose lo must be > 0 (bounds only, as a branching does it)"""
    assert float(p["lo"][i]) > 0.0
    q = _copy(p)
    q["ub"][row_columns(p, i)] = 0.0
    return q


def farkas_violation(p, dy):
    """relative failure of dy as a Farkas certificate of primal infeasibility: with g = -A^T dy and the reduced costs of the
    finite-bounds rule, (||g - rc||_inf) / (sum B(dy, lo, hi) + sum B(rc, lb, ub)); the denominator must be positive
    -> (ratio, denominator)"""
    A = H.csr_of(p)
    lo, hi, lb, ub = (np.asarray(p[k], float) for k in ("lo", "hi", "lb", "ub"))
    g = -1.0 * (A.T @ dy)
    bv = np.where(g > 0, lb, ub)
    rc = np.where(np.isfinite(bv), g, 0.0)
    den = float(_bound_value_product(dy, lo, hi).sum() + _bound_value_product(rc, lb, ub).sum())
    return float(np.max(np.abs(g - rc), initial=0.0)) / den if den > 0 else INF, den
