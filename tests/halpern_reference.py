"""numpy restatement of the restarted reflected-Halpern PDHG mode (solver mode 4, docs/design/04d_halpern_mode.md).

Written from the mode's specification, not from the device code: the tests hold the HIP kernels and the host driver against it.

On the scaled problem (Ruiz, 10 rounds, then Pock-Chambolle with alpha = 1), T(z) = (x', y') is one PDHG step
    x' = proj_[lb, ub](x - tau (c - A^T y)),   y' = max(n + sigma lo, min(n + sigma hi, 0)),  n = y - sigma A (2 x' - x),
with tau = eta / omega, sigma = eta omega, and the iteration is
    z^{k+1} = w_k (2 T(z^k) - z^k) + (1 - w_k) z^0,   w_k = (k + 1) / (k + 2),
k = steps since the last restart, z^0 = the iterate at the last restart.  A^T y^{k+1} is formed by the same linear combination from
A^T y', A^T y^k and A^T y^0 (the variant the device layer uses: no third product per step).

  * `ruiz_pock_chambolle`, `power_iteration`, `initial_weight`: what precedes the first step;
  * `HalpernIteration`: the iteration on a scaled problem given eta and omega (the GPU tests feed it the DEVICE's scaled problem, step
    size and weight, so that a comparison sees the kernels alone);
  * `run`: major iterations (evaluation of T(z^k) on the unscaled problem, termination, the three restart tests, the weight update);
  * `solve`: everything from the user's LP."""
import numpy as np
import scipy.sparse as sp

STEP_SAFETY = 0.998
POWER_TOLERANCE = 1e-6
POWER_MAX_PRODUCTS = 5000
MAJOR_ITERATION = 40
SUFFICIENT, NECESSARY, ARTIFICIAL = 0.2, 0.8, 0.36
THETA = 0.99


def csr_of(p):
    return sp.csr_matrix((np.asarray(p["values"], float), np.asarray(p["indices"]), np.asarray(p["offsets"])),
                         shape=(int(p["m"]), int(p["n"])))


def ruiz_pock_chambolle(A, ruiz=10, alpha=1.0):
    """-> (D_r A D_c, D_r, D_c): `ruiz` rounds of inf-norm equilibration, both sides from the same snapshot, then Pock-Chambolle"""
    m, n = A.shape
    dr, dc = np.ones(m), np.ones(n)
    B = A.copy().tocsr()
    for _ in range(ruiz):
        Ba = abs(B)
        r = np.sqrt(np.maximum(Ba.max(axis=1).toarray().ravel(), 0))
        c = np.sqrt(np.maximum(Ba.max(axis=0).toarray().ravel(), 0))
        r[r == 0] = 1
        c[c == 0] = 1
        B = sp.diags(1 / r) @ B @ sp.diags(1 / c)
        dr /= r
        dc /= c
    Ba = abs(B)
    r = np.sqrt(np.asarray(Ba.power(alpha).sum(axis=1)).ravel())
    c = np.sqrt(np.asarray(Ba.power(2 - alpha).sum(axis=0)).ravel())
    r[r == 0] = 1
    c[c == 0] = 1
    B = sp.diags(1 / r) @ B @ sp.diags(1 / c)
    return B.tocsr(), dr / r, dc / c


def power_iteration(B, tol=POWER_TOLERANCE, max_products=POWER_MAX_PRODUCTS):
    """-> (estimate of sigma_max(B), products of B^T B formed): from 1 / sqrt(n), until ||B^T B v|| moves by at most tol relative"""
    BT = B.T.tocsr()
    n = B.shape[1]
    v = np.full(n, 1.0 / np.sqrt(n))
    est, done = 0.0, 0
    while done < max_products:
        w = BT @ (B @ v)
        s2 = np.linalg.norm(w)
        done += 1
        if not s2 > 0.0:
            est = 0.0
            break
        v = w / s2
        settled = abs(s2 - est) <= tol * s2
        est = s2
        if settled:
            break
    return np.sqrt(est), done


def combine_finite_abs_bounds(lo, hi):
    return np.maximum(np.where(np.isfinite(lo), np.abs(lo), 0.0), np.where(np.isfinite(hi), np.abs(hi), 0.0))


def initial_weight(c, lo, hi):
    nc, nb = np.linalg.norm(c), np.linalg.norm(combine_finite_abs_bounds(lo, hi))
    return nc / nb if nc > 0 and nb > 0 else 1.0


class HalpernIteration:
    """the iteration on a SCALED problem; `step` returns r_k^2 of the step it took and keeps T(z^k) in `.tx`, `.ty`"""

    def __init__(self, B, c, lb, ub, lo, hi, eta, omega, x=None, y=None):
        self.B = sp.csr_matrix(B)
        self.BT = self.B.T.tocsr()
        m, n = self.B.shape
        self.c, self.lb, self.ub, self.lo, self.hi = (np.asarray(v, float) for v in (c, lb, ub, lo, hi))
        self.eta, self.omega = float(eta), float(omega)
        self.x = np.minimum(np.maximum(np.zeros(n) if x is None else np.asarray(x, float), self.lb), self.ub)
        self.y = np.zeros(m) if y is None else np.asarray(y, float).copy()
        self.aty = self.BT @ self.y
        self.k = 0
        self.r = self.r_first = self.r2 = 0.0
        self.tx, self.ty = self.x.copy(), self.y.copy()
        self._anchor()

    def _anchor(self):
        self.x0, self.y0, self.aty0 = self.x.copy(), self.y.copy(), self.aty.copy()

    def operator(self, x, y, aty):
        """T(z) and A^T y' for a point given with its A^T y"""
        tau, sigma = self.eta / self.omega, self.eta * self.omega
        xp = np.maximum(np.minimum(x - tau * (self.c - aty), self.ub), self.lb)
        v = self.B @ (xp - x + xp)
        nxt = y - sigma * v
        yp = np.maximum(nxt + sigma * self.lo, np.minimum(nxt + sigma * self.hi, 0.0))
        return xp, yp, self.BT @ yp

    def metric2(self, dx, dy, at_dy):
        """||(dx, dy)||_M^2 of PDHG's metric under this sign convention; at_dy = A^T dy"""
        return (self.omega / self.eta) * (dx @ dx) + 2.0 * (dx @ at_dy) + (dy @ dy) / (self.eta * self.omega)

    def step(self):
        xp, yp, atyp = self.operator(self.x, self.y, self.aty)
        r2 = self.metric2(xp - self.x, yp - self.y, atyp - self.aty)
        self.r2, self.r = r2, np.sqrt(max(r2, 0.0))
        if self.k == 0:
            self.r_first = self.r
        w = (self.k + 1.0) / (self.k + 2.0)
        w0 = 1.0 - w
        self.x = w * (2.0 * xp - self.x) + w0 * self.x0
        self.y = w * (2.0 * yp - self.y) + w0 * self.y0
        self.aty = w * (2.0 * atyp - self.aty) + w0 * self.aty0
        self.tx, self.ty = xp, yp
        self.k += 1
        return r2

    def restart(self, theta=THETA):
        """-> (||x - x0||, ||y - y0||); smooths the weight when both exceed 1e-10 (theta < 0: never), moves the anchor, k <- 0"""
        dx, dy = np.linalg.norm(self.x - self.x0), np.linalg.norm(self.y - self.y0)
        if theta >= 0 and dx > 1e-10 and dy > 1e-10:
            self.omega = float(np.exp(theta * np.log(dy / dx) + (1 - theta) * np.log(self.omega)))
        self._anchor()
        self.k = 0
        return dx, dy


def convergence(p, A, xu, yu):
    """convergence information of an UNSCALED point: min-form objectives, l2 residuals, gap; -> dict"""
    sgn = -1.0 if p.get("maximize") else 1.0
    c0 = sgn * np.asarray(p["c"], float)
    lo, hi, lb, ub = (np.asarray(p[k], float) for k in ("lo", "hi", "lb", "ub"))
    ax = A @ xu
    viol = np.maximum(lo - ax, 0) + np.maximum(ax - hi, 0)
    g = c0 - A.T @ yu
    rc = np.where(g > 0, np.where(np.isfinite(lb), g, 0.0), np.where(np.isfinite(ub), g, 0.0))

    def bound_value(v, lower, upper):
        return np.where(v > 0, np.where(np.isfinite(lower), lower, 0.0) * v, np.where(np.isfinite(upper), upper, 0.0) * v)

    pobj, dobj = float(c0 @ xu), float(bound_value(yu, lo, hi).sum() + bound_value(rc, lb, ub).sum())
    return dict(primal_objective=pobj, dual_objective=dobj, gap=abs(pobj - dobj), primal_residual=float(np.linalg.norm(viol)),
                dual_residual=float(np.linalg.norm(g - rc)), norm_b=float(np.linalg.norm(combine_finite_abs_bounds(lo, hi))),
                norm_c=float(np.linalg.norm(c0)))


def optimal(cv, eps):
    return (cv["primal_residual"] <= eps + eps * cv["norm_b"] and cv["dual_residual"] <= eps + eps * cv["norm_c"] and
            cv["gap"] <= eps + eps * (abs(cv["primal_objective"]) + abs(cv["dual_objective"])))


def run(p, it, dr, dc, eps=1e-4, max_iterations=200000, max_major=None, restarts=True, major=MAJOR_ITERATION, theta=THETA):
    """major iterations of a HalpernIteration `it` on the LP `p` whose scaling is (dr, dc) -> dict(status, iterations, objective,
    restarts, flags [a bool per major iteration that did not terminate], weights [omega after each major iteration])"""
    A = csr_of(p)
    sgn = -1.0 if p.get("maximize") else 1.0
    offset = float(p.get("objective_offset", 0.0))
    total, r_prev, n_restarts, flags, weights, majors = 0, None, 0, [], [], 0
    cv = None
    while total < max_iterations and (max_major is None or majors < max_major):
        for _ in range(major):
            it.step()
        total += major
        majors += 1
        cv = convergence(p, A, it.tx * dc, it.ty * dr)
        if optimal(cv, eps):
            return dict(status="Optimal", iterations=total, objective=sgn * cv["primal_objective"] + offset, restarts=n_restarts,
                        flags=flags, weights=weights, x=it.tx * dc, y=it.ty * dr)
        r, r0 = it.r, it.r_first
        do = restarts and (r <= SUFFICIENT * r0 or (r <= NECESSARY * r0 and r_prev is not None and r > r_prev) or
                           it.k >= ARTIFICIAL * total)
        r_prev = r
        if do:
            it.restart(theta)
            r_prev = None
            n_restarts += 1
        flags.append(bool(do))
        weights.append(it.omega)
    obj = sgn * cv["primal_objective"] + offset if cv else float("nan")
    return dict(status="IterationLimit", iterations=total, objective=obj, restarts=n_restarts, flags=flags, weights=weights,
                x=it.tx * dc, y=it.ty * dr)


def scaled_problem(p):
    """-> (B, dr, dc, c, lb, ub, lo, hi) of the min-form LP after the mode's scaling"""
    sgn = -1.0 if p.get("maximize") else 1.0
    B, dr, dc = ruiz_pock_chambolle(csr_of(p))
    return (B, dr, dc, sgn * np.asarray(p["c"], float) * dc, np.asarray(p["lb"], float) / dc, np.asarray(p["ub"], float) / dc,
            np.asarray(p["lo"], float) * dr, np.asarray(p["hi"], float) * dr)


def solve(p, eps=1e-4, max_iterations=200000, **kw):
    B, dr, dc, c, lb, ub, lo, hi = scaled_problem(p)
    sigma_max, _ = power_iteration(B)
    eta = STEP_SAFETY / sigma_max if sigma_max > 0 else 1.0
    it = HalpernIteration(B, c, lb, ub, lo, hi, eta, initial_weight(c, lo, hi))
    return run(p, it, dr, dc, eps=eps, max_iterations=max_iterations, **kw)
