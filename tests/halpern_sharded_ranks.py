"""TEST UTILITY: W ranks of a row-block sharded context in reflected-Halpern mode (cuoptamd_settings::halpern_sharded) behind the interface
tests/halpern_step_scenario.py documents in its first lines, so that the scenario and tests/halpern_step_reference.py check the sharded
Halpern step on the GLOBAL LP, unchanged.  Built on tests/sharded_ranks.py: the worker threads, the command protocol and its failure
rules, and the assembly of row blocks and slices are that module's.

What HalpernAssembled adds to sharded_ranks.Assembled:
    hal()              rank 0's pdlpdev_halpern; all five fields are the same on every rank
    halpern_restart    the two distances are the same bits on every rank (the weight: part of ctl(), which is compared field by field)
    get("PART_A")      the ranks' dy2 partials side by side
    get("PART_AT")     all ranks' interaction partials, then all ranks' dx2 partials (each rank holds its column block's: interaction
                       first, dx2 behind).  halpern_step_reference's bound "(nb + 16) u sum |partial| for any summation tree" then
                       covers the reduction over the ranks in rank order, with nb the total count: a rank's sum of its own partials
                       and the W - 1 additions behind it are one tree over all of them.
    spectral_norm      sigma_max is the same bits on every rank
A rank is capi.Solver(p, mode=4, halpern_sharded=1, rank=, world=, comm_id=) prepared as test_halpern_step_layouts_gpu.prepared prepares
a single context: eta = STEP_SAFETY / sigma_max from the sharded power iteration, omega from the norms of c and b, the start scaled and
projected, A^T y, the start its own anchor."""
import numpy as np

import attempt_reference as ar
import halpern_reference as H
import sharded_ranks as sr
from eval_reference import _segment_sums

MOST_PARTIALS = 1 << 16
PARTIALS = ("PART_A", "PART_AT")


class HalpernRank(sr.RankOnDevice):
    def __init__(self, p, x0, y0, sp, rank, world, cid, solver_kw):
        from cuopt_amd import capi
        self.capi = capi
        self.solver = capi.Solver(p, mode=4, halpern_sharded=1, rank=rank, world=world, comm_id=cid, **solver_kw)
        self.dev = d = self.solver.device
        self.r0, self.r1 = self.solver.row_range()
        self.n, self.ml = int(p["n"]), self.r1 - self.r0
        self.nnz = int(p["offsets"][self.r1]) - int(p["offsets"][self.r0])
        self.sigma_max, products = d.spectral_norm()
        assert self.sigma_max > 0.0 and 1 <= products <= 5000
        nr = d.init_norms()
        omega = np.sqrt(nr[1]) / np.sqrt(nr[2]) if nr[1] > 0 and nr[2] > 0 else 1.0
        d.call("set_step", H.STEP_SAFETY / self.sigma_max, omega)
        d.call("set_initial", capi._ptr(np.ascontiguousarray(x0, dtype=np.float64)), capi._ptr(np.ascontiguousarray(y0[self.r0:self.r1], dtype=np.float64)))
        d.call("project_primal")
        d.call("compute_aty")
        d.halpern_restart(-1.0)

    def _count(self, name):
        return MOST_PARTIALS if name in PARTIALS else super()._count(name)

    def get_many(self, names):
        out = super().get_many(names)
        for k in names:
            assert k not in PARTIALS or len(out[k]) < MOST_PARTIALS, "more partials than the test downloads"
        return out

    def run(self, target):
        return ar.ctl_dict(self.dev.run(target))

    def hal(self):
        return self.dev.halpern()  # (as the last ctl() / run() / restart read it back)

    def halpern_restart(self, theta):
        return np.array(self.dev.halpern_restart(theta)[:2], dtype=np.float64)

    def spectral_norm(self):
        return float(self.dev.spectral_norm()[0])

    def sigma(self):
        return float(self.sigma_max)


class HalpernDeviceRanks(sr.DeviceRanks):
    def _worker(self, rank, p, x0, y0, sp, solver_kw):
        # (sharded_ranks.DeviceRanks._worker with the Halpern rank in RankOnDevice's place)
        try:
            rk = HalpernRank(p, x0, y0, sp, rank, self.world, self.cid, solver_kw)
            self.answers.put((rank, True, None))
        except BaseException as e:
            self.answers.put((rank, False, ("set-up: %r" % (e,), getattr(e, "code", 0))))
            return
        while True:
            item = self.inbox[rank].get()
            if item is None:
                break
            op, args = item
            try:
                self.answers.put((rank, True, getattr(rk, op)(*args)))
            except BaseException as e:
                self.answers.put((rank, False, ("%s%r: %r" % (op, args[:1], e), getattr(e, "code", 0))))
        try:
            rk.close()
        except Exception:
            pass


class HalpernAssembled(sr.Assembled):
    def hal(self):
        hs = self.b.each("hal")
        for r, h in enumerate(hs):
            assert h == hs[0] or all(ar.bits_equal([h[k]], [hs[0][k]]) for k in hs[0]), ("pdlpdev_halpern of rank %d differs from rank 0's" % r, h, hs[0])
        return dict(hs[0])

    def get(self, name):
        if name not in PARTIALS:
            return super().get(name)
        per = self._fetch(name)
        if name == "PART_A":
            return np.concatenate(per)
        assert all(len(a) % 2 == 0 for a in per), [len(a) for a in per]
        return np.concatenate([a[:len(a) // 2] for a in per] + [a[len(a) // 2:] for a in per])

    def run(self, target):
        cs = self._do("run", int(target))
        return cs[0]

    def halpern_restart(self, theta):
        dist = self._do("halpern_restart", float(theta))
        for r, d in enumerate(dist):
            assert ar.bits_equal(d, dist[0]), ("halpern_restart: rank %d returns other distances than rank 0" % r, list(d), list(dist[0]))
        return float(dist[0][0]), float(dist[0][1])

    def sigma_max(self, again=False):
        """sigma_max as every rank's set-up found it (again: a fresh power iteration on every rank) -- the same bits on all ranks"""
        ss = self._do("spectral_norm") if again else self.b.each("sigma")
        assert all(s == ss[0] for s in ss), ("sigma_max differs between the ranks", ss)
        return ss[0]


def on_device(p, x0, y0, world, **solver_kw):
    """-> HalpernAssembled over W prepared device ranks on the owner-computes dataflow (CUOPT_AMD_SHARD_DATAFLOW is the caller's: unset or owner)"""
    ranks = HalpernDeviceRanks(p, x0, y0, None, world, "owner", **solver_kw)
    try:
        return HalpernAssembled(ranks, None)
    except BaseException:
        ranks.close()
        raise


# ---- W float64 stand-in ranks on the host ------------------------------------------------------------------------------------------------
class HalpernStandInRanks(sr.StandInRanks):
    """sharded_ranks.StandInRanks with the Halpern step of cuopt_amd/csrc/pdlp_device.hip enqueue_attempt (owner-computes dataflow) in
    the averaging attempt's place: k_primal on the slice, the rows of A with y' into AVG_Y and the gathered dual, the column block
    with the combination on sliced anchors, the three sums added in rank order, one decision for all ranks; run_epilogue replicates
    X, ATY and x' of the run's last step (AVG_X) from their owners.  Whatever a rank does not own at that point of the dataflow is
    NaN: a stale entry that the assembly (or the stand-in itself) read would poison everything behind it.  float64, numpy's own order
    inside a rank.  It stands in for the device where the assembly, the LPs and the scenario are tested without one; it is no second
    reference."""

    def __init__(self, S, prob, x, y, dr, dc, world, bounds, sigma_max):
        super().__init__(S, prob, None, x, y, dr, dc, world, "owner", bounds)
        self.sigma_max = float(sigma_max)
        for k in self.ranks:
            k.h = dict(r=0.0, r_first=0.0, r2=0.0, r2_min=np.inf, k=0)
            k.v.update(LAST_RESTART_ATY=np.zeros(S.n), PART_A=np.zeros(1), PART_AT=np.zeros(2))
            k.xp = None  # x' of a run's last step, on the slice

    def _hal(self):
        return [dict(k.h) for k in self.ranks]

    def _sigma(self):
        return [self.sigma_max] * self.world

    def _one_step(self, last):
        import halpern_step_reference as hr
        P, S = self.prob, self.S
        c0 = self.ranks[0].c
        if c0["error"] or c0["steps_taken"] >= c0["target_steps"]:
            return
        trial, whole = [], np.full(self.n, np.nan)
        for k in self.ranks:  # k_primal on the slice, pending_avg = 0
            c, cur, a, b = k.c, k.c["cur"], k.c0, k.c0 + k.nc
            x, aty = k.x[cur][a:b], k.aty[cur][a:b]
            nxt = x - c["tau"] * (P["C"][a:b] - aty)
            nxt = np.where(nxt < P["UB"][a:b], nxt, P["UB"][a:b])
            nxt = np.where(nxt > P["LB"][a:b], nxt, P["LB"][a:b])
            xbar = np.full(self.n, np.nan)
            xbar[a:b] = nxt - x + nxt
            k.v["XBAR"] = xbar
            whole[a:b] = xbar[a:b]  # (the all-gather: every slice from its owner)
            trial.append(nxt)
        assert np.isfinite(whole).all()
        yps, dy2 = [], []
        for k in self.ranks:  # the rows of A with HalpernShardedDualEpilogue
            c, cur = k.c, k.c["cur"]
            y = k.y[cur]
            ax = _segment_sums(k.val * whole[k.idx], k.off, np.zeros(k.r1 - k.r0))
            ny = y - c["sigma"] * ax
            with np.errstate(invalid="ignore", over="ignore"):
                low, up = ny + c["sigma"] * P["LO"][k.r0:k.r1], ny + c["sigma"] * P["HI"][k.r0:k.r1]
                inner = np.where(up < 0.0, up, 0.0)
                yp = np.where(low > inner, low, inner)
                dy2.append(float(np.sum((yp - y) * (yp - y))))
            k.v["AVG_Y"] = yp
            k.y[cur ^ 1] = hr.combine(k.h["k"], yp, y, k.v["LAST_RESTART_Y"])
            yps.append(yp)
        ywhole = np.concatenate(yps)  # (the gathered dual: every row block from its owner)
        sums = []
        for k, xp in zip(self.ranks, trial):  # the column block: complete column sums on the owner, the combination on sliced anchors
            cur, a, b = k.c["cur"], k.c0, k.c0 + k.nc
            seg = slice(k.t0, k.t1)
            col = _segment_sums(P["A_VALUES"][S.order[seg]] * ywhole[S.t_rows[seg]], S.t_off[a:b + 1] - k.t0, np.zeros(k.nc))
            x, aty = k.x[cur][a:b], k.aty[cur][a:b]
            dx = xp - x
            with np.errstate(invalid="ignore", over="ignore"):
                sums.append((dy2[k.rank], float(np.sum((col - aty) * dx)), float(np.sum(dx * dx))))
            xn, atyn = np.full(self.n, np.nan), np.full(self.n, np.nan)
            xn[a:b] = hr.combine(k.h["k"], xp, x, k.v["LAST_RESTART_X"][a:b])
            atyn[a:b] = hr.combine(k.h["k"], col, aty, k.v["LAST_RESTART_ATY"][a:b])
            k.x[cur ^ 1], k.aty[cur ^ 1] = xn, atyn
            if last:
                k.xp = xp
            k.v["PART_A"], k.v["PART_AT"] = np.array([sums[-1][0]]), np.array([sums[-1][1], sums[-1][2]])
        with np.errstate(invalid="ignore", over="ignore"):
            d2, it, x2 = (self._rank_order([s[i] for s in sums]) for i in range(3))  # ONE all-reduce of the three packed sums
        for k in self.ranks:  # the same decision on every rank (halpern_decision_from_sums)
            c, h = k.c, k.h
            r2 = hr.r2_of(c, d2, it, x2)
            c.update(last_interaction=it, last_movement=r2, last_dx2=x2, last_dy2=d2, attempts=c["attempts"] + 1)
            if r2 != r2 or not r2 < hr.OVERFLOW:
                c["error"] = 1
            else:
                r = float(np.sqrt(max(r2, 0.0)))
                h.update(r=r, r2=r2, r_first=(r if h["k"] == 0 else h["r_first"]), r2_min=min(h["r2_min"], r2), k=h["k"] + 1)
            c.update(k=c["k"] + 1, cur=c["cur"] ^ 1, steps_taken=c["steps_taken"] + 1, its_since_restart=c["its_since_restart"] + 1)

    def _epilogue(self):
        """run_epilogue in Halpern mode: X and ATY of the current side and x' of the run's last step all-gathered from their owners"""
        cur = self.ranks[0].c["cur"]
        wx, wa, wp = (np.full(self.n, np.nan) for _ in range(3))
        for k in self.ranks:
            a, b = k.c0, k.c0 + k.nc
            wx[a:b], wa[a:b] = k.x[cur][a:b], k.aty[cur][a:b]
            if k.xp is not None:
                wp[a:b] = k.xp
        for k in self.ranks:
            k.x[cur], k.aty[cur] = wx.copy(), wa.copy()
            if k.xp is not None:
                k.v["AVG_X"] = wp.copy()
            k.xp = None

    def _run(self, target):
        for k in self.ranks:
            k.c["target_steps"] = target
        rounds = 0
        while self.ranks[0].c["error"] == 0 and self.ranks[0].c["steps_taken"] < target:
            self._one_step(self.ranks[0].c["steps_taken"] + 1 >= target)
            rounds += 1
        if rounds:
            self._epilogue()
        return [dict(k.c) for k in self.ranks]

    def _halpern_restart(self, theta):
        primal, dual = [], []
        for k in self.ranks:
            cur, v = k.c["cur"], k.v
            dxv, dyv = v["LAST_RESTART_X"] - k.x[cur], v["LAST_RESTART_Y"] - k.y[cur]
            primal.append(float(np.sum(dxv * dxv)))  # (replicated: every rank over all columns)
            dual.append(float(np.sum(dyv * dyv)))
            v["LAST_RESTART_X"], v["LAST_RESTART_Y"], v["LAST_RESTART_ATY"] = k.x[cur].copy(), k.y[cur].copy(), k.aty[cur].copy()
        total = self._rank_order(dual)  # (the dual side is sharded: one sum over the ranks, before the weight is formed)
        out = []
        for k, p2 in zip(self.ranks, primal):
            dx, dy, c = float(np.sqrt(p2)), float(np.sqrt(total)), k.c
            if theta >= 0.0 and dx > 1.0e-10 and dy > 1.0e-10:
                w = float(np.exp(theta * np.log(dy / dx) + (1.0 - theta) * np.log(c["primal_weight"])))
                c.update(primal_weight=w, tau=c["step_size"] / w, sigma=c["step_size"] * w)
            c["its_since_restart"] = 0
            k.h["k"] = 0
            out.append(np.array([dx, dy]))
        return out


def stand_in(p, x0, y0, dr, dc, world):
    """halpern_step_scenario.stand_in's set-up on W stand-in ranks -> (HalpernAssembled, Structure, the scaled problem)"""
    import scipy.sparse as sp
    from cuopt_amd import capi
    S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
    prob = dict(A_VALUES=np.asarray(p["values"], float) * dr[S.rows] * dc[S.idx], C=p["c"] * dc, LB=p["lb"] / dc, UB=p["ub"] / dc, LO=p["lo"] * dr,
                HI=p["hi"] * dr)
    sigma = H.power_iteration(sp.csr_matrix((prob["A_VALUES"], S.idx, S.off), shape=(S.m, S.n)))[0]
    eta = H.STEP_SAFETY / sigma if sigma > 0 else 1.0
    x = np.asarray(x0, float) / dc
    x = np.minimum(np.maximum(x, prob["LB"]), prob["UB"])
    ranks = HalpernStandInRanks(S, prob, x, np.asarray(y0, float) / dr, dr, dc, world, capi.partition_rows(p["m"], p["offsets"], world), sigma)
    dev = HalpernAssembled(ranks, None)
    dev.set_step(eta, H.initial_weight(prob["C"], prob["LO"], prob["HI"]))
    dev.compute_aty()
    dev.halpern_restart(-1.0)
    return dev, S, prob
