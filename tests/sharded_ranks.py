"""TEST UTILITY: W ranks of a row-block sharded context behind the interface tests/attempt_scenario.py documents in its first lines, so
that the scenario and tests/attempt_reference.py check the sharded attempt on the GLOBAL LP, unchanged.

Assembled is the interface.  It talks to a backend that holds the ranks and answers each(op, *args) with one result per rank:
    DeviceRanks    one worker thread per rank, each with its own capi.Solver(p, rank=, world=, comm_id=softcomm_id(W)) on ONE device behind
                   the in-process communicator (tests/test_sharded_attempts_gpu.py);
    StandInRanks   W float64 stand-in ranks on the host, partial sums added in rank order, everything a rank does not own filled with
                   NaN (tests/test_attempt_reference.py: the assembly, the LPs and the scenario's conditions are proven without a GPU).

What Assembled assembles, and what it asserts on the way:
    ctl()          rank 0's control block; all 17 fields are the same on every rank
    get(m-sized)   the ranks' row blocks side by side (A_VALUES: their nonzeros)
    get(n-sized)   rank 0's vector, and every rank holds rank 0's bits -- except X_OTHER, ATY_OTHER and XBAR under the sliced dataflows
                   (rsag, owner): the trial side of a rejected attempt and xbar are valid on the owner's slice only (under the halo
                   exchange xbar elsewhere only on the ranges a rank's rows reference), so they are taken slice by slice from their
                   owners and not compared across ranks
    put("Y", a)    every rank its rows; an n-sized buffer whole to every rank
    restart        the two squared distances are the same on every rank
    eval_infeasibility, trust_region_bounds   the four / six figures are the same bits on every rank (tests/test_restart_inputs_gpu.py)
A snapshot of the scenario asks for nine buffers: the first of them fetches all nine and the control block from every rank in ONE
command, the rest is served from that until the next command that changes something.

A command goes to all ranks and returns when all have answered.  A rank that raises, or that has not answered within the command's time
limit, ends the test: the communicator is aborted (pdlpdev_comm_abort wakes the ranks waiting in a barrier), the threads are joined and
the rank's message is the assertion's.  Nothing is retried and no further command is issued.  A rank that did not answer, a HIP error
(-2) and a wait of the peer transport that ran out of patience (-6) are a hang or a fault of the device: they end the whole pytest
session, so that nothing more is started on a GPU that may be in a bad state."""
import ctypes as C
import queue
import threading
import time

import numpy as np

import attempt_reference as ar
from eval_reference import _segment_sums

INF = np.inf
M_SIZED = ("Y", "Y_OTHER", "SUM_Y", "AVG_Y", "LO", "HI", "DROW", "LAST_RESTART_Y", "AX_U_CURRENT", "AX_U_AVERAGE", "AX_U_LAST_RESTART")
SLICE_ONLY = ("X_OTHER", "ATY_OTHER", "XBAR")   # sliced dataflows: valid on the owner's slice only
SNAPSHOT = ar.STATE + ("XBAR",)                 # fetched together, once per rank
FLOWS = {"allreduce": 1, "rsag": 2, "owner": 3}  # pdlpdev_shard_dataflow
COMMAND_SECONDS = 120.0


def slices_of(n, world, flow):
    """[(first column, columns)] per rank: setup_dataflow's slice = ceil(n / world) rounded up to 16; (0, n) under the replicated dataflow"""
    if flow == "allreduce":
        return [(0, n)] * world
    per = (n + world - 1) // world
    width = (per + 15) & ~15
    return [(min(r * width, n), max(0, min(width, n - r * width))) for r in range(world)]


class Assembled:
    def __init__(self, backend, sp):
        self.b, self.sp = backend, sp
        self.world, self.flow, self.n = backend.world, backend.flow, backend.n
        self.bounds, self.slices = list(backend.bounds), list(backend.slices)
        assert self.slices == slices_of(self.n, self.world, self.flow), (self.slices, "the ranks' slices against setup_dataflow's formula")
        self._cache = {}

    # ---- what changes nothing ----
    def _fetch(self, name):
        if name not in self._cache:
            names = SNAPSHOT if name in SNAPSHOT or name == "ctl" else (name,)
            per_rank = self.b.each("get_many", names)
            for k in tuple(names) + ("ctl",):
                self._cache[k] = [d[k] for d in per_rank]
        return self._cache[name]

    def ctl(self):
        cs = self._fetch("ctl")
        for r, c in enumerate(cs):
            assert set(c) == set(ar.CTL_FIELDS) and c == cs[0], ("the control block of rank %d differs from rank 0's" % r, c, cs[0])
        return dict(cs[0])

    def get(self, name):
        per = self._fetch(name)
        if name == "A_VALUES" or name in M_SIZED:
            if name in M_SIZED:
                for r, a in enumerate(per):
                    assert len(a) == self.bounds[r + 1] - self.bounds[r], (name, r, len(a))
            return np.concatenate(per)
        assert all(len(a) == self.n for a in per), (name, [len(a) for a in per])
        if self.flow == "allreduce" or name not in SLICE_ONLY:
            for r, a in enumerate(per):
                assert ar.bits_equal(a, per[0]), ("%s: rank %d does not hold rank 0's bits" % (name, r), int(np.argmax(a.view(np.int64) != per[0].view(np.int64))))
            return per[0].copy()
        out = np.full(self.n, np.nan)
        for (c0, nc), a in zip(self.slices, per):
            out[c0:c0 + nc] = a[c0:c0 + nc]
        return out

    def download(self, name, count):  # (capi.Device's name for it: test_eval_layouts_gpu._check_vectors)
        a = self.get(name)
        assert len(a) == count, (name, len(a), count)
        return a

    # ---- what does ----
    def _do(self, op, *args, **kw):
        self._cache.clear()
        return self.b.each(op, *args, **kw)

    def put(self, name, a):
        self._do("put", name, np.ascontiguousarray(a, dtype=np.float64))

    def attempt(self):
        self.attempts(1)

    def attempts(self, count):
        self._do("attempts", int(count))

    def run(self, target):
        self._do("run", int(target))

    def flush(self):
        self._do("flush")

    def make_average(self, mode):
        self._do("make_average", int(mode))

    def restart(self, which, unscaled):
        dist = self._do("restart", int(which), int(unscaled))
        for r, d in enumerate(dist):
            assert ar.bits_equal(d, dist[0]), ("restart: rank %d returns other distances than rank 0" % r, list(d), list(dist[0]))
        return np.array(dist[0])

    def set_step(self, step, weight):
        self._do("set_step", float(step), float(weight))

    def compute_aty(self):
        self._do("compute_aty")

    def eval(self, which, rule_finite, eps):
        """pdlpdev_eval on every rank -> the eight scalars, identical on all ranks"""
        evs = self._do("eval", int(which), bool(rule_finite), float(eps))
        for r, e in enumerate(evs):
            assert e == evs[0], ("eval: rank %d returns other scalars than rank 0" % r, e, evs[0])
        return evs[0]

    def eval_infeasibility(self, which, rule_finite=True):
        out = self._do("eval_infeasibility", int(which), bool(rule_finite))
        for r, e in enumerate(out):
            assert e == out[0] and all(bits_of(e[k]) == bits_of(out[0][k]) for k in e), ("eval_infeasibility: rank %d against rank 0" % r, e, out[0])
        return out[0]

    def trust_region_bounds(self, which, *args, **kw):
        """pdlpdev_trust_region_bounds on every rank -> the six figures, the same bits on all ranks"""
        out = self._do("trust_region_bounds", int(which), args, kw)
        for r, e in enumerate(out):
            assert all(bits_of(e[k]) == bits_of(out[0][k]) for k in out[0]), ("trust_region_bounds: rank %d against rank 0" % r, e, out[0])
        return out[0]

    def close(self):
        self.b.close()


def bits_of(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


# ---- W worker threads, each with one rank's solver ---------------------------------------------------------------------------------------
class RankOnDevice:
    """one rank: the solver's constructor does the sharded set-up (scaling, owner_setup, p2p_setup); then the state
    test_attempt_layouts_gpu.prepared creates"""

    def __init__(self, p, x0, y0, sp, rank, world, cid, solver_kw):
        from cuopt_amd import capi
        self.capi = capi
        self.solver = capi.Solver(p, rank=rank, world=world, comm_id=cid, **solver_kw)
        self.dev = d = self.solver.device
        self.r0, self.r1 = self.solver.row_range()
        self.n, self.ml = int(p["n"]), self.r1 - self.r0
        self.nnz = int(p["offsets"][self.r1]) - int(p["offsets"][self.r0])
        d.call("set_step_params", C.byref(capi.StepParams(**sp)))
        d.call("set_initial", capi._ptr(np.ascontiguousarray(x0, dtype=np.float64)), capi._ptr(np.ascontiguousarray(y0[self.r0:self.r1], dtype=np.float64)))
        d.call("project_primal")
        d.call("set_step", 1.0 / d.init_norms()[0], 1.0)
        d.call("compute_aty")

    def info(self):
        d, flow = self.dev, self.capi.lib.pdlpdev_shard_dataflow(self.dev.handle)
        return dict(rows=(self.r0, self.r1), slice=d.shard_slice(), dataflow=flow, layout=d.layout(), owner_layout=d.owner_layout() if flow == 3 else None,
                    wire=d.wire_bytes(), p2p=bool(self.capi.lib.pdlpdev_shard_transport(d.handle)), dense=d.dense_info())

    def _count(self, name):
        return self.nnz if name == "A_VALUES" else self.ml if name in M_SIZED else self.n

    def get_many(self, names):
        out = {k: self.dev.download(k, self._count(k)) for k in names}
        out["ctl"] = ar.ctl_dict(self.dev.ctl())
        return out

    def put(self, name, a):
        self.dev.upload(name, a[self.r0:self.r1] if name in M_SIZED else a)

    def attempts(self, count):
        self.dev.attempts(count)

    def run(self, target):
        self.dev.run(target)

    def flush(self):
        self.dev.call("flush_average")

    def make_average(self, mode):
        self.dev.call("make_average", mode)

    def restart(self, which, unscaled):
        dist = np.zeros(2)
        self.dev.call("restart", which, unscaled, self.capi._ptr(dist))
        return dist

    def set_step(self, step, weight):
        self.dev.call("set_step", step, weight)

    def compute_aty(self):
        self.dev.call("compute_aty")

    def eval(self, which, rule_finite, eps):
        return {k: float(v) for k, v in self.dev.eval(which, rule_finite=rule_finite, eps_p=eps, eps_d=eps).items()}

    def eval_infeasibility(self, which, rule_finite):
        return self.dev.eval_infeasibility(which, rule_finite=rule_finite)

    def trust_region_bounds(self, which, args, kw):
        return self.dev.trust_region_bounds(which, *args, **kw)

    def close(self):
        self.solver.close()


class DeviceRanks:
    def __init__(self, p, x0, y0, sp, world, flow, **solver_kw):
        from cuopt_amd import capi
        self.capi, self.world, self.flow, self.n = capi, world, flow, int(p["n"])
        self.cid = capi.softcomm_id(world)
        self.dead, self.answers = None, queue.Queue()
        self.inbox = [queue.Queue() for _ in range(world)]
        self.threads = [threading.Thread(target=self._worker, args=(r, p, x0, y0, sp, solver_kw), daemon=True) for r in range(world)]
        for t in self.threads:
            t.start()
        self._collect("set-up", COMMAND_SECONDS)
        try:
            self.info = self.each("info")
            self.bounds = [self.info[0]["rows"][0]] + [i["rows"][1] for i in self.info]
            self.slices = [i["slice"] for i in self.info]
            assert all(i["dataflow"] == FLOWS[flow] for i in self.info), (flow, [i["dataflow"] for i in self.info])
            assert self.bounds == capi.partition_rows(p["m"], p["offsets"], world).tolist(), self.bounds
        except BaseException:
            self.close()
            raise

    def _worker(self, rank, p, x0, y0, sp, solver_kw):
        try:
            rk = RankOnDevice(p, x0, y0, sp, rank, self.world, self.cid, solver_kw)
            self.answers.put((rank, True, None))
        except BaseException as e:  # (told to the main thread, which fails the test)
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

    def _collect(self, what, seconds):
        out, left, deadline = [None] * self.world, self.world, time.monotonic() + seconds
        while left:
            try:
                rank, ok, value = self.answers.get(timeout=max(0.0, deadline - time.monotonic()))
            except queue.Empty:
                self._fail("%s: %d rank(s) did not answer within %g s" % (what, left, seconds), fatal=True)
            if not ok:
                self._fail("rank %d, %s" % (rank, value[0]), fatal=value[1] in (-2, -6))
            out[rank], left = value, left - 1
        return out

    def _fail(self, message, fatal=False):
        self.dead = message
        self.capi.comm_abort(self.cid)  # (the ranks waiting for the failed one leave their barriers with an error)
        self.close()
        if fatal:
            import pytest
            pytest.exit("sharded ranks: " + message, returncode=3)
        raise AssertionError(message)

    def each(self, op, *args, seconds=COMMAND_SECONDS):
        assert self.dead is None, ("no command behind a failed one", self.dead)
        for q in self.inbox:
            q.put((op, args))
        return self._collect(op, seconds)

    def close(self):
        for q in self.inbox:
            q.put(None)
        for t in self.threads:
            t.join(timeout=30.0)
        self.threads = []


def on_device(p, x0, y0, sp, world, flow, **solver_kw):
    """-> Assembled over W device ranks, prepared; CUOPT_AMD_SHARD_DATAFLOW (and whatever else the ranks' set-up reads) is the caller's"""
    ranks = DeviceRanks(p, x0, y0, sp, world, flow, **solver_kw)
    try:
        return Assembled(ranks, sp)
    except BaseException:
        ranks.close()
        raise


# ---- W float64 stand-in ranks on the host ------------------------------------------------------------------------------------------------
class _HostRank:
    pass


class StandInRanks:
    """attempt_scenario.HostStandIn split into W ranks as cuopt_amd/csrc/pdlp_device.hip enqueue_attempt shards the attempt: row blocks
    by capi.partition_rows, slices by setup_dataflow's formula, partial products and sums added in rank order, and a rank's copy of
    whatever it does not own at that point of the dataflow overwritten with NaN -- a stale entry that the assembly (or the stand-in
    itself) read would poison everything behind it.  float64, numpy's own order inside a rank.  It is no second reference."""

    def __init__(self, S, prob, sp, x, y, dr, dc, world, flow, bounds):
        self.S, self.prob, self.sp, self.world, self.flow, self.n = S, prob, sp, world, flow, S.n
        self.bounds, self.slices, self.dr, self.dc = [int(b) for b in bounds], slices_of(S.n, world, flow), dr, dc
        assert self.bounds[0] == 0 and self.bounds[-1] == S.m and all(a < b for a, b in zip(self.bounds[:-1], self.bounds[1:])), self.bounds
        self.ranks = []
        for r in range(world):
            k, r0, r1 = _HostRank(), self.bounds[r], self.bounds[r + 1]
            k.rank = r
            k0, k1 = int(S.off[r0]), int(S.off[r1])
            k.r0, k.r1, k.c0, k.nc = r0, r1, *self.slices[r]
            k.off, k.idx, k.val = S.off[r0:r1 + 1] - k0, S.idx[k0:k1], prob["A_VALUES"][k0:k1]
            k.T = ar.Structure(r1 - r0, S.n, k.off, k.idx)  # (this row block's transpose: the partial A^T product)
            k.c = dict(step_size=0.0, primal_weight=1.0, tau=0.0, sigma=0.0, sum_weights=0.0, last_interaction=0.0, last_movement=0.0, last_dx2=0.0,
                       last_dy2=0.0, k=0, cur=0, pending_avg=0, steps_taken=0, attempts=0, target_steps=0, error=0, its_since_restart=0)
            k.x, k.aty = [np.array(x, float), np.zeros(S.n)], [np.zeros(S.n), np.zeros(S.n)]
            k.y = [np.array(y[r0:r1], float), np.zeros(r1 - r0)]
            k.v = dict(XBAR=np.zeros(S.n), SUM_X=np.zeros(S.n), AVG_X=np.zeros(S.n), LAST_RESTART_X=np.zeros(S.n), SUM_Y=np.zeros(r1 - r0),
                       AVG_Y=np.zeros(r1 - r0), LAST_RESTART_Y=np.zeros(r1 - r0))
            # the owner's columns over ALL rows, rows ascending (pdlpdev_owner_setup): positions in the global transposition
            k.t0, k.t1 = int(S.t_off[k.c0]), int(S.t_off[k.c0 + k.nc])
            self.ranks.append(k)

    def each(self, op, *args):
        return getattr(self, "_" + op)(*args)

    def close(self):
        pass

    # ---- per rank ----
    def _get_many(self, names):
        out = []
        for k in self.ranks:
            cur, d = k.c["cur"], {}
            pairs = dict(X=k.x, Y=k.y, ATY=k.aty)
            for name in names:
                if name in pairs:
                    d[name] = pairs[name][cur].copy()
                elif name.endswith("_OTHER"):
                    d[name] = pairs[name[:-6]][cur ^ 1].copy()
                elif name == "A_VALUES":
                    d[name] = k.val.copy()
                elif name in ("LO", "HI"):
                    d[name] = self.prob[name][k.r0:k.r1].copy()
                elif name == "DROW":
                    d[name] = self.dr[k.r0:k.r1].copy()
                elif name == "DCOL":
                    d[name] = self.dc.copy()
                else:
                    d[name] = (self.prob[name] if name in self.prob else k.v[name]).copy()
            d["ctl"] = dict(k.c)
            out.append(d)
        return out

    def _put(self, name, a):
        for k in self.ranks:
            {"X": k.x, "Y": k.y, "ATY": k.aty}[name][k.c["cur"]] = np.array(a[k.r0:k.r1] if name in M_SIZED else a, float)
        return [None] * self.world

    def _set_step(self, step, weight):
        for k in self.ranks:
            if step >= 0.0:
                k.c["step_size"] = step
            k.c.update(primal_weight=weight, tau=k.c["step_size"] / weight, sigma=k.c["step_size"] * weight)
        return [None] * self.world

    @staticmethod
    def _rank_order(parts):
        total = parts[0].copy() if isinstance(parts[0], np.ndarray) else parts[0]
        for q in parts[1:]:
            total = total + q
        return total

    def _partial_at(self, k, y):
        return _segment_sums(k.val[k.T.order] * y[k.T.t_rows], k.T.t_off, np.zeros(self.n))

    def _compute_aty(self):
        total = self._rank_order([self._partial_at(k, k.y[k.c["cur"]]) for k in self.ranks])  # (one all-reduce: replicated)
        for k in self.ranks:
            k.aty[k.c["cur"]] = total.copy()
        return [None] * self.world

    def _outside(self, k, a):
        """the rank's slice of `a`, NaN everywhere else (sliced dataflows)"""
        out = np.full(self.n, np.nan)
        out[k.c0:k.c0 + k.nc] = a[k.c0:k.c0 + k.nc]
        return out

    def _one_attempt(self):
        P, S, sliced = self.prob, self.S, self.flow != "allreduce"
        c0 = self.ranks[0].c
        if c0["error"] or c0["steps_taken"] >= c0["target_steps"]:
            return
        trial = []
        for k in self.ranks:  # k_primal: on the slice (all columns under the replicated dataflow)
            c, cur = k.c, k.c["cur"]
            a, b = (k.c0, k.c0 + k.nc) if sliced else (0, self.n)
            x, aty = k.x[cur][a:b], k.aty[cur][a:b]
            nxt = x - c["tau"] * (P["C"][a:b] - aty)
            nxt = np.where(nxt < P["UB"][a:b], nxt, P["UB"][a:b])
            nxt = np.where(nxt > P["LB"][a:b], nxt, P["LB"][a:b])
            xn, xbar = np.full(self.n, np.nan), np.full(self.n, np.nan)
            xn[a:b], xbar[a:b] = nxt, nxt - x + nxt
            if c["pending_avg"]:
                s = k.v["SUM_X"][a:b] + c["step_size"] * x
                k.v["SUM_X"] = np.full(self.n, np.nan)  # (the other slices' sums are their owners' until the hook's epilogue)
                k.v["SUM_X"][a:b] = s
            trial.append(xn)
            k.v["XBAR"] = xbar
        if sliced:  # all-gather of xbar (the halo exchange brings the same values where a rank's rows look)
            whole = np.full(self.n, np.nan)
            for k in self.ranks:
                whole[k.c0:k.c0 + k.nc] = k.v["XBAR"][k.c0:k.c0 + k.nc]
            assert np.isfinite(whole).all()
        ynew, dy2 = [], []
        for k in self.ranks:  # the A product with DualEpilogue on the rank's rows
            c, cur = k.c, k.c["cur"]
            xbar = whole if sliced else k.v["XBAR"]
            y = k.y[cur]
            ax = _segment_sums(k.val * xbar[k.idx], k.off, np.zeros(k.r1 - k.r0))
            ny = y - c["sigma"] * ax
            with np.errstate(invalid="ignore"):
                low, up = ny + c["sigma"] * P["LO"][k.r0:k.r1], ny + c["sigma"] * P["HI"][k.r0:k.r1]
            inner = np.where(up < 0.0, up, 0.0)
            ny = np.where(low > inner, low, inner)
            if c["pending_avg"]:
                k.v["SUM_Y"] = k.v["SUM_Y"] + c["step_size"] * y
            ynew.append(ny)
            dy2.append(float(np.sum((ny - y) * (ny - y))))
        sums = []  # per rank (dy2, interaction, dx2) as the decision gets them
        if self.flow == "owner":  # complete column sums on the owner, from the gathered y'
            ywhole = np.concatenate(ynew)
            for k, xn in zip(self.ranks, trial):
                cur, a, b = k.c["cur"], k.c0, k.c0 + k.nc
                seg = slice(k.t0, k.t1)
                col = _segment_sums(P["A_VALUES"][S.order[seg]] * ywhole[S.t_rows[seg]], S.t_off[a:b + 1] - k.t0, np.zeros(k.nc))
                naty = np.full(self.n, np.nan)
                naty[a:b] = col
                dx = xn[a:b] - k.x[cur][a:b]
                sums.append((dy2[k.rank], float(np.sum((col - k.aty[cur][a:b]) * dx)), float(np.sum(dx * dx)), naty))
        else:
            partial = [self._partial_at(k, ny) for k, ny in zip(self.ranks, ynew)]
            for r, (k, xn) in enumerate(zip(self.ranks, trial)):
                cur = k.c["cur"]
                a, b = (k.c0, k.c0 + k.nc) if sliced else (0, self.n)
                col = self._rank_order([q[a:b] for q in partial])  # (reduce-scatter / all-reduce: the ranks' partials in rank order)
                naty = np.full(self.n, np.nan)
                naty[a:b] = col
                dx = xn[a:b] - k.x[cur][a:b]
                sums.append((dy2[r], float(np.sum((col - k.aty[cur][a:b]) * dx)), float(np.sum(dx * dx)), naty))
        if sliced:  # ONE all-reduce of the three packed sums
            three = [self._rank_order([s[i] for s in sums]) for i in range(3)]
        else:       # dy2 travelled with the partial products; interaction and dx2 are each rank's own, over all columns
            three = None
            total_dy2 = self._rank_order([s[0] for s in sums])
        for r, (k, xn, ny) in enumerate(zip(self.ranks, trial, ynew)):
            cur = k.c["cur"]
            d2, it, x2 = three if sliced else (total_dy2, sums[r][1], sums[r][2])
            k.c = ar.decision(k.c, d2, it, x2, self.sp)["ctl"]
            k.x[cur ^ 1], k.y[cur ^ 1], k.aty[cur ^ 1] = xn, ny, sums[r][3]

    def _epilogue(self):
        """run_epilogue: X, ATY and SUM_X of the current side all-gathered from their owners (sliced dataflows)"""
        if self.flow == "allreduce":
            return
        cur = self.ranks[0].c["cur"]
        for pick, store in ((lambda k: k.x[cur], lambda k, a: k.x.__setitem__(cur, a)), (lambda k: k.aty[cur], lambda k, a: k.aty.__setitem__(cur, a)),
                            (lambda k: k.v["SUM_X"], lambda k, a: k.v.__setitem__("SUM_X", a))):
            whole = np.full(self.n, np.nan)
            for k in self.ranks:
                whole[k.c0:k.c0 + k.nc] = pick(k)[k.c0:k.c0 + k.nc]
            for k in self.ranks:
                store(k, whole.copy())

    def _attempts(self, count):
        for k in self.ranks:
            k.c["target_steps"] = k.c["steps_taken"] + count
        if not self.ranks[0].c["error"]:
            for _ in range(count):
                self._one_attempt()
            self._epilogue()
        return [None] * self.world

    def _run(self, target):
        for k in self.ranks:
            k.c["target_steps"] = target
        rounds = 0
        while self.ranks[0].c["error"] == 0 and self.ranks[0].c["steps_taken"] < target:
            self._one_attempt()
            rounds += 1
        if rounds:
            self._epilogue()
        return [None] * self.world

    def _flush(self):
        for k in self.ranks:
            c, cur = k.c, k.c["cur"]
            if c["pending_avg"]:
                k.v["SUM_X"], k.v["SUM_Y"] = k.v["SUM_X"] + c["step_size"] * k.x[cur], k.v["SUM_Y"] + c["step_size"] * k.y[cur]
            c["pending_avg"] = 0
        return [None] * self.world

    def _make_average(self, mode):
        for k in self.ranks:
            cur, v = k.c["cur"], k.v
            if mode == 0:
                v["AVG_X"], v["AVG_Y"] = k.x[cur].copy(), k.y[cur].copy()
            elif mode == 1:
                v["AVG_X"], v["AVG_Y"] = np.zeros(self.n), np.zeros(k.r1 - k.r0)
            else:
                v["AVG_X"], v["AVG_Y"] = v["SUM_X"] / k.c["sum_weights"], v["SUM_Y"] / k.c["sum_weights"]
        return [None] * self.world

    def _restart(self, which, unscaled):
        primal, dual = [], []
        for k in self.ranks:
            cur, v = k.c["cur"], k.v
            for pair, avg, anchor, d, out in ((k.x, "AVG_X", "LAST_RESTART_X", self.dc, primal), (k.y, "AVG_Y", "LAST_RESTART_Y", self.dr[k.r0:k.r1], dual)):
                cand = v[avg].copy() if which == ar.AVERAGE else pair[cur].copy()
                diff = v[anchor] - cand
                if unscaled:
                    diff = diff * d
                out.append(float(np.sum(diff * diff)))
                pair[cur], v[anchor] = cand, cand.copy()
            v["SUM_X"], v["SUM_Y"] = np.zeros(self.n), np.zeros(k.r1 - k.r0)
            k.c.update(sum_weights=0.0, its_since_restart=0, pending_avg=0)
        total = self._rank_order(dual)  # (the dual side is sharded: one sum over the ranks)
        return [np.array([p, total]) for p in primal]


def stand_in(p, x0, y0, dr, dc, sp, world, flow):
    """attempt_scenario.stand_in's step 1 on W stand-in ranks -> (Assembled, Structure, the scaled problem)"""
    from cuopt_amd import capi
    S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
    prob = dict(A_VALUES=np.asarray(p["values"], float) * dr[S.rows] * dc[S.idx], C=p["c"] * dc, LB=p["lb"] / dc, UB=p["ub"] / dc, LO=p["lo"] * dr,
                HI=p["hi"] * dr)
    x = np.asarray(x0, float) / dc
    x = np.minimum(np.maximum(x, prob["LB"]), prob["UB"])
    ranks = StandInRanks(S, prob, sp, x, np.asarray(y0, float) / dr, dr, dc, world, flow, capi.partition_rows(p["m"], p["offsets"], world))
    dev = Assembled(ranks, sp)
    dev.set_step(1.0 / np.abs(prob["A_VALUES"]).max(), 1.0)
    dev.compute_aty()
    return dev, S, prob


# ---- the band LP of the transport and halo cases -----------------------------------------------------------------------------------------
BAND_START = (32768, 200)  # where the search for the band LP starts
BAND_LP = (4096, 200)      # ... and where it ends at world 4 (smallest_band; tests/test_attempt_reference.py holds the two together)


def halo_rule(p, world):
    """pdlpdev_owner_setup's and halo_setup's decision, restated on the host: per peer ONE range of xbar (the columns of that peer's
    slice this rank's rows reference) and one of the gathered y' (the positions of that peer's rows this rank's columns reference); the
    halo exchange is taken when the largest volume a rank receives, times 4, is at most the two all-gathers' -> (use, worst, full)"""
    from cuopt_amd import capi
    m, n, off, idx = p["m"], p["n"], np.asarray(p["offsets"], np.int64), np.asarray(p["indices"], np.int64)
    bounds = capi.partition_rows(m, p["offsets"], world).astype(np.int64)
    width = ((n + world - 1) // world + 15) & ~15
    ypad = (int(np.diff(bounds).max()) + 15) & ~15
    rows = np.repeat(np.arange(m), np.diff(off))
    row_rank, col_rank = np.searchsorted(bounds, rows, side="right") - 1, idx // width
    pos = rows + row_rank * ypad - bounds[row_rank]
    worst = 0
    for r in range(world):
        volume = 0
        for q in range(world):
            if q == r:
                continue
            cols = idx[(row_rank == r) & (col_rank == q)]   # rank r's rows looking into rank q's slice
            spots = pos[(col_rank == r) & (row_rank == q)]  # rank r's columns looking at rank q's rows
            volume += (int(cols.max()) + 1 - int(cols.min()) if len(cols) else 0) + (int(spots.max()) + 1 - int(spots.min()) if len(spots) else 0)
        worst = max(worst, volume)
    full = (world - 1) * (width + ypad)
    return worst * 4 <= full, worst, full


def band_lp(m, band, seed=8):
    """the pattern and values of synthetic.generate(m, m, 10, seed=2, band=band) with the row and column kinds, the objective and the
    start of eval_lps.edge_lp (equality rows among them, which the scenario's forced rejection needs) -> (p, x0, y0)"""
    from cuopt_amd import synthetic
    g = synthetic.generate(m, m, 10, seed=2, band=band)
    rng = np.random.default_rng(seed)
    n = m
    p = dict(m=m, n=n, offsets=g["offsets"], indices=g["indices"], values=g["values"])
    row_kind, col_kind = rng.permutation(np.arange(m) % 5), rng.permutation(np.arange(n) % 5)
    b, w = rng.standard_normal(m), np.abs(rng.standard_normal(m)) + 0.5
    p["lo"] = np.choose(row_kind, [np.full(m, -INF), b - 1.0, b, np.full(m, -INF), b - 1.0])
    p["hi"] = np.choose(row_kind, [b + 3.0, np.full(m, INF), b, np.full(m, INF), b - 1.0 + w])
    p["lb"] = np.choose(col_kind, [-INF, -INF, 0.0, 1.5, 0.0]).astype(np.float64)
    p["ub"] = np.choose(col_kind, [INF, 5.0, INF, 1.5, 5.0]).astype(np.float64)
    p["c"] = rng.standard_normal(n)
    x = np.abs(rng.standard_normal(n)) * (rng.random(n) < 0.7)
    x[col_kind == 3] = 1.5
    return p, x, rng.standard_normal(m)


def smallest_band(world=4):
    """(m, band): from BAND_START, m halved while the halo rule still holds on the halved LP; the band is kept -- a narrower one only
    shortens the ranges, and at 200 a range (up to 2 x 200 entries) still spans more than one 256-thread block of the range copies"""
    m, band = BAND_START
    assert halo_rule(band_lp(m, band)[0], world)[0], "the halo rule does not hold where the search starts"
    while m >= 2 * 1024 and halo_rule(band_lp(m // 2, band)[0], world)[0]:
        m //= 2
    return m, band
