"""CPU: the edge LPs, the feature detector and the scenario of tests/test_batch_attempts_gpu.py (tests/batch_cases.py) on K float64
stand-ins behind the batch's interface: the LPs are what their generator promises, every feature is there under the two cutting rules
as batch_cases restates them, the scenario has the properties the GPU test relies on -- and three deliberately wrong stand-ins each
FAIL it, so the checks bite without a kernel being touched."""
import numpy as np
import pytest

import attempt_reference as ar
import batch_cases as bc
from test_attempt_reference import scaling_of, step_params


@pytest.fixture(scope="module")
def edge():
    p, x0, y0 = bc.edge_lp()
    return p, x0, y0, scaling_of(p)


def transposed(p):
    S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
    return S, S.t_off, S.t_rows


def test_the_edge_lp_is_what_its_generator_promises(edge):
    p = edge[0]
    m, n, off, idx = p["m"], p["n"], np.asarray(p["offsets"], np.int64), np.asarray(p["indices"], np.int64)
    assert (m, n, len(idx)) == (7244, 7200, 26520) and m % 512 and n % 512
    S, t_off, t_rows = transposed(p)
    for rows, o, ix in ((m, off, idx), (n, t_off, t_rows)):
        lens = np.diff(o)
        assert lens.max() == bc.MAX_ROW and (lens == 0).sum() > 512
        inside = np.ones(len(ix), bool)
        inside[o[:-1][lens > 0]] = False  # (the first entry of a row has no predecessor in it)
        step = np.diff(ix, prepend=-10)
        assert (step[inside] >= 2).all(), "columns ascending within a row, and no two adjacent: no run of consecutive columns"
    assert (np.bincount(idx, minlength=n) == 0).any() and (np.diff(off) == 0).any()
    heads, (u_q, u_p) = p["heads"], p["uniform"]
    assert (np.diff(off)[heads[0]:heads[0] + u_q] == bc.UNIFORM).all() and (np.diff(t_off)[heads[1]:heads[1] + u_p] == bc.UNIFORM).all()
    assert (u_q, u_p) == (420, 360) and pow(bc.STRIDE, -1, 360) == 131 and pow(bc.STRIDE, -1, 420) == 191


@pytest.mark.parametrize("K", [2, 4, 8, 16])
@pytest.mark.parametrize("layout", ["stream", "panel"])
def test_every_feature_is_there_under_the_restated_cuts(edge, layout, K):
    """(the GPU test asserts the same on the boundaries the batch itself reports)"""
    p = edge[0]
    S, t_off, t_rows = transposed(p)
    cuts = bc.stream_cuts if layout == "stream" else bc.panel_cuts
    for side, (o, ix, ncols) in enumerate(((S.off, S.idx, p["n"]), (t_off, t_rows, p["m"]))):
        row0 = cuts(o)
        missing = set(bc.FEATURES) - bc.features(o, row0, K, ix, ncols)
        assert not missing, (layout, K, "side %d" % side, sorted(missing))
        assert row0[-1] - row0[-2] == 1 and o[row0[-2]] == o[-1], "the last block: one row, no entries, off[r0] == nnz"


def test_the_detector_reports_only_what_is_there():
    off = np.array([0, 128, 256, 256, 384, 512, 600])  # K = 16: boundaries at 256 and 512
    f = bc.features(off, [0, 6], 16)
    assert {"row ends on a boundary", "row starts on a boundary", "empty row on a boundary", "nch=3", "nr<64", "empty row"} <= f
    assert not f & {"nch=1", "nch=2", "128-entry row across a boundary", "nr=1", "nr=512", "empty last block", "nch=0 in the middle", "CHUNK entries"}
    f = bc.features(np.array([0, 200, 328, 328]), [0, 2, 3], 16)
    assert {"128-entry row across a boundary", "nch=2", "nr=1", "empty last block"} <= f and "row ends on a boundary" not in f
    assert "128-entry row across a boundary" not in bc.features(np.array([0, 200, 328, 328]), [0, 2, 3], 8)  # (one chunk of 512: no boundary)
    assert "2*CHUNK entries" in bc.features(np.array([0, 100, 228, 256, 512]), [0, 4], 16, [0] * 512, 2) and "CHUNK entries" in bc.features([0, 512], [0, 1], 8)
    assert "empty column" in bc.features([0, 1], [0, 1], 2, [1], 2) and "empty column" not in bc.features([0, 2], [0, 1], 2, [0, 1], 2)


@pytest.mark.parametrize("uniform_parent", [True, False])
def test_the_members_are_feasible_and_differ_as_promised(edge, uniform_parent):
    p = edge[0]
    ms = bc.members(p, 16, uniform_parent)
    for lb, ub, lo, hi, how in ms:
        assert bc.feasible(p, lb, ub, lo, hi)
    uniform = [bool((lb == 0).all() and np.isinf(ub).all()) for lb, ub, *_ in ms]
    assert uniform[0] == uniform_parent and not uniform[1] and uniform[2] and ms[2][4] == "reset-back" and not any(uniform[3:])
    lo3, hi3 = ms[3][2:4]
    assert (lo3 != p["lo"]).any() and (lo3 == hi3).sum() > 100 and np.isinf(lo3).sum() > 100 and np.isinf(hi3).sum() > 100
    assert ((p["lo"] == p["hi"]) & np.isfinite(p["lo"])).sum() > 100


def test_the_banded_edge_lp(edge):
    p = bc.banded_edge_lp()[0]
    off, idx = np.asarray(p["offsets"], np.int64), np.asarray(p["indices"], np.int64)
    lens = np.diff(off)
    assert p["m"] % 512 and p["n"] % 512 and lens.max() <= 14 and (lens[700:790] == 0).all() and (lens[-37:] == 0).all()
    inside = np.ones(len(idx), bool)
    inside[off[:-1][lens > 0]] = False
    assert (np.diff(idx, prepend=-10)[inside] >= 2).all() and (np.bincount(idx, minlength=p["n"]) == 0).sum() >= 20
    assert bc.feasible(p, p["lb"], p["ub"], p["lo"], p["hi"])


# ---- the scenario on K stand-ins --------------------------------------------------------------------------------------------------------
def make(edge, K, member=bc.Member, batch=bc.BatchStandIn, uniform_parent=True):
    p, x0, y0, (dr, dc) = edge
    sp = step_params(1)
    devs, S, probs = bc.stand_in_members(p, x0, y0, dr, dc, sp, bc.members(p, K, uniform_parent), member)
    b = batch(devs, bc.stream_cuts(S.off), bc.stream_cuts(S.t_off))
    return b, devs, S, probs, sp


@pytest.mark.parametrize("K,uniform_parent", [(2, True), (4, True), (4, False)])
def test_scenario_on_the_stand_in_members(edge, K, uniform_parent):
    b, devs, S, probs, sp = make(edge, K, uniform_parent=uniform_parent)
    worst = bc.run_batch_scenario(b, devs, S, probs, sp, "stand-in K=%d" % K, refresh=lambda l: devs[l].prob)
    print(worst.line("stand-in-K%d-%s" % (K, "uniform" if uniform_parent else "nonuniform")))
    assert max(worst.values()) <= 1.0 and min(worst[k] for k in ("dy2", "dx2", "inter")) > 0.0, worst


class DropsABoundaryEntry(bc.Member):
    """row 12 of A starts on entry 1024 of its block of 512 rows, a chunk boundary at every K: its first product is left out"""

    def row_sums(self, xbar):
        out = super().row_sums(xbar)
        k0, k1 = int(self.S.off[12]), int(self.S.off[13])
        out[12] = ar.rowsums_f64(self.prob["A_VALUES"][k0 + 1:k1], xbar, [0, k1 - k0 - 1], self.S.idx[k0 + 1:k1])[0]
        return out


class SwapsTwoMembers(bc.BatchStandIn):
    def view(self, side):
        v = super().view(side)
        v["vK"][:, [0, 1]] = v["vK"][:, [1, 0]]
        return v


class MovesARestingSum(bc.BatchStandIn):
    def rest(self, l):
        super().rest(l)
        self.devs[l].v["SUM_X"][7] += 2.0 ** -30


def test_three_wrong_stand_ins_fail_the_scenario(edge):
    p = edge[0]
    assert p["offsets"][12] == 1024 and p["offsets"][13] == 1152  # (row 12 is PRE's last: on the boundary 1024)
    for kw, stage in ((dict(member=DropsABoundaryEntry), "y'"), (dict(batch=SwapsTwoMembers), "xbar|yK"), (dict(batch=MovesARestingSum), "resting member's buffer moved")):
        b, devs, S, probs, sp = make(edge, 4, **kw)
        with pytest.raises(AssertionError, match=stage):
            bc.run_batch_scenario(b, devs, S, probs, sp, "wrong stand-in", refresh=lambda l: devs[l].prob)


def test_the_jagged_detector_reports_only_what_is_there():
    off = np.concatenate([[0], np.cumsum([8] * 64 + [5] * 10 + [0])])
    assert bc.jag_features(off, [0, 75], 2, 8) == {"pass of fewer than 64 rows", "kmax not a multiple of U", "row without nonzeros"}
    assert bc.jag_features(off, [0, 64, 75], 2, 8) == {"pass of fewer than 64 rows", "kmax not a multiple of U", "row without nonzeros", "several blocks"}
    assert bc.jag_features(off, [0, 75], 16, 16) == {"pass of fewer than 64 rows", "row without nonzeros"} and bc.jag_unroll(16, 16) == 1
    assert bc.jag_features(off[:65], [0, 64], 2, 8) == set() and (bc.jag_unroll(2, 8), bc.jag_unroll(16, 8), bc.jag_unroll(2, 16)) == (8, 2, 8)
    assert "nr<64" not in bc.features([0, 0], [0, 1], 2) and "nr=1" in bc.features([0, 0], [0, 1], 2)
