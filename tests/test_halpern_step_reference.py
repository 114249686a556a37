"""CPU: the stage-by-stage restatement of one reflected-Halpern step and its restart (tests/halpern_step_reference.py) against
numbers worked out by hand, and the scenario of tests/test_halpern_step_layouts_gpu.py (tests/halpern_step_scenario.py) on a plain
float64 stand-in for the device, on the three LPs its 13 layout ids use: the stand-in stays inside every derived bound, and the
scenario has the properties the GPU test relies on -- every step moves both halves (dx2, dy2, r2 > 0), the interaction's bound is at
most 1e-10 of sum |t_j dx_j| (so the check is four orders sharper than a comparison at 1e-10 of a norm), empty rows and columns and
rows and columns with a workgroup of their own exist, and no row or column is left out of a comparison.  The last section hands
check_step stand-ins that are subtly WRONG in one place each and asserts that the failure names the stage.

The fixed point.  attempt_scenario.tiny_lp("fixed-point") (c = 0, y = 0, free rows) IS a fixed point of T under this mode's tau and
sigma -- under any: x' = proj(x - tau (0 - A^T 0)) = x and y' = max(-inf, min(+inf, 0)) = 0 = y -- so the GPU test's fixed-point case
uses it as it stands.  What keeps its BITS is the first step behind a restart only: there w = w0 = 1/2 and x/2 + x/2 is exact, while
from k = 1 on fl(fl(2/3) x) + fl(w0 x) may differ from x in its last bit.  Such an x is still inside the bounds, T still maps it to
itself, and r2 stays exactly 0: that is what is asserted for the second step."""
import fractions

import numpy as np
import pytest

import attempt_reference as ar
import attempt_scenario as asc
import eval_reference as er
import frame_reference as fr
import halpern_reference as H
import halpern_step_reference as hr
import halpern_step_scenario as sc
import resident_lps as rl
from eval_lps import DENSE_ROWS, EMPTY_COLS, LONG_COLS, LONG_ROWS, SEEDS, WIDE_N, edge_lp
from test_attempt_reference import arrays, ctl_of, scaling_of

INF = np.inf
LPS = [(4500, False, SEEDS[0]), (2400, True, SEEDS[1]), (2400, False, SEEDS[0], WIDE_N)]
LP_IDS = ["col4500", "dense-col2400", "col2400-60000-columns"]
INTER_BOUND_REL = 1e-10  # (a CPU run of the restatement measured 6.9e-12 at worst)
LONG_ROW, PANEL_OWN_ROW = 128, 4096  # kLongRow: beyond it the stream layout gives a row a workgroup; kPanelOwnRow: the panel layout does


# ---- by hand -----------------------------------------------------------------------------------------------------------------------------
def hand_case():
    """A = [1 2 0 0; 0 1 0 1; 0 0 0 0] (row 2 and column 2 empty), c = (-1, -2, 1, 0), x >= 0, x_1 <= 1; row 0: <= 1, row 1: = 2,
    row 2: >= -1.  Step 1/2 at weight 2 (tau = 1/4, sigma = 1), k = 2: w = 3/4, w0 = 1/4.  From x = (0, 0, 1, 0), y = (0, 0, 2),
    A^T y = 0, the anchor x0 = (4, 0, 0, 8), y0 = (4, -4, 0), A^T y0 = (4, 4, 0, -4), on side 1 of the ping-pong pairs.
       x' = (1/4, 1/2, 3/4, 0), xbar = (1/2, 1, 1/2, 0), A xbar = (5/2, 1, 0)
       row 0: next = -5/2, up = -3/2 < 0: y' = -3/2      row 1: next = -1, low = up = 1: y' = 1      row 2: next = 2, low = 1 > 0: y' = 1
       v = A^T y' = (-3/2, -2, 0, 1); dx = (1/4, 1/2, -1/4, 0), dy = (-3/2, 1, -1), t = v
       dx2 = 3/8, dy2 = 17/4, interaction = -3/8 - 1 = -11/8, r2 = 4 (3/8) + 2 (-11/8) + 17/4 = 3
       x^{k+1} = 3/4 xbar + x0 / 4 = (11/8, 3/4, 3/8, 2), y^{k+1} = 3/4 (-3, 2, 0) + (1, -1, 0) = (-5/4, 1/2, 0)
       A^T y^{k+1} = 3/4 (-3, -4, 0, 2) + (1, 1, 0, -1) = (-5/4, -2, 0, 1/2)   (= A^T of y^{k+1}, as it must)"""
    S = ar.Structure(3, 4, [0, 2, 4, 4], [0, 1, 1, 3])
    prob = arrays(A_VALUES=[1, 2, 1, 1], C=[-1, -2, 1, 0], LB=[0, 0, 0, 0], UB=[INF, 1, INF, INF], LO=[-INF, 2, -1], HI=[1, 2, INF])
    ctl = ctl_of(step_size=0.5, primal_weight=2.0, tau=0.25, sigma=1.0, k=7, cur=1, steps_taken=7, attempts=7, its_since_restart=2, target_steps=7)
    before = dict(arrays(X=[0, 0, 1, 0], Y=[0, 0, 2], ATY=[0, 0, 0, 0], SUM_X=[0, 0, 0, 0], SUM_Y=[0, 0, 0], LAST_RESTART_X=[4, 0, 0, 8],
                         LAST_RESTART_Y=[4, -4, 0], LAST_RESTART_ATY=[4, 4, 0, -4]), ctl=ctl, hal=dict(r=2.0, r_first=5.0, r2=4.0, r2_min=1.0, k=2))
    after_ctl = dict(ctl, last_dy2=4.25, last_interaction=-1.375, last_dx2=0.375, last_movement=3.0, k=8, cur=0, steps_taken=8, attempts=8,
                     its_since_restart=3, target_steps=8)
    after = dict(before, ctl=after_ctl, hal=dict(r=float(np.sqrt(3.0)), r_first=5.0, r2=3.0, r2_min=1.0, k=3),
                 **arrays(X=[1.375, 0.75, 0.375, 2], Y=[-1.25, 0.5, 0], ATY=[-1.25, -2, 0, 0.5], X_OTHER=[0, 0, 1, 0], Y_OTHER=[0, 0, 2],
                          ATY_OTHER=[0, 0, 0, 0], XBAR=[0.5, 1, 0.5, 0], AVG_X=[0.25, 0.5, 0.75, 0], AVG_Y=[-1.5, 1, 1],
                          PART_A=[2.25, 2.0], PART_AT=[-0.375, -1.0, 0.3125, 0.0625]))
    return S, prob, before, after


@pytest.mark.parametrize("exact", [False, True], ids=["longdouble", "fractions"])
def test_step_by_hand(exact):
    exact = exact or not er.LONGDOUBLE_IS_EXTENDED
    S, prob, before, after = hand_case()
    assert hr.weights(2) == (0.75, 0.25) and hr.weights(0) == (0.5, 0.5) and hr.weights(1)[0] == 2.0 / 3.0 and hr.weights(1)[1] == 1.0 - 2.0 / 3.0
    assert fractions.Fraction(float(hr.r2_of(before["ctl"], 4.25, -1.375, 0.375))) == 3
    r = hr.check_step(S, prob, before, after, "by hand", exact=exact)
    assert r["ratios"] == dict(y=0.0, aty=0.0, dy2=0.0, dx2=0.0, inter=0.0, part=0.0) and r["compared"] == dict(y=3, aty=4)
    assert (r["dy2"], r["dx2"], r["inter"], r["absinter"], r["r2"], r["error"], r["k_before"], r["cur_before"]) == (4.25, 0.375, -1.375, 1.375, 3.0, 0, 2, 1)
    # the bound of column 0: 2 w (L + 16) u |a y'| + 4 u (w (2 |v| + |a|) + w0 |a0|) = (3/2) 17 (3/2) u + 4 (9/4 + 1) u = 51.25 u
    for shift, inside in ((50.0, True), (52.0, False)):
        moved = dict(after, ATY=after["ATY"] + np.array([shift * er.U, 0, 0, 0]))
        if inside:
            assert hr.check_step(S, prob, before, moved, exact=exact)["ratios"]["aty"] == shift / 51.25
        else:
            with pytest.raises(AssertionError, match=r"A\^T y\^\{k\+1\} outside its bound"):
                hr.check_step(S, prob, before, moved, exact=exact)
    # the interaction: (n + 16) u sum |t dx| + sum |dx| bound_v = 20 (11/8) u + (1/4) 17 (3/2) u + (1/2) 18 4 u = 69.875 u
    for shift, inside in ((68.0, True), (72.0, False)):
        moved = dict(after, ctl=dict(after["ctl"], last_interaction=-1.375 + shift * er.U))
        moved["ctl"]["last_movement"] = hr.r2_of(before["ctl"], 4.25, moved["ctl"]["last_interaction"], 0.375)
        moved["hal"] = dict(after["hal"], r2=moved["ctl"]["last_movement"], r=float(np.sqrt(moved["ctl"]["last_movement"])))
        moved["PART_AT"] = np.array([-0.375 + shift * er.U, -1.0, 0.3125, 0.0625])
        if inside:
            assert hr.check_step(S, prob, before, moved, exact=exact)["ratios"]["inter"] == pytest.approx(shift / 69.875, rel=1e-12)
        else:
            with pytest.raises(AssertionError, match="inter outside its bound"):
                hr.check_step(S, prob, before, moved, exact=exact)
    # one number off at a time: the failure names the stage
    up = np.nextafter
    for key, value, stage in (("AVG_X", [0.25, 0.5, up(0.75, 1), 0], r"x' \(AVG_X\)"), ("XBAR", [0.5, 1, up(0.5, 1), 0], "xbar"),
                              ("X", [1.375, 0.75, 0.375, up(2, 3)], r"x\^\{k\+1\}"), ("AVG_Y", [-1.5, 1 + 2.0 ** -40, 1], r"y' \(AVG_Y\) outside"),
                              ("AVG_Y", [-1.5, 1, up(1, 2)], r"y' \(AVG_Y\) of the empty rows"), ("Y", [-1.25, up(0.5, 1), 0], r"y\^\{k\+1\}"),
                              ("ATY", [-1.25, -2, up(0, 1), 0.5], r"A\^T y\^\{k\+1\} outside its bound', inf, 2"),  # (a zero bound)
                              ("X_OTHER", [0, 0, up(1, 2), 0], "changed its own input X"), ("LAST_RESTART_ATY", [4, 4, 0, up(-4, 0)], "changed LAST_RESTART_ATY"),
                              ("SUM_Y", [0, 0, 1], "changed SUM_Y"), ("PART_A", [2.25, 2.0 + 2.0 ** -40], "partials of dy2"),
                              ("PART_AT", [-0.375, -1.0, 0.0625, 0.3125 + 2.0 ** -40], "partials of dx2"),
                              ("PART_AT", [0.3125, 0.0625, -0.375, -1.0], "partials of interaction")):
        with pytest.raises(AssertionError, match=stage):
            hr.check_step(S, prob, before, dict(after, **{key: np.array(value, dtype=np.float64)}), exact=exact)
    for key, value, stage in (("last_dy2", 4.25 * (1 + 2.0 ** -40), "dy2 outside"), ("last_dx2", 0.375 * (1 + 2.0 ** -40), "dx2 outside"),
                              ("last_movement", up(3.0, 4), "r2"), ("k", 7, "counter k"), ("cur", 1, "cur did not flip"), ("sigma", 2.0, "changed sigma"),
                              ("error", 1, "error"), ("its_since_restart", 1, "its_since_restart")):
        with pytest.raises(AssertionError, match=stage):
            hr.check_step(S, prob, before, dict(after, ctl=dict(after["ctl"], **{key: value})), exact=exact)
    for key, value, stage in (("r2", up(3.0, 4), r"hal\.r2"), ("r", up(np.sqrt(3.0), 2), r"hal\.r'"), ("r_first", float(np.sqrt(3.0)), "r_first"),
                              ("r2_min", 3.0, "r2_min"), ("k", 1, r"hal\.k")):
        with pytest.raises(AssertionError, match=stage):
            hr.check_step(S, prob, before, dict(after, hal=dict(after["hal"], **{key: value})), exact=exact)
    # k = 0 in front of the step: r_first IS written, r2_min follows a smaller r2
    b0 = dict(before, hal=dict(before["hal"], k=0, r2_min=9.0))
    a0 = dict(after, hal=dict(after["hal"], k=1, r_first=float(np.sqrt(3.0)), r2_min=3.0),
              **arrays(X=[2.25, 0.5, 0.25, 4], Y=[0.5, -1, 0], ATY=[0.5, 0, 0, -1]))  # w = w0 = 1/2: (xbar + x0) / 2 ...
    hr.check_step(S, prob, b0, a0, exact=exact)
    with pytest.raises(AssertionError, match="r_first"):
        hr.check_step(S, prob, b0, dict(a0, hal=dict(a0["hal"], r_first=5.0)), exact=exact)
    # the step error: r2 >= 1e100 from the device's own sums; hal keeps every field, the counters advance
    big = dict(after["ctl"], last_dy2=1e101, error=1)
    big["last_movement"] = hr.r2_of(before["ctl"], 1e101, -1.375, 0.375)
    assert hr.check_decision(before, dict(after, ctl=big, hal=before["hal"])) == dict(r2=big["last_movement"], error=1)
    with pytest.raises(AssertionError, match="hal behind the step error"):
        hr.check_decision(before, dict(after, ctl=big, hal=dict(before["hal"], k=3)))
    nan = dict(big, last_dy2=INF, last_interaction=-INF, last_movement=float("nan"))
    assert hr.check_decision(before, dict(after, ctl=nan, hal=before["hal"]))["error"] == 1


@pytest.mark.parametrize("exact", [False, True], ids=["longdouble", "fractions"])
def test_restart_by_hand(exact):
    """x = (3, 0, 0, 0) against the anchor (0, 4, 0, 0): 5; y = 0 against (0, 12, 5): 13; theta = 1/2 at weight 4:
    w = exp(ln(13 / 5) / 2 + ln(4) / 2) = sqrt(10.4)"""
    exact = exact or not er.LONGDOUBLE_IS_EXTENDED
    ctl = ctl_of(step_size=0.5, primal_weight=4.0, tau=0.125, sigma=2.0, k=9, cur=1, steps_taken=9, attempts=9, its_since_restart=4, target_steps=9)
    hal = dict(r=2.0, r_first=5.0, r2=4.0, r2_min=1.0, k=4)
    before = dict(arrays(X=[3, 0, 0, 0], Y=[0, 0, 0], ATY=[1, 2, 3, 4], LAST_RESTART_X=[0, 4, 0, 0], LAST_RESTART_Y=[0, 12, 5], LAST_RESTART_ATY=[0, 0, 0, 0]),
                  ctl=ctl, hal=hal)
    w = float(np.exp(0.5 * np.log(13.0 / 5.0) + 0.5 * np.log(4.0)))
    assert w == pytest.approx(np.sqrt(10.4), rel=1e-15)
    moved = dict(before, LAST_RESTART_X=before["X"], LAST_RESTART_Y=before["Y"], LAST_RESTART_ATY=before["ATY"], hal=dict(hal, k=0))
    after = dict(moved, ctl=dict(ctl, primal_weight=w, tau=0.5 / w, sigma=0.5 * w, its_since_restart=0))
    r = hr.check_restart(before, after, (5.0, 13.0), 0.5, exact=exact)
    assert r["smoothed"] and r["ratios"]["dist"] == 0.0 and r["ratios"]["weight"] <= 1.0
    ref, rel = hr.weight_reference(0.5, (5.0, 13.0), 4.0)
    assert rel == er.U * (8.0 + 6.0 * (abs(float(0.5 * np.log(np.longdouble(2.6)))) + abs(float(0.5 * np.log(np.longdouble(4.0))))))
    kept = dict(moved, ctl=dict(ctl, its_since_restart=0))
    assert not hr.check_restart(before, kept, (5.0, 13.0), -1.0, exact=exact)["smoothed"]
    with pytest.raises(AssertionError, match="without smoothing"):
        hr.check_restart(before, after, (5.0, 13.0), -1.0, exact=exact)
    with pytest.raises(AssertionError, match="primal_weight outside its bound"):
        hr.check_restart(before, dict(after, ctl=dict(after["ctl"], primal_weight=w * (1 + 1e-13))), (5.0, 13.0), 0.5, exact=exact)
    with pytest.raises(AssertionError, match="primal_weight outside its bound"):
        hr.check_restart(before, kept, (5.0, 13.0), 0.5, exact=exact)
    with pytest.raises(AssertionError, match="tau / sigma"):
        hr.check_restart(before, dict(after, ctl=dict(after["ctl"], tau=0.125)), (5.0, 13.0), 0.5, exact=exact)
    with pytest.raises(AssertionError, match="dist outside its bound"):
        hr.check_restart(before, after, (5.0 * (1 + 1e-14), 13.0), 0.5, exact=exact)
    with pytest.raises(AssertionError, match="anchor LAST_RESTART_ATY"):
        hr.check_restart(before, dict(after, LAST_RESTART_ATY=before["LAST_RESTART_ATY"]), (5.0, 13.0), 0.5, exact=exact)
    with pytest.raises(AssertionError, match="hal.k"):
        hr.check_restart(before, dict(after, hal=hal), (5.0, 13.0), 0.5, exact=exact)
    with pytest.raises(AssertionError, match="the restart changed hal"):
        hr.check_restart(before, dict(after, hal=dict(hal, k=0, r_first=0.0)), (5.0, 13.0), 0.5, exact=exact)
    # a distance under the threshold of 1e-10: 2^-34 = 5.8e-11
    near = dict(before, LAST_RESTART_X=np.array([3 + 2.0 ** -34, 0, 0, 0]))
    d = float(near["LAST_RESTART_X"][0] - 3.0)
    assert d == 2.0 ** -34 <= 1e-10 and not hr.check_restart(near, dict(kept, ctl=dict(ctl, its_since_restart=0)), (d, 13.0), 0.5, exact=exact)["smoothed"]


# ---- the GPU test's scenario on the float64 stand-in ------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=LPS, ids=LP_IDS)
def lp(request):
    p, x, y = edge_lp(*request.param)
    return request.param, p, x, y, scaling_of(p)


def test_long_rows_as_equalities_on_the_stand_in(lp, request):
    """the second LP of every id: the same matrix and start, the long and the dense rows as equality rows -- every one of them then
    has a y' that moves with its row sum (nonzero, and not clamped), on each of the three checked steps"""
    spec, p, x0, y0, (dr, dc) = lp
    rows = tuple(LONG_ROWS) + (tuple(DENSE_ROWS) if spec[1] else ())
    hidden = [r for r in rows if not (np.isfinite(p["lo"][r]) and p["lo"][r] == p["hi"][r])]
    print("LONG ROWS %s: %d of %d are no equality rows as the LP stands" % (request.node.callspec.id, len(hidden), len(rows)))
    q = sc.rows_as_equalities(p, rows)
    assert all(q["lo"][r] == q["hi"][r] and np.isfinite(q["lo"][r]) for r in rows) and (np.diff(q["offsets"]) == np.diff(p["offsets"])).all()
    dev, S, prob = sc.stand_in(q, x0, y0, dr, dc)
    worst, record = sc.steps_and_a_restart(dev, S, prob, request.node.callspec.id)
    print(worst.line(request.node.callspec.id + " long rows as equalities"))
    assert max(worst.values()) <= 1.0 and all(r["inter_bound_rel"] <= INTER_BOUND_REL and r["compared"] == dict(y=S.m, aty=S.n) for r in record)
    assert (dev.get("AVG_Y")[list(rows)] != 0.0).all()


def test_scenario_on_the_stand_in(lp, request):
    """every bound holds for plain float64 sums, and the scenario and the LP have the properties the GPU test relies on"""
    spec, p, x0, y0, (dr, dc) = lp
    name = request.node.callspec.id
    dev, S, prob = sc.stand_in(p, x0, y0, dr, dc)
    # the LP: empty rows and columns, rows and columns with a workgroup of their own, the 2049-entry row
    assert (S.len_r == 0).sum() >= 60 and (S.len_c[list(EMPTY_COLS)] == 0).all() and (S.len_c == 0).sum() >= len(EMPTY_COLS)
    assert all(l <= S.len_r[r] <= l + len(LONG_COLS) for r, l in LONG_ROWS.items())  # (a long column may pass through a long row)
    assert (S.len_r > LONG_ROW).sum() >= len(LONG_ROWS) and (S.len_c > LONG_ROW).sum() == len(LONG_COLS) and S.len_c.max() == S.len_c[LONG_COLS[1]] == spec[0]
    assert spec[0] > PANEL_OWN_ROW or spec[0] == 2400  # (the gather-free layout holds no column of 4500: its ids take the LP with 2400)
    record = []
    worst = sc.run_scenario(dev, S, prob, name, record)
    print(worst.line(name))
    assert max(worst.values()) <= 1.0 and min(worst[k] for k in ("y", "aty", "dy2", "dx2", "inter", "dist", "weight")) > 0.0, worst
    assert len(record) == 6
    for r in record:
        assert r["dx2"] > 0.0 and r["dy2"] > 0.0 and r["r2"] > 0.0, r
        assert r["inter_bound_rel"] <= INTER_BOUND_REL, r["inter_bound_rel"]
        assert r["compared"] == dict(y=S.m, aty=S.n), r["compared"]  # no element is excluded from any comparison
    assert dev.hal()["r2_min"] > 0.0  # (the minimum over EVERY step, the run of seven included)
    print("INTER BOUND %s worst %.3g of sum |t dx|" % (name, max(r["inter_bound_rel"] for r in record)))


@pytest.mark.parametrize("name", ["shapes", "chunks"])
def test_tail_lps_on_the_stand_in(name):
    """the two LPs of tests/test_panel_epilogue_tail_gpu.py, which the GPU test's tail cases step on: every step moves both halves
    and stays inside the bounds in plain float64"""
    from test_panel_epilogue_tail_gpu import lp as tail_lp
    p, x0, y0 = tail_lp(name)[:3]
    dr, dc = scaling_of(p)
    dev, S, prob = sc.stand_in(p, x0, y0, dr, dc)
    worst, record = sc.steps_and_a_restart(dev, S, prob, name)
    print(worst.line("stand-in " + name))
    assert max(worst.values()) <= 1.0 and all(r["inter_bound_rel"] <= INTER_BOUND_REL and r["compared"] == dict(y=S.m, aty=S.n) for r in record)


@pytest.mark.parametrize("wrong,stage,steps", [
    ("w", r"x\^\{k\+1\}", 1), ("anchor", r"A\^T y\^\{k\+1\} outside its bound", 1), ("avg_y", r"y' \(AVG_Y\) outside its bound", 2),
    ("r_first", "r_first", 2), ("factor2", r"r2 \(last_movement\)", 1), ("row-entry", r"y' \(AVG_Y\) outside its bound.*, 2999\)", 1),
    ("xprime", r"x' \(AVG_X\)", 1)])
def test_the_rules_name_the_stage(wrong, stage, steps):
    """a stand-in that is wrong in ONE place fails check_step at that stage (and, for the dropped entry, at that row).  Two of them
    show from the second step on only: r_first is written rightly at k = 0, and right behind a restart the anchor is the iterate, so
    that y^{k+1} = (2 y' - y) / 2 + y / 2 IS y' -- which is why the scenario checks steps at k = 1 and 2 as well."""
    p, x0, y0 = edge_lp(*LPS[0])
    dr, dc = scaling_of(p)
    drop = None
    if wrong == "row-entry":  # the entry of the 2049-nonzero row that weighs most in the first step's A xbar
        dev, S, prob = sc.stand_in(p, x0, y0, dr, dc)
        dev.run(1)
        a, b = S.off[2999], S.off[3000]
        assert 2049 <= b - a <= 2049 + len(LONG_COLS)
        drop = (2999, int(np.argmax(np.abs(prob["A_VALUES"][a:b] * dev.get("XBAR")[S.idx[a:b]]))))
        # On the LP as it stands row 2999 is a FREE row: y' = 0 there whatever its sum, and the dropped entry shows nowhere ...
        assert p["lo"][2999] == -INF and p["hi"][2999] == INF
        dev, S, prob = sc.stand_in(p, x0, y0, dr, dc, wrong=wrong, drop=drop)
        sc.one_step(dev, S, prob, "a free row hides its sum")
        p = sc.rows_as_equalities(p, LONG_ROWS)  # ... so the GPU test ALSO runs every id with the long rows as equality rows
    dev, S, prob = sc.stand_in(p, x0, y0, dr, dc, wrong=wrong, drop=drop)
    for i in range(steps - 1):
        sc.one_step(dev, S, prob, "%s step %d" % (wrong, i))  # (nothing is wrong yet)
    with pytest.raises(AssertionError, match=stage):
        sc.one_step(dev, S, prob, wrong)


# ---- the scalar branches ---------------------------------------------------------------------------------------------------------------------
def overflow_lp():
    """tiny_lp("dual-only") with row 0 turned into a "<=" row: y_0 = 1e200 is projected to 0 there, dy_0^2 overflows"""
    p, x0, y0 = asc.tiny_lp("dual-only")
    lo = p["lo"].copy()
    lo[0] = -INF
    return dict(p, lo=lo), x0, y0


def test_fixed_point_on_the_stand_in():
    p, x0, y0 = asc.tiny_lp("fixed-point")
    dev, S, prob = sc.stand_in(p, x0, y0, np.ones(p["m"]), np.ones(p["n"]))
    start = sc.snapshot(dev)
    for i in range(2):
        r, before, after = sc.one_step(dev, S, prob, "fixed point %d" % i)
        assert (r["r2"], r["dx2"], r["dy2"], r["inter"], r["error"]) == (0.0, 0.0, 0.0, 0.0, 0), r
        assert (after["hal"]["r"], after["hal"]["r_first"], after["hal"]["r2_min"]) == (0.0, 0.0, 0.0)
        if i == 0:
            assert all(ar.bits_equal(after[k], start[k]) for k in ("X", "Y", "ATY")), "the fixed point moved"
    assert np.abs(after["X"] - start["X"]).max() <= 2.0 * er.U * np.abs(start["X"]).max()


def test_overflow_on_the_stand_in():
    p, x0, y0 = overflow_lp()
    dev, S, prob = sc.stand_in(p, x0, y0, np.ones(p["m"]), np.ones(p["n"]))
    assert prob["LO"][0] == -INF and np.isfinite(prob["HI"][0])
    y = dev.get("Y")
    y[0] = 1e200
    dev.put("Y", y)
    before = sc.snapshot(dev)
    dev.run(1)
    after = sc.snapshot(dev, hr.AFTER)
    assert hr.check_decision(before, after, "overflow")["error"] == 1 and after["ctl"]["last_dy2"] == INF and after["AVG_Y"][0] == 0.0
    assert after["hal"] == before["hal"] and (after["ctl"]["attempts"], after["ctl"]["steps_taken"], after["ctl"]["cur"]) == (1, 1, 1)
    dev.run(2)
    assert dev.ctl()["attempts"] == 1


# ---- the resident one-workgroup loop: its rules, its LPs and its cases on the resident stand-in -----------------------------------------
# What tests/test_halpern_resident_steps_gpu.py needs of tests/resident_lps.py, asserted below on the reference alone; the GPU file takes
# its id lists from here.
EVAL_STEPS = (1, 2, 3, 4, 40)  # T(z^k) behind these many steps is looked at; the GPU test evaluates behind 3 and 4
G_IS_ZERO = tuple(rl.SCENARIO) + tuple(rl.FULL) + ("past-n", "past-nnz", "cols-only")  # ids with a column whose reduced-cost gradient is exactly 0
LINF_POSITIVE = tuple(k for k in rl.ALL if not k.startswith("minimal"))                # ids on which both l-infinity figures are positive
EVALUATED = tuple(k for k in rl.ALL if k in G_IS_ZERO and k in LINF_POSITIVE)          # where test_eval_layouts_gpu's checks apply as they stand
COMPOSITION_LPS = ("t0", "minimal-1x2")
RESTARTS_IN_1000 = 6


def resident_stand_in(name, **kw):
    p, x0, y0 = rl.lp(name)
    dr, dc = fr.scaling(p)
    return sc.stand_in(p, x0, y0, dr, dc, resident=True, **kw) + (p, dr, dc)


@pytest.mark.parametrize("name", list(rl.ALL))
def test_resident_scenario_on_the_stand_in(name):
    """the six-part scenario by the resident rules: y' and A^T y^{k+1} bit for bit, the three sums and the distances inside their bounds"""
    dev, S, prob, p, dr, dc = resident_stand_in(name)
    record = []
    worst = sc.run_scenario(dev, S, prob, name, record, resident=True)
    print(worst.line("stand-in " + name))
    assert max(worst.values()) <= 1.0 and worst["y"] == worst["aty"] == worst["part"] == 0.0, worst
    assert len(record) == 6 and all(r["error"] == 0 and r["compared"] == dict(y=S.m, aty=S.n) for r in record)
    assert all(r["inter_bound_rel"] <= INTER_BOUND_REL for r in record)


@pytest.mark.parametrize("name", list(rl.FULL) + list(rl.EDGE))
def test_edge_steps_on_the_stand_in(name):
    """the GPU test's edge case: each of the three steps moves both halves and the restart behind them is smoothed, on every edge LP"""
    dev, S, prob = resident_stand_in(name)[:3]
    worst, record = sc.edge_steps(dev, S, prob, name)
    print(worst.line("stand-in edge " + name))
    assert max(worst.values()) <= 1.0 and len(record) == 5, worst


@pytest.mark.parametrize("name", list(rl.ALL))
def test_resident_lps_hold_what_the_halpern_tests_need(name):
    """the scenario's conditions (the test above asserts them on every id); hardly a reduced-cost tie at any evaluated T(z^k); which ids
    hold a column with g = 0 and positive l-infinity figures (test_eval_layouts_gpu's checks ask for both); and the restatement
    restarts at its first major iteration, so that a solve of 400 steps runs the restart kernels"""
    dev, S, prob, p, dr, dc = resident_stand_in(name)
    share = 0.0
    for steps in EVAL_STEPS:
        dev.run(steps)
        c = dev.ctl()
        assert (c["steps_taken"], c["error"]) == (steps, 0), c
        for rule in (True, False):
            ref = er.evaluate(p, dev.get("AVG_X") * dc, dev.get("AVG_Y") * dr, rule_finite=rule, eps_p=1e-4, eps_d=1e-4)
            share = max(share, float(ref["near_tie"].mean()))
            assert ref["near_tie"].mean() <= 0.005, (name, steps, rule)
            assert bool(ref["g_is_zero"].any()) == (name in G_IS_ZERO), (name, steps, rule)
            positive = ref["LINF_PRES_REL"] > 0.0 and ref["LINF_DRES_REL"] > 0.0
            assert positive == (name in LINF_POSITIVE), (name, steps, rule, ref["LINF_PRES_REL"], ref["LINF_DRES_REL"])
    import scipy.sparse as sp
    fresh = resident_stand_in(name)[0]
    it = H.HalpernIteration(sp.csr_matrix((prob["A_VALUES"], S.idx, S.off), shape=(S.m, S.n)), prob["C"], prob["LB"], prob["UB"], prob["LO"], prob["HI"],
                            fresh.it.eta, fresh.it.omega, x=fresh.it.x, y=fresh.it.y)
    r = H.run(p, it, dr, dc, eps=0.0, max_iterations=1000)
    print("TIES %s worst share %.4f; restarts %d flags %s" % (name, share, r["restarts"], "".join("R" if f else "." for f in r["flags"])))
    assert r["status"] == "IterationLimit" and r["flags"][0] and r["restarts"] == RESTARTS_IN_1000 and sum(r["flags"][:10]) >= 1, r["flags"]


def test_evaluated_ids_are_what_the_issue_names():
    assert EVALUATED == ("t0", "t1", "t2", "t0-full", "t1-full", "t2-full", "past-n", "past-nnz", "cols-only")
    assert set(rl.ALL) - set(G_IS_ZERO) == {"rows-only", "spanning", "minimal-1x2", "minimal-2x1"}


@pytest.mark.parametrize("start", sc.STARTS)
@pytest.mark.parametrize("name", COMPOSITION_LPS)
def test_composition_case_on_the_stand_in(name, start):
    """the three starts exist on these LPs -- the restart of `restarted` is smoothed and moves the anchor -- and the stand-in passes
    (the equality itself is trivial on the host)"""
    assert sc.check_composition(lambda: resident_stand_in(name)[:3], name, start) == sc.LAUNCH_STEPS == 12


def _seen_row(name="t0"):
    """an equality row of at least two entries, and the position of the entry that weighs most in the first step's A xbar"""
    dev, S, prob, p, dr, dc = resident_stand_in(name)
    st = sc.snapshot(dev)
    xbar = hr.primal(prob, st["ctl"], st)["xbar"]
    for row in np.nonzero((p["lo"] == p["hi"]) & (S.len_r >= 2))[0]:
        a, b = S.off[row], S.off[row + 1]
        weight = np.abs(prob["A_VALUES"][a:b] * xbar[S.idx[a:b]])
        if weight.max() > 0.0:
            return int(row), int(np.argmax(weight))
    raise AssertionError("no equality row whose sum is seen")


def _seen_at_entry(name="t0"):
    """(entry of A^T's CSR, its column): one ulp on that value changes the bits of the first step's A^T y^{k+1} in that column"""
    dev, S, prob, p, dr, dc = resident_stand_in(name)
    st = sc.snapshot(dev)
    dev.run(1)
    yp, base = dev.get("AVG_Y"), prob["A_VALUES"][S.order]
    for j in np.nonzero(S.len_c >= 1)[0]:
        e = S.t_off[j]
        sums = []
        for first in (base[e], np.nextafter(base[e], np.inf)):
            v = np.float64(0.0)
            for q in range(e, S.t_off[j + 1]):
                v = v + (first if q == e else base[q]) * yp[S.t_rows[q]]
            sums.append(hr.combine(0, v, st["ATY"][j], st["LAST_RESTART_ATY"][j]))
        if not ar.bits_equal([sums[0]], [sums[1]]):
            return int(e), int(j)
    raise AssertionError("no entry of A^T whose last bit is seen")


@pytest.mark.parametrize("wrong,stage,steps", [
    ("w", r"x\^\{k\+1\}", 1), ("anchor", r"'A\^T y\^\{k\+1\}', \d+", 1), ("avg_y", r"\"y' \(AVG_Y\)\", \d+", 1), ("r_first", "r_first", 2),
    ("factor2", r"r2 \(last_movement\)", 1), ("row-entry", r"\"y' \(AVG_Y\)\", %d\)", 1), ("xprime", r"x' \(AVG_X\)", 1),
    ("at-values", r"'A\^T y\^\{k\+1\}', %d\)", 1)])
def test_the_resident_rules_name_the_stage(wrong, stage, steps):
    """every wrong stand-in of the layouts' rules, and the one whose A^T values are A's, fails check_step(resident=True) at its stage --
    the dropped entry at its row, the last bit of one A^T value at its column.  (AVG_Y holding y^{k+1} shows on the FIRST step here:
    fl(fl(2 y' - y) / 2 + y / 2) is y' to within the layouts' bound, not to the bit.)"""
    kw = {}
    if wrong == "row-entry":
        row, position = _seen_row()
        kw, stage = dict(drop=(row, position)), stage % row
    if wrong == "at-values":
        entry, column = _seen_at_entry()
        kw, stage = dict(at_entry=entry), stage % column
        dev, S, prob = resident_stand_in("t0", **kw)[:3]  # (the stand-in that reads AT_VALUES passes with that entry)
        assert (prob["AT_VALUES"] != prob["A_VALUES"][S.order]).sum() == 1
        sc.one_step(dev, S, prob, "AT_VALUES read", resident=True)
    dev, S, prob = resident_stand_in("t0", wrong=wrong, **kw)[:3]
    for i in range(steps - 1):
        sc.one_step(dev, S, prob, "%s step %d" % (wrong, i), resident=True)  # (nothing is wrong yet)
    with pytest.raises(AssertionError, match=stage):
        sc.one_step(dev, S, prob, wrong, resident=True)


@pytest.mark.parametrize("wrong,stage", [("last-store", r"one launch against single steps', 'X_OTHER'"),
                                         ("made", r"a launch without a step changed', 'AVG_X'")])
def test_the_composition_case_names_the_buffer(wrong, stage):
    """z^k not stored on the last step of a multi-step launch, and a launch without a step that rewrites AVG_X: a single-step check
    sees neither (there the store is of what the side holds already, and every checked launch makes a step); check_composition does"""
    dev, S, prob = resident_stand_in("t0", wrong=wrong)[:3]
    for i in range(3):
        sc.one_step(dev, S, prob, "%s step %d" % (wrong, i), resident=True)
        hr.check_last_step_store(S, prob, sc.snapshot(dev, hr.AFTER_RESIDENT), wrong)
    for steps in (5, 4):  # (an odd and an even number of steps in one launch)
        dev.run(dev.ctl()["steps_taken"] + steps)
        if wrong == "last-store":
            with pytest.raises(AssertionError, match="is not the point whose image the average slots hold"):
                hr.check_last_step_store(S, prob, sc.snapshot(dev, hr.AFTER_RESIDENT), wrong)
        else:
            hr.check_last_step_store(S, prob, sc.snapshot(dev, hr.AFTER_RESIDENT), wrong)
    for start in sc.STARTS:
        with pytest.raises(AssertionError, match=stage):
            sc.check_composition(lambda: resident_stand_in("t0", wrong=wrong)[:3], "t0", start)
