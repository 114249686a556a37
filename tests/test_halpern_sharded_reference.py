"""CPU: the scenario of tests/test_halpern_sharded_gpu.py (tests/halpern_step_scenario.py) on W float64 stand-in ranks
(tests/halpern_sharded_ranks.HalpernStandInRanks), behind the SAME assembly the GPU test uses (HalpernAssembled).  No library code of
the feature runs here: the test passes with and without it.  What it proves is what the GPU test rests on:

  * the assembly reads nothing a rank does not own.  The stand-in ranks shard the Halpern step as enqueue_attempt does on the
    owner-computes dataflow -- row blocks from capi.partition_rows, slices from sharded_ranks.slices_of -- and fill everything a rank
    does not own at that point of the dataflow with NaN: x', xbar, x^{k+1} and A^T y^{k+1} outside the slice; X, ATY and AVG_X are
    replicated by the epilogue only, AVG_X from the owners' x'.  A value taken from the wrong rank poisons the check behind it
    (test_the_assembly_sees_a_stale_entry shows it failing, at the stage).
  * the LPs keep the scenario's properties in the sharded order of summation: every checked step has dx2 > 0 and dy2 > 0, both
    distances of the first restart are far above 1e-10 (run_scenario asserts > 1e-6), and no row block is empty.
  * every derived bound of tests/halpern_step_reference.py holds for plain float64 sums in that order.

The three sums and the reduction over the ranks.  A rank adds its own partials (the stand-in: one per sum; the device: one per
workgroup, by k_pack_step_sums or k_halpern_decision_p2p) and the W ranks' sums are added in rank order.  The assembly presents PART_A
as the ranks' partials side by side and PART_AT as all ranks' interaction partials followed by all ranks' dx2 partials, nb in total
each.  halpern_step_reference's rule for the partials is |sum in the control block - exact sum of the partials| <= (nb + 16) u
sum |partial| FOR ANY SUMMATION TREE over the nb partials (Higham, section 4.2: a tree of nb leaves has at most nb - 1 additions
on any path).  "Each rank's own tree, then W - 1 additions in rank order" IS one tree over the nb leaves: its longest path has at most
(nb_r - 1) + (W - 1) <= nb - 1 additions, where nb_r <= nb - (W - 1) is the largest rank's count, because every other rank holds at
least one partial.  So the W - 1 additions are counted inside nb - 1 already, and the bound is used as it stands, with nb the total.
The same holds for dy2, dx2 and the interaction against the vectors: their (N + 16) u rules are stated for any tree over the N terms,
and a rank's slice or row block followed by the rank-order additions is such a tree.  No bound is widened.  The restart's dual
distance likewise: W block sums added in rank order are a tree over the m squares."""
import numpy as np
import pytest

import attempt_reference as ar
import attempt_scenario as asc
import halpern_sharded_ranks as hs
import halpern_step_reference as hr
import halpern_step_scenario as sc
import sharded_ranks as sr
from test_attempt_reference import LP_IDS, LPS, scaling_of
from eval_lps import edge_lp
from test_halpern_step_reference import overflow_lp

# (test_attempt_reference.LPS: 0 the 6000 x 6000 LP of the stream, panel and jagged ids, 1 the gather-free id's)
WORLD4 = (0, 1)


@pytest.fixture(scope="module")
def sharded_lps():
    out = []
    for spec in LPS[:2]:
        p, x, y = edge_lp(*spec)
        out.append((p, x, y, scaling_of(p)))
    return out


def _scenario(lp, world, name):
    p, x0, y0, (dr, dc) = lp
    dev, S, prob = hs.stand_in(p, x0, y0, dr, dc, world)
    assert all(b > a for a, b in zip(dev.bounds[:-1], dev.bounds[1:])), ("an empty row block", dev.bounds)
    assert dev.slices == sr.slices_of(p["n"], world, "owner")
    record = []
    worst = sc.run_scenario(dev, S, prob, name, record)
    print(worst.line(name.replace(" ", "-")))
    assert max(worst.values()) <= 1.0 and min(worst[k] for k in ("y", "aty", "dy2", "dx2", "inter", "dist", "weight")) > 0.0, worst
    assert len(record) == 6
    for r in record:
        assert r["dx2"] > 0.0 and r["dy2"] > 0.0 and r["r2"] > 0.0, r
        assert r["compared"] == dict(y=S.m, aty=S.n), r["compared"]  # no element is excluded from any comparison
    # between the runs every rank holds the replicated vectors whole, and what is slice-only is NaN elsewhere on every rank
    for k in dev.b.ranks:
        cur = k.c["cur"]
        assert np.isfinite(k.x[cur]).all() and np.isfinite(k.aty[cur]).all() and np.isfinite(k.v["AVG_X"]).all()
        if world > 1:
            outside = np.ones(S.n, bool)
            outside[k.c0:k.c0 + k.nc] = False
            assert np.isnan(k.v["XBAR"][outside]).all()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_sharded_scenario_on_the_stand_in_ranks(sharded_lps, world):
    _scenario(sharded_lps[0], world, "stand-in ranks world %d" % world)


@pytest.mark.parametrize("which", WORLD4, ids=[LP_IDS[w] for w in WORLD4])
def test_sharded_scenario_of_the_layout_cases_on_the_stand_in_ranks(sharded_lps, which):
    _scenario(sharded_lps[which], 4, "stand-in ranks %s world 4" % LP_IDS[which])


def test_sharded_scenario_on_the_band_lp():
    p, x0, y0 = sr.band_lp(*sr.BAND_LP)
    _scenario((p, x0, y0, scaling_of(p)), 4, "stand-in ranks band world 4")


def test_fixed_point_with_empty_slices():
    p, x0, y0 = asc.tiny_lp("fixed-point")
    dev, S, prob = hs.stand_in(p, x0, y0, np.ones(p["m"]), np.ones(p["n"]), 8)
    assert [s[1] for s in dev.slices] == [16, 16, 16, 12, 0, 0, 0, 0]
    start = sc.snapshot(dev)
    for i in range(2):
        r, before, after = sc.one_step(dev, S, prob, "fixed point %d" % i)
        assert (r["r2"], r["dx2"], r["dy2"], r["inter"], r["error"]) == (0.0, 0.0, 0.0, 0.0, 0), r
        if i == 0:
            assert all(ar.bits_equal(after[k], start[k]) for k in ("X", "Y", "ATY")), "the fixed point moved"


def test_overflow_with_empty_slices():
    p, x0, y0 = overflow_lp()
    dev, S, prob = hs.stand_in(p, x0, y0, np.ones(p["m"]), np.ones(p["n"]), 8)
    assert [s[1] for s in dev.slices] == [16, 16, 16, 12, 0, 0, 0, 0]
    y = dev.get("Y")
    y[0] = 1e200
    dev.put("Y", y)
    before = sc.snapshot(dev)
    dev.run(1)
    after = sc.snapshot(dev, hr.AFTER)  # (ctl() and hal(): every rank holds rank 0's)
    assert hr.check_decision(before, after, "overflow")["error"] == 1 and after["ctl"]["last_dy2"] == np.inf and after["AVG_Y"][0] == 0.0
    assert after["hal"] == before["hal"] and (after["ctl"]["attempts"], after["ctl"]["steps_taken"], after["ctl"]["cur"]) == (1, 1, 1)
    assert dev.run(2)["attempts"] == 1


def test_the_assembly_sees_a_stale_entry(sharded_lps):
    """what the stand-in ranks prove rests on this: a value taken from a rank that does not own it fails the check, at the stage --
    for a slice-only buffer (xbar, through a slice that begins one column early: the other side of the pairs and x' are replicated
    there, xbar is NaN) and for the replicated x' (AVG_X left un-replicated on one
    rank: the assembly compares every rank with rank 0)"""
    p, x0, y0, (dr, dc) = sharded_lps[0]
    dev, S, prob = hs.stand_in(p, x0, y0, dr, dc, 4)
    sc.one_step(dev, S, prob, "a sound step")
    before = sc.snapshot(dev)
    dev.run(before["ctl"]["steps_taken"] + 1)
    kept = list(dev.slices)
    dev.slices = [kept[0], (kept[1][0] - 1, kept[1][1] + 1), *kept[2:]]  # (rank 1's slice taken one column early: column 1503 is rank 0's)
    dev._cache.clear()
    after = sc.snapshot(dev, hr.AFTER)
    with pytest.raises(AssertionError, match="xbar"):
        hr.check_step(S, prob, before, after, "stale")
    dev.slices = kept
    dev._cache.clear()
    hr.check_step(S, prob, before, sc.snapshot(dev, hr.AFTER), "sound again")
    dev.b.ranks[2].v["AVG_X"] = np.full(S.n, np.nan)  # (a rank the epilogue forgot)
    dev._cache.clear()
    with pytest.raises(AssertionError, match="AVG_X: rank 2 does not hold rank 0's bits"):
        dev.get("AVG_X")
