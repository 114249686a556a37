"""GPU: infeasibility detection for the members of a Halpern LOCKSTEP batch (solver mode 4 with cuoptamd_settings::halpern_lockstep,
halpern_infeasibility and halpern_lockstep_rays; kernels_batch_halpern_ray.hip, docs/design/04d_halpern_mode.md "The K-wide ray pass").
The contract: the K-wide plain product gives every member the bits of the parent's own plain product; the ray pass only reads the
iterates, so every member still gets, BIT FOR BIT, what its own freshly created Solver(mode=4, halpern_infeasibility=1) gives -- the
lockstep batch's state, the four figures, the verdict and the step at which it falls, the certificate --; and the figures are those of
the certificate the member hands out.  The family of LPs and the verdict names: tests/halpern_lockstep_rays_case.py."""
import numpy as np
import pytest

import halpern_lockstep_rays_case as case
import halpern_ray_reference as R
from cuopt_amd import capi
from halpern_lockstep_case import KEYS_F64, KEYS_INT, close_all, layout_is, same, state
from halpern_lockstep_rays_case import FIGURES, KW, LIMIT, RAY_VERDICTS, SINGLE, VERDICT, family, make_batch, member_lp, same_snapshot, snapshot
from test_halpern_infeasibility_gpu import check_verdict

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- 1. the K-wide plain product against the parent's own --------------------------------------------------------------------------
def product_inputs(k, cols, rng):
    """K random vectors: one with exact zeros in half of its places, one all zero, one with a few entries of 1e300 (K = 2: the first
    carries the zeros and the large entries)"""
    vs = [rng.standard_normal(cols) for _ in range(k)]
    vs[0][rng.choice(cols, size=cols // 2, replace=False)] = 0.0
    vs[1][:] = 0.0
    big = vs[2] if k > 2 else vs[0]
    big[rng.choice(cols, size=5, replace=False)] = 1e300
    return vs


@pytest.mark.parametrize("base", ["large", "small"])
@pytest.mark.parametrize("layout", ["panel", "stream"])
@pytest.mark.parametrize("k", [2, 4, 8, 16])
def test_k_wide_plain_product_is_the_parents_own(k, layout, base, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    solvers, batch = make_batch(base, list(range(k)), **KW)
    layout_is(solvers[0], layout)
    parent, rng = solvers[0], np.random.default_rng(100 * k + len(layout))
    for transpose in (False, True):
        cols, rows = (parent.m, parent.n) if transpose else (parent.n, parent.m)
        vs = product_inputs(k, cols, rng)
        want = [parent.device.spmv(v, transpose, rows) for v in vs]
        assert np.max(np.abs(want[2 if k > 2 else 0])) > 1e250 and not np.any(want[1])  # (the large entries reach the sums; 0 stays 0)
        for on in (None, [0 if l % 3 == 2 else 1 for l in range(k)]):
            got = batch.spmv(vs, transpose=transpose, on=on)
            for l in range(k):
                if on is None or on[l]:
                    assert np.array_equal(bits(got[l]), bits(want[l])), (k, layout, base, transpose, l, int(np.sum(bits(got[l]) != bits(want[l]))))
                else:  # (the sentinel the output buffer was made with)
                    assert np.all(np.isnan(got[l])), (k, layout, base, transpose, l)
    close_all(batch, solvers)


# ---- 2. figures and trajectories, bit for bit ---------------------------------------------------------------------------------------
def batch_against_singles(base, k, layout, single, checkpoints=True, **kw):
    """the batch of the first k members against their single solves after advance(40), after advance(130) and at the end; the counters
    of the passes on the way.  Returns the final results."""
    solvers, batch = make_batch(base, list(range(k)), **dict(KW, **kw))
    layout_is(solvers[0], layout)
    if checkpoints:
        got = batch.advance(40)
        st = batch.ray_stats()
        print(k, layout, "after 40:", st)
        assert st == dict(wide_passes=1, members_served=k, single_passes=0), st  # (one period, one K-wide pass, every member in it)
        for l in range(k):
            assert got[l]["steps_taken"] == 40 and got[l]["num_major_iterations"] == 1
            same_snapshot(snapshot(solvers[l], got[l], False), single[l][0], "LP %d after 40 iterations" % l)
        # (the snapshot's second rule is not what the period left: a single pass per member, here and in the single solves alike)
        assert batch.ray_stats()["single_passes"] == k
        got = batch.advance(130)  # (170 iterations: ends inside a period -- the passes at 80, 120, 160; none at 170)
        st = batch.ray_stats()
        print(k, layout, "after 170:", st)
        assert st == dict(wide_passes=4, members_served=4 * k, single_passes=k), st
        for l in range(k):
            assert got[l]["steps_taken"] == 170 and got[l]["num_major_iterations"] == 4
            same_snapshot(snapshot(solvers[l], got[l], False), single[l][1], "LP %d after 170 iterations" % l)
        assert batch.ray_stats()["single_passes"] == 3 * k  # (no figures at 170: both rules of the snapshot take the single pass)
    got = batch.advance()
    st = batch.ray_stats()
    print(k, layout, "at the end:", st, [(g["status_name"], g["steps_taken"]) for g in got])
    # the major iteration at 200 found the batch's pass, not a single one: the count is the snapshots' alone
    assert st["single_passes"] == (3 * k if checkpoints else 0), st
    assert st["wide_passes"] >= max(g["steps_taken"] for g in got) // 40, st  # (at least one K-wide pass per period)
    assert st["members_served"] == sum(g["num_major_iterations"] for g in got), st  # (every major iteration found its figures)
    for l in range(k):
        same_snapshot(snapshot(solvers[l], got[l], True), single[l][-1], "LP %d at the end" % l)
    case.verdicts_are_the_tables(got, list(range(k)))
    assert all(g["steps_taken"] < LIMIT for g in got)
    close_all(batch, solvers)
    return got


@pytest.mark.parametrize("layout", ["panel", "stream"])
@pytest.mark.parametrize("k", [2, 4, 8, 16])
def test_figures_and_trajectories_are_bit_identical_to_single_solves(k, layout, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    got = batch_against_singles("large", k, layout, case.singles("large", layout))
    if k >= 4:  # members end at different steps and rest while the others go on
        assert len({g["steps_taken"] for g in got}) > 1


# ---- 3. tiny blocks: blocks shorter than a workgroup ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 16])
def test_tiny_blocks(k, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "stream")
    batch_against_singles("small", k, "stream", case.singles("small", "stream", False), checkpoints=False)


# ---- 4. the figures against the certificate ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["panel", "stream"])
def test_figures_are_those_of_the_certificate(layout, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    k = 4
    solvers, batch = make_batch("large", list(range(k)), **KW)
    layout_is(solvers[0], layout)
    got = batch.advance(40)
    for l in range(k):
        p = member_lp("large", l)
        dx, dy = solvers[l].ray()
        ref = R.ray_info(p, dx, dy)
        print(layout, l, case.figures(got[l]), ref)
        assert np.any(dx != 0.0) and np.any(dy != 0.0)
        for key in FIGURES:
            assert got[l][key] == pytest.approx(ref[key], rel=1e-10, abs=1e-12), (l, key)
    got = batch.advance()
    for l in range(k):
        if got[l]["status_name"] in RAY_VERDICTS:
            check_verdict(member_lp("large", l), got[l], VERDICT[l], solvers[l])
    assert sum(g["status_name"] in RAY_VERDICTS for g in got) == 2
    close_all(batch, solvers)


# ---- 5. mixed membership, resting members, a second round after resets -------------------------------------------------------------------
def test_mixed_membership_and_a_second_round(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    with_rays = case.singles("large", "panel")
    plain = {k: v for k, v in SINGLE.items() if k != "halpern_infeasibility"}
    without = {}
    for l in (0, 3):  # (freshly created, the option off: their own solves)
        s = capi.Solver(member_lp("large", l), **plain)
        without[l] = state(s, s.advance())
        s.close()
    off = dict(halpern_infeasibility=0)
    solvers, batch = make_batch("large", [0, 1, 2, 3], per_member={0: off, 1: {}, 2: {}, 3: off}, **KW)  # (a clone without settings of its own keeps its parent's)
    got = batch.advance()
    print([(g["status_name"], g["steps_taken"]) for g in got], batch.ray_stats())
    assert [g["status_name"] for g in got] == ["Optimal", "DualInfeasible", "PrimalInfeasible", "Optimal"]
    assert len({g["steps_taken"] for g in got}) > 1  # (the members with a ray verdict rest while the others go on)
    for l in (0, 3):
        same(state(solvers[l], got[l]), without[l], "LP %d, without the detection" % l)
    for l in (1, 2):
        same_snapshot(snapshot(solvers[l], got[l], True), with_rays[l][-1], "LP %d" % l)
    st = batch.ray_stats()
    assert st["members_served"] == got[1]["num_major_iterations"] + got[2]["num_major_iterations"], st
    batch.close()
    # second round: members 1 and 2 swap their bounds (the table refresh, the new verdicts), 0 and 3 start again under their own
    _, bounds = family("large")
    src = [0, 2, 1, 3]
    reset_kw = {k: v for k, v in KW.items() if k != "mode"}  # (a reset with settings replaces them all: the options again)
    for l in range(4):
        kw = dict(reset_kw, halpern_infeasibility=0) if l in (0, 3) else reset_kw
        solvers[l].reset(lb=bounds[src[l]][0], ub=bounds[src[l]][1], **kw)
    batch = capi.SharedMatrixBatch(solvers)
    got = batch.advance()
    print([(g["status_name"], g["steps_taken"]) for g in got], batch.ray_stats())
    assert [g["status_name"] for g in got] == ["Optimal", "PrimalInfeasible", "DualInfeasible", "Optimal"]
    for l in (0, 3):
        same(state(solvers[l], got[l]), without[l], "LP %d, second round" % l)
    for l in (1, 2):
        same_snapshot(snapshot(solvers[l], got[l], True), with_rays[src[l]][-1], "LP %d, second round" % l)
    close_all(batch, solvers)


# ---- 6. the loop adds no synchronisation ---------------------------------------------------------------------------------------------------
def test_the_pass_adds_no_synchronisation(monkeypatch):
    """170 iterations (four major iterations) of K = 4 with halpern_infeasibility on and off, halpern_lockstep_rays on in both: every
    member's loop synchronisations are the same -- the figures ride on the evaluation's read-back -- and with it on they are there"""
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    single = case.singles("large", "panel")
    syncs = {}
    for on in (1, 0):
        solvers, batch = make_batch("large", [0, 1, 2, 3], **dict(KW, halpern_infeasibility=on))
        batch.advance(40)
        got = batch.advance(130)
        syncs[on] = [s.device.loop_stats()["loop_syncs"] for s in solvers]
        st = batch.ray_stats()
        assert st == (dict(wide_passes=4, members_served=16, single_passes=0) if on else dict(wide_passes=0, members_served=0, single_passes=0)), st
        if on:
            for l in range(4):
                assert case.figures(got[l]) == single[l][1][1], l
        close_all(batch, solvers)
    print(syncs)
    assert syncs[1] == syncs[0] and min(syncs[1]) > 0, syncs


# ---- 7. plain launches against graph replay -----------------------------------------------------------------------------------------------
def test_plain_launches_give_the_bits_of_graph_replay(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    batch_against_singles("large", 4, "panel", case.singles("large", "panel"), use_graph=0)


# ---- 8. routing and refusals ---------------------------------------------------------------------------------------------------------------
# The routing rule of docs/design/07_measurement.md, "Halpern mode" (at K = 4 the lockstep median of the call's wall time to 1e-8 must
# beat the sequential median by more than the two spreads combined) keeps the routing on the CSR stream layout -- expected path
# "shared_matrix_halpern" -- and not on the row-sum panels, which keep the clones one after the other under the new field too.
@pytest.mark.parametrize("layout,path", [("stream", "shared_matrix_halpern"), ("panel", "shared_matrix")])
def test_batch_solve_routes_through_the_lockstep_batch(layout, path, monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", layout)
    lps = [member_lp("large", l) for l in range(16)]
    single = case.singles("large", layout)
    together = capi.batch_solve(lps, **KW)
    assert capi.batch_solve_last_path() == path
    without = capi.batch_solve(lps, **{k: v for k, v in KW.items() if k != "halpern_lockstep_rays"})
    assert capi.batch_solve_last_path() == "shared_matrix"  # (as before: one set-up, the clones one after the other)
    for l in range(16):
        want = single[l][-1]
        for out in (together, without):
            for key in KEYS_INT + KEYS_F64 + FIGURES:
                assert out[l][key] == want[0][0][key], (l, key, out[l][key], want[0][0][key])
            for name, v in zip(("x", "y", "reduced_cost"), want[0][1]):
                np.testing.assert_array_equal(out[l][name], v, err_msg="LP %d: %s" % (l, name))
    case.verdicts_are_the_tables(together, list(range(16)))


def test_refusals_and_non_effects(monkeypatch):
    monkeypatch.setenv("CUOPT_AMD_SPMV_LAYOUT", "panel")
    lp, bounds = family("large")
    # the new field on some members only: -7, by name
    no_rays = dict(halpern_lockstep_rays=0)
    with pytest.raises(capi.CuOptError) as e:
        make_batch("large", [0, 1], per_member={1: no_rays}, **KW)
    assert e.value.code == -7 and "halpern_lockstep_rays" in str(e.value), str(e.value)
    # without it on any member: today's refusal, by its own name
    with pytest.raises(capi.CuOptError) as e:
        make_batch("large", [0, 1], **dict(KW, **no_rays))
    assert e.value.code == -7 and "halpern_infeasibility" in str(e.value) and "halpern_lockstep_rays" not in str(e.value), str(e.value)
    # the averaging modes ignore the field; their batch has no ray pass
    out = []
    for extra in (dict(), dict(halpern_lockstep_rays=1, halpern_infeasibility=1)):
        parent = capi.Solver(dict(lp, lb=bounds[0][0], ub=bounds[0][1]), tol=1e-4, iteration_limit=1500, **extra)
        child = parent.clone(lb=bounds[3][0], ub=bounds[3][1])
        batch = capi.SharedMatrixBatch([parent, child])
        got = batch.advance()
        out.append([(got[l], s.solution()) for l, s in enumerate((parent, child))])
        rule = (capi.C.c_int32 * 2)(1, 1)
        rc = capi.lib.pdlpdev_batch_halpern_rays(capi.c_void_p(capi.lib.cuoptamd_batch_device(batch.handle)), rule)
        assert rc == -7 and "Halpern" in capi.lib.pdlpdev_last_error().decode()
        assert batch.ray_stats() == dict(wide_passes=0, members_served=0, single_passes=0)
        close_all(batch, [parent, child])
    for (a, sa), (b, sb) in zip(*out):
        for key in KEYS_INT + KEYS_F64:
            assert a[key] == b[key], (key, a[key], b[key])
        for u, v in zip(sa, sb):
            np.testing.assert_array_equal(u, v)
