"""GPU: row-block sharded SOLVES in reflected-Halpern mode (cuoptamd_settings::halpern_sharded) through capi.Solver and cuOptSolve.

W ranks on one device behind the in-process communicator (host threads, one mode-4 solver each) against the single-GPU mode-4 solve of
the same LP; one rank behind a real RCCL communicator, where the steps are replayed from captured graphs; what stays refused, by name.
eta differs from the single solve's in the last bits of sigma_max (the sharded power iteration adds the partial products in rank
order), so nothing is compared bit for bit with the single solve: the figures are those of tests/test_sharded_gpu.py.

Every case fails on a library without the feature (the -7 refusal of a sharded mode-4 solver, or the missing field)."""
import threading

import numpy as np
import pytest
from conftest import decode_problem, set_tune

from cuopt_amd import capi, synthetic
from test_halpern_reference import RAW, known_objective

pytestmark = pytest.mark.gpu
AFIRO = "afiro"


@pytest.fixture(autouse=True)
def owner_dataflow(monkeypatch):
    monkeypatch.delenv("CUOPT_AMD_SHARD_DATAFLOW", raising=False)  # (the default: owner-computes)
    monkeypatch.delenv("CUOPT_AMD_SHARD_TRANSPORT", raising=False)


def run_sharded(p, world, mode=4, **kw):
    """test_sharded_gpu.run_sharded for a mode-4 solver -> per rank (result, x, y, row range, wire bytes)"""
    cid = capi.softcomm_id(world)
    out, err = [None] * world, []
    if mode == 4:
        kw = dict(kw, halpern_sharded=1)

    def worker(rank):
        try:
            s = capi.Solver(p, mode=mode, rank=rank, world=world, comm_id=cid, **kw)
            assert capi.lib.pdlpdev_shard_dataflow(s.device.handle) == 3
            wire = s.device.wire_bytes()
            r = s.advance()
            x, y, rc = s.solution()
            out[rank] = (r, x, y, s.row_range(), wire)
            s.close()
        except Exception as e:  # surface in the main thread
            err.append(e)
            capi.comm_abort(cid)

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not err, err
    assert all(o is not None for o in out), "a rank did not finish"
    return out


def test_sharded_first_iterations_walk_the_single_solves_path():
    p = synthetic.generate(3000, 3000, 10, seed=4)
    for its in (40, 80):
        one = capi.Solver(p, mode=4, tol=0.0, iteration_limit=its)
        a = one.advance()
        one.close()
        b = run_sharded(p, 4, tol=0.0, iteration_limit=its)[0][0]
        assert (a["steps_taken"], a["num_restarts"], a["num_major_iterations"]) == (b["steps_taken"], b["num_restarts"], b["num_major_iterations"]), (a, b)
        assert a["steps_taken"] == its
        assert b["primal_weight"] == pytest.approx(a["primal_weight"], rel=1e-9)
        assert b["primal_objective"] == pytest.approx(a["primal_objective"], rel=1e-9, abs=1e-9)


_single = {}


def single_solve(p):
    if "r" not in _single:
        s = capi.Solver(p, mode=4, tol=1e-6)
        _single["r"] = s.advance()
        s.close()
    return _single["r"]


@pytest.mark.parametrize("world", [2, 8])
def test_sharded_solve_matches_the_single_solve(world):
    p = synthetic.generate(6000, 5000, 8, seed=61)
    rs = single_solve(p)
    out = run_sharded(p, world, tol=1e-6)
    covered = 0
    for r, x, yl, (r0, r1), _ in out:
        assert (r["status_name"], r["steps_taken"], r["num_restarts"]) == (out[0][0]["status_name"], out[0][0]["steps_taken"], out[0][0]["num_restarts"])
        assert r["primal_objective"] == out[0][0]["primal_objective"]
        np.testing.assert_array_equal(x, out[0][1])
        covered += r1 - r0
    assert covered == p["m"]
    r0 = out[0][0]
    assert r0["status_name"] == rs["status_name"] == "Optimal"
    scale = 1 + abs(p["objective_star"])
    assert abs(r0["primal_objective"] - p["objective_star"]) <= 2e-5 * scale
    assert abs(r0["primal_objective"] - rs["primal_objective"]) <= 2e-5 * scale
    assert r0["relative_gap"] <= 1e-5
    print("STEPS world %d: sharded %d, single %d" % (world, r0["steps_taken"], rs["steps_taken"]))
    assert 0.5 * rs["steps_taken"] - 80 <= r0["steps_taken"] <= 2.0 * rs["steps_taken"] + 80


def test_wire_bytes_are_those_of_a_stable2_rank():
    """the same two vectors and three scalars travel"""
    p = synthetic.generate(3000, 3000, 10, seed=4)
    halpern = [o[4] for o in run_sharded(p, 4, tol=0.0, iteration_limit=1)]
    stable = [o[4] for o in run_sharded(p, 4, mode=1, tol=0.0, iteration_limit=1)]
    assert halpern == stable and halpern[0]["bytes"] > 0, (halpern, stable)


@pytest.mark.parametrize("transport", ["collective", "p2p"])
def test_one_rank_behind_rccl_replays_captured_steps(transport, monkeypatch):
    """a real communicator at world 1: the collectives are captured with the kernels around them (the first step goes out as plain
    launches), the peer transport is kernels only; Optimal at the known objective; a reset and a second advance repeat the first bit for bit"""
    monkeypatch.setenv("CUOPT_AMD_SHARD_TRANSPORT", transport)
    p = synthetic.generate(6000, 5000, 8, seed=61)
    rs = single_solve(p)
    s = capi.Solver(p, mode=4, halpern_sharded=1, tol=1e-6, rank=0, world=1, comm_id=capi.comm_unique_id())
    try:
        assert capi.lib.pdlpdev_shard_dataflow(s.device.handle) == 3
        assert bool(capi.lib.pdlpdev_shard_transport(s.device.handle)) == (transport == "p2p")
        first = s.advance()
        x1, y1, _ = s.solution()
        scale = 1 + abs(p["objective_star"])
        assert first["status_name"] == "Optimal" and abs(first["primal_objective"] - p["objective_star"]) <= 2e-5 * scale
        assert abs(first["primal_objective"] - rs["primal_objective"]) <= 2e-5 * scale and first["relative_gap"] <= 1e-5
        s.reset()
        second = s.advance()
        x2, y2, _ = s.solution()
        assert (second["steps_taken"], second["num_restarts"], second["primal_objective"]) == (first["steps_taken"], first["num_restarts"], first["primal_objective"])
        np.testing.assert_array_equal(x1, x2)
        np.testing.assert_array_equal(y1, y2)
    finally:
        s.close()


def test_what_stays_refused_is_refused_by_name(monkeypatch):
    p = decode_problem(RAW[AFIRO])
    monkeypatch.setenv("CUOPT_AMD_SMALL", "0")
    # without the setting: the refusals tests/test_halpern_gpu.py pins
    with pytest.raises(capi.CuOptError) as e:
        capi.Solver(p, mode=4, rank=0, world=2, comm_id=capi.softcomm_id(2))
    assert e.value.code == -7 and "Halpern" in str(e.value)
    r = capi.solve(p, method=1, pdlp_solver_mode=4, amd_num_gpus=2)
    assert r["return_code"] == capi.CUOPT_VALIDATION_ERROR and "Halpern" in r["error_string"]
    # with it: the other dataflows, by name
    for flow in ("rsag", "allreduce"):
        monkeypatch.setenv("CUOPT_AMD_SHARD_DATAFLOW", flow)
        with pytest.raises(capi.CuOptError) as e:
            capi.Solver(p, mode=4, halpern_sharded=1, rank=0, world=1, comm_id=capi.softcomm_id(1))
        assert e.value.code == -7 and "Halpern" in str(e.value) and flow in str(e.value) and "dataflow" in str(e.value).lower()
    monkeypatch.delenv("CUOPT_AMD_SHARD_DATAFLOW")
    for kw in (dict(halpern_infeasibility=1), dict(halpern_resident=1), dict(halpern_batch=1)):
        with pytest.raises(capi.CuOptError) as e:
            capi.Solver(p, mode=4, halpern_sharded=1, rank=0, world=1, comm_id=capi.softcomm_id(1), **kw)
        assert e.value.code == -7 and "halpern_sharded" in str(e.value) and list(kw)[0] in str(e.value)
    for kw in (dict(amd_halpern_infeasibility=1), dict(amd_halpern_resident=1), dict(amd_halpern_batch=1)):
        # (cuoptamd_solve_sharded refuses before it counts devices or spawns a rank: a validation error on a box of any size)
        r = capi.solve(p, method=1, pdlp_solver_mode=4, amd_halpern_sharded=1, amd_num_gpus=2, **kw)
        assert r["return_code"] == capi.CUOPT_VALIDATION_ERROR and list(kw)[0][4:] in r["error_string"] and "halpern_sharded" in r["error_string"], r["error_string"]
    s = capi.Solver(p, mode=4, halpern_sharded=1, rank=0, world=1, comm_id=capi.softcomm_id(1))
    try:
        for kw in (dict(halpern_sharded=1, halpern_infeasibility=1), dict(halpern_sharded=1, halpern_resident=1)):
            with pytest.raises(capi.CuOptError) as e:  # a refused reset leaves the solver as it was
                s.reset(**kw)
            assert e.value.code == -7 and "halpern_sharded" in str(e.value)
        first = s.advance()
        assert first["status_name"] == "Optimal"
        assert abs(first["primal_objective"] - known_objective(AFIRO)) <= 1e-3 * (1 + abs(known_objective(AFIRO)))
        with pytest.raises(capi.CuOptError) as e:
            s.get_warm_start()
        assert e.value.code == -7 and "halpern_sharded" in str(e.value)
        with pytest.raises(capi.CuOptError) as e:
            capi.SharedMatrixBatch([s, s])
        assert e.value.code == -7 and "halpern_sharded" in str(e.value)
    finally:
        s.close()


def test_cuoptsolve_shards_a_halpern_solve(monkeypatch):
    """cuOptSolve with amd_num_gpus = 2: on the in-process communicator (two ranks on one device) it solves afiro to the golden objective
    and the solve info says so; with real devices asked for and only one visible it answers the runtime error about GPUs, not the
    mode's validation error"""
    p = decode_problem(RAW[AFIRO])
    want = known_objective(AFIRO)
    set_tune(monkeypatch, soft_communicator=1)
    r = capi.solve(p, method=1, pdlp_solver_mode=4, amd_halpern_sharded=1, amd_num_gpus=2)
    assert r["return_code"] == capi.CUOPT_SUCCESS and r["status"] == "Optimal" and r["gpus"] == 2, (r["return_code"], r.get("error_string"))
    assert abs(r["objective"] - want) <= 1e-3 * (1 + abs(want)), (r["objective"], want)
    assert r["solve_info"]["halpern_sharded"] == 1 and r["solve_info"]["pdlp_algorithm"] == "reflected_halpern"
    set_tune(monkeypatch, soft_communicator=None)
    if capi.device_count() < 2:
        r = capi.solve(p, method=1, pdlp_solver_mode=4, amd_halpern_sharded=1, amd_num_gpus=2)
        assert r["return_code"] == capi.CUOPT_RUNTIME_ERROR and "GPUs requested" in r["error_string"] and "visible" in r["error_string"], r["error_string"]


@pytest.mark.parametrize("transport", ["collective", "p2p"])
def test_rccl_two_ranks_in_one_process(transport, monkeypatch):
    """two devices, two host threads, real RCCL (or the direct peer stores), in the style of test_method_and_multigpu_gpu's case"""
    if capi.device_count() < 2:
        pytest.skip("needs two visible devices")
    set_tune(monkeypatch, soft_communicator=None)
    monkeypatch.setenv("CUOPT_AMD_SHARD_TRANSPORT", transport)
    p = synthetic.generate(6000, 5000, 8, seed=61)
    single = capi.solve(p, method=1, pdlp_solver_mode=4, tol=1e-6)
    r = capi.solve(p, method=1, pdlp_solver_mode=4, amd_halpern_sharded=1, tol=1e-6, amd_num_gpus=2)
    assert r["status"] == "Optimal" and r["gpus"] == 2 and r["solve_info"]["halpern_sharded"] == 1
    assert abs(r["objective"] - single["objective"]) <= 2e-5 * (1 + abs(single["objective"]))
