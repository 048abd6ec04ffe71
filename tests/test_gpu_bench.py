"""bench.py as a program on the GPU box: the N = 1 line's contract fields, the plain (lean) line and its --dump-outputs, and the
self-launched N = 2 run over the host-staged transport (two processes share the one GPU) with its self-check against a single-rank
replay of the same iterations (--full)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]                      # ONE JSON line
    return json.loads(lines[0])


def test_single_gpu_line_has_the_contract_fields():
    rec = _run("--full", "--grid", "128", "--steps", "20", "--warmup", "5", "--no-extras", "--cpu-iters", "1")
    assert rec["n_gpus"] == 1 and rec["steps"] == 20 and rec["warmup"] == 5 and rec["unit"] == "iterations/s" and rec["dtype"] == "f64"
    assert rec["higher_is_better"] is True and rec["data"] == "synthetic" and rec["vs_baseline"] is None and "workload" in rec["config"]
    assert abs(rec["value"] - 1e3 / rec["ms_per_step"]) <= 1e-6 * rec["value"]
    rf = rec["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert rf["launches_timed"] == 20 and rf["algorithmic_bytes_per_launch"] == 12 * rec["config"]["nnz"] + 4 * (rec["config"]["rows"] + 1) + 16 * rec["config"]["rows"]
    cb = rec["cpu_baseline"]
    assert cb["cores"] == 1 and cb["kind"] == "port" and cb["value"] > 0 and "sample" in cb
    # the HIP loop against the oracle on the same iterations of the same full-size system, in the line itself (north star: 1e-10)
    # (against the oracle with exactly summed dot products: 1e-10; against the reference's serial order: within that order's own rounding)
    assert cb["gpu_vs_compensated_oracle_relative_difference"] <= 1e-10 and cb["gpu_within_reference_rounding"] is True, cb
    # ... and in the validation mode (dot_order = 1) the same iterations give the oracle's residual bit for bit
    assert cb["gpu_equals_oracle_in_reference_order_mode"] is True and cb["gpu_residual_in_reference_order_mode"] == cb["residual"], cb
    assert rf["traffic"] is None or "RECORDED" in rf["traffic_source"]


def _dumped(d):
    x, res = np.load(d / "x.npy"), np.load(d / "residual_after_steps.npy")
    assert x.dtype == np.float64 and res.dtype == np.float64 and res.shape == (1,)
    return x, res


def _check_against_oracle(x, residual, n, iterations):
    """x and the residual norm after `iterations` CG iterations from x0 = 0 on the 7-point n^3 system, b = 1, against the CPU oracle
    (north star: 1e-10 relative; the loops differ only in the order of the dot products' sums)."""
    from oracle import oracle as O

    e, c, r = O.poisson_csr(n, n, n)
    xr, rr = np.zeros(n**3), C.c_double(0)
    O.lib().oracle_cg_steps(e, c, r, n**3, xr, np.ones(n**3), iterations, C.byref(rr), np.empty(3 * n**3))
    assert np.abs(x - xr).max() <= 1e-10 * np.abs(xr).max()
    assert abs(residual - rr.value) <= 1e-10 * rr.value, (residual, rr.value)


def test_plain_line_is_lean_and_dumps_what_the_timed_steps_computed(tmp_path):
    """Without --full the line carries the headline and the in-loop roofline, and none of the objects that take work of their own;
    --dump-outputs writes the iterate after the warm-up and the timed steps (all of x at this size) and the residual of the last step."""
    n, steps, warmup = 24, 9, 3
    rec = _run("--grid", str(n), "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "out"))
    assert rec["steps"] == steps and rec["warmup"] == warmup and rec["unit"] == "iterations/s" and rec["dtype"] == "f64" and rec["higher_is_better"] is True
    assert abs(rec["value"] - 1e3 / rec["ms_per_step"]) <= 1e-6 * rec["value"] and rec["roofline"]["launches_timed"] == steps
    for k in ("cpu_baseline", "roofline_csr_spmv", "lossless_forms", "mgcg"):
        assert k not in rec, k
    x, res = _dumped(tmp_path / "out")
    assert sorted(os.listdir(tmp_path / "out")) == ["residual_after_steps.npy", "x.npy"]
    assert x.shape == (n**3,) and res[0] == rec["residual_after_steps"]
    _check_against_oracle(x, res[0], n, warmup + steps)


@pytest.mark.parametrize("solver", ["cg", "mgcg"])
def test_two_self_launched_ranks_check_themselves_against_one_rank(solver, tmp_path):
    rec = _run("--full", "--gpus", "2", "--grid", "64", "--steps", "8", "--warmup", "2", "--allow-fallback", "--solver", solver,
               "--dump-outputs", str(tmp_path / "out"))
    assert rec["n_gpus"] == 2 and rec["scaling"] == "strong"
    if "rccl" not in rec["config"]["transport"].lower() or "fallback" in rec["config"]["transport"].lower():
        assert "not a scaling result" in rec["config"]["transport"]             # one GPU: the host-staged transport, and the line says so
    par = rec["parity_vs_single_rank"]
    assert par["within_1e-10"] is True and par["relative_difference"] <= 1e-10, par
    assert par["partitioned_residual_after_steps"] == rec["residual_after_steps"]
    pr = rec["per_rank"]
    assert len(pr["seconds_for_the_timed_steps"]) == 2 and len(pr["spmv_avg_launch_ms"]) == 2
    assert abs(max(pr["seconds_for_the_timed_steps"]) - rec["ms_per_step"] * rec["steps"] / 1e3) <= 1e-9       # the line reports the slowest rank
    assert par["single_rank_ms_per_step"] > 0 and par["speedup_vs_single_rank"] > 0
    # --dump-outputs gathers x over the ranks: all 64^3 entries, and the residual the line reports
    x, res = _dumped(tmp_path / "out")
    assert x.shape == (64**3,) and res[0] == rec["residual_after_steps"]
    if solver == "cg":
        _check_multirank_extras(rec, 2)
        _check_against_oracle(x, res[0], 64, 2 + 8)


def _check_multirank_extras(rec, world):
    """The N > 1 line of the driver's command explains itself: config 4 (row-partitioned MGCG) with its own self-check and 1-GPU leg,
    the communicator's prices, the three halo schedules next to the library's choice (Mgcg/cuBlas/Mgcg/MgcgMain.cs:143-167 times the
    1-GPU and N-GPU legs in one run; ConjugateGradientParallelGpu.cs:384-419,463,499,525 are the steps priced)."""
    assert "extras_aborted" not in rec, rec.get("extras_aborted")
    cp = rec["comm_probe"]
    for k in ("allreduce_8B_us", "allreduce_16B_us", "fork_join_us", "kernel_boundary_us"):
        assert cp[k] is not None and cp[k] >= 0, (k, cp)
    for k in ("neighbour_exchange_one_plane_us", "neighbour_exchange_8B_us"):      # timed on RCCL only: a host-staged transport reports null, never a near-zero figure
        assert (cp[k] is not None and cp[k] > 0) if cp["transport"] == "rccl" else cp[k] is None, (k, cp)
    assert cp["fork_join_us"] > 0 and cp["kernel_boundary_us"] > 0 and cp["plane_bytes"] == 8 * round(rec["config"]["rows"] ** (1 / 3)) ** 2
    sc = rec["schedules"]
    for k in ("exchange_in_line", "interior_rows_on_side_stream", "exchange_on_side_stream", "library_default"):
        assert sc[k]["ms_per_iteration"] > 0, (k, sc)
    assert sc["exchange_in_line"]["overlap_active_rank0"] is False and sc["interior_rows_on_side_stream"]["overlap_active_rank0"] is True
    mg = rec["mgcg"]
    assert mg["ms_per_iteration"] > 0 and mg["iterations_to_1e-8"] > 0 and mg["solve_s"] > 0
    par = mg["parity_vs_single_rank"]
    assert par["within_1e-10"] is True and par["same_iterations_to_1e-8"] is True, par
    assert mg["single_rank"]["iterations_to_1e-8"] == mg["iterations_to_1e-8"]
    assert mg["speedup_vs_single_rank"]["solver_time"] > 0 and mg["speedup_vs_single_rank"]["per_iteration"] > 0
    for k in ("exchange_in_line", "interior_rows_on_side_stream", "exchange_on_side_stream", "library_default", "per_pass_exchanges"):
        assert mg["schedules"][k]["ms_per_iteration"] > 0, (k, mg["schedules"])
    # the deep-halo cycle (bit 2 of the folds) is the default wherever the slabs are thick enough; the per-pass schedule never has it
    assert not mg["schedules"]["per_pass_exchanges"]["folds_rank0"] & 4
    planes = round(rec["config"]["rows"] ** (1 / 3)) // world
    assert bool(mg["folds_rank0"] & 4) == (planes // 2 >= 2 and planes // 4 >= 4 and os.environ.get("MGCG_DEEP_HALO", "1") != "0"), (mg["folds_rank0"], planes)


@pytest.mark.parametrize("solver", ["cg", "mgcg"])
def test_two_ranks_over_rccl_when_the_box_has_two_devices(solver):
    """The same self-launched run WITHOUT --allow-fallback: two ranks on two devices form a real RCCL communicator (the one step no
    one-GPU box can take), and the line's self-check says whether the partitioned loop computed what one rank computes.  Skipped on a
    box with one device."""
    from conjugategradient_amd import _lib

    if _lib.lib().GetDeviceCount() < 2 or os.environ.get("MGCG_VIRTUAL_DEVICES"):
        pytest.skip("needs two physical devices")
    rec = _run("--full", "--gpus", "2", "--grid", "128", "--steps", "10", "--warmup", "3", "--solver", solver)
    assert rec["n_gpus"] == 2 and rec["config"]["transport"] == "rccl"
    par = rec["parity_vs_single_rank"]
    assert par["within_1e-10"] is True, par
    if solver == "cg":
        _check_multirank_extras(rec, 2)
        assert rec["comm_probe"]["transport"] == "rccl" and rec["comm_probe"]["allreduce_8B_us"] > 0 and rec["comm_probe"]["neighbour_exchange_one_plane_us"] > 0
