"""bench.py as the driver starts it: `python3 bench.py --gpus N` with no launcher must put N ranks on the job by itself (children
started before the parent touches the GPU) and say so in its line; with a launcher's environment it runs as one of the ranks."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--pairs", "20000", "--alleles", "16", "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--ont-sample", "0",
         "--many-alleles-sample", "0", "--recruit-sample", "0", "--map-sample", "0", "--recovery-sample", "0", "--ont-stream-sample", "0", "--ont-whole-path-sample", "0", "--exact-sample", "0"]


def run_bench(extra, env_drop=("WORLD_SIZE", "RANK", "LOCAL_RANK")):
    env = {k: v for k, v in os.environ.items() if k not in env_drop}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, capture_output=True, text=True, env=env, timeout=1500)


def test_self_launch_without_a_gpu_fails_loudly():
    """CPU tier: the parent starts its two children, they find no device, the parent exits non-zero and prints no line."""
    from locityper_amd import api
    if api.device_count() > 0:
        pytest.skip("a GPU is visible: the launch is covered by the gpu-marked test below")
    r = run_bench(["--gpus", "2"])
    assert r.returncode != 0 and r.stdout.strip() == "" and "child ranks exited" in r.stderr


@pytest.mark.gpu
def test_self_launch_reports_the_ranks_it_started():
    from locityper_amd import api
    ndev = api.device_count()
    over = [] if ndev >= 2 else ["--oversubscribe"]
    r = run_bench(["--gpus", "2"] + over)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["launch"].startswith("self-spawned") and out["devices_used"] == min(2, ndev)
    assert out["solver"]["all_calls_equal_truth"] is True
    # more ranks than devices without the explicit flag: refused, non-zero, no line
    if ndev < 2:
        r2 = run_bench(["--gpus", "2"])
        assert r2.returncode != 0 and r2.stdout.strip() == ""
    # one rank: the plain single-process form
    r1 = run_bench(["--gpus", "1"])
    assert r1.returncode == 0, r1.stderr[-3000:]
    o1 = json.loads(r1.stdout.strip().splitlines()[-1])
    assert o1["n_gpus"] == 1 and o1["launch"] == "single process" and o1["rccl_ranks"] is None


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["--shard-reads", "--shard-chains"])
def test_one_locus_sharded_over_the_ranks_through_the_whole_path(mode):
    """BASELINE configs[4]'s form (`--shard-reads`: the reads of ONE locus over the ranks — run_filter scores all-reduced, location-table
    rows all-gathered per solver stage, chains dealt to the ranks) and the chain-sharded form, solver on, through the launch path of the
    driver. RCCL refuses two ranks on one device, so a one-GPU box runs the communicator with one rank; two devices run two."""
    from locityper_amd import api
    n = 2 if api.device_count() >= 2 else 1
    r = run_bench(["--gpus", str(n), mode])
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["n_gpus"] == n and out["rccl_ranks"] == n and out["scaling"] == "strong"
    assert out["solver"] is not None and tuple(out["called_genotype"]) == tuple(out["true_genotype"])
    # call by call, the timed steps give the per-stage figures themselves: a plain line carries them
    assert out["reads_scored_per_s"] > 0 and out["solver"]["call_by_call_stage_ms"]["score_prefilter"] > 0
    if n > 1:
        assert out["ms_per_step_ranks"]["min"] <= out["ms_per_step_ranks"]["max"] == pytest.approx(out["ms_per_step"])


@pytest.mark.gpu
def test_plain_line_full_line_and_the_dumped_outputs(tmp_path):
    """A plain run prints the headline alone; --dump-outputs writes the call of the last timed step as float64 arrays; --full adds the
    figures beside the timed region. The same arguments give the same inputs, so both runs dump the same call."""
    import numpy as np
    plain, full = tmp_path / "plain", tmp_path / "full"
    r = run_bench(["--gpus", "1", "--dump-outputs", str(plain)])
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["full"] is False and out["steps"] == 2 and out["ms_per_step"] > 0 and out["dtype"] == "f64"
    assert "roofline_all" not in out and "distinct_loci_queue" not in out and "per_step" not in out["solver"]
    arrays = {p.name: np.load(p) for p in plain.glob("*.npy")}
    assert {"call_ixs.npy", "call_genotypes.npy", "call_ln_probs.npy", "call_quality.npy"} <= set(arrays)
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert tuple(arrays["call_genotypes.npy"][0]) == tuple(out["called_genotype"]) == tuple(out["true_genotype"])
    assert arrays["call_quality.npy"][0] == out["solver"]["quality"]
    r = run_bench(["--gpus", "1", "--full", "--dump-outputs", str(full)])
    assert r.returncode == 0, r.stderr[-3000:]
    out_full = json.loads(r.stdout.strip().splitlines()[-1])
    assert out_full["full"] is True and "roofline_all" in out_full and "call_by_call_stage_ms" in out_full["solver"]
    assert "distinct_loci_queue" in out_full and out_full["distinct_loci_queue"]["all_calls_equal_truth"] is True
    assert sorted(p.name for p in full.glob("*.npy")) == sorted(arrays)
    for name, a in arrays.items():
        np.testing.assert_allclose(np.load(full / name), a, rtol=1e-12, atol=0, err_msg=name)
