"""bench.py: the algorithmic work it prices the step with and, on the GPU, the
one-line JSON contract: the headline of a plain run (and its --dump-outputs files), and with --full
the roofline with the dominant kernel, the probes and the distributed fields."""
import importlib.util
import json
import math
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("pis_bench", os.path.join(HERE, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("size,gflop", [(256, 272.4), (512, 1089.5), (1024, 4357.9)])
def test_conv_flops_per_image(size, gflop):
    """2 x MACs x 3 over every conv / convT minus enc1.conv0's input gradient."""
    assert abs(_bench().conv_flops_per_image(size, size) / 1e9 - gflop) < 0.1


@pytest.mark.gpu
def test_bench_json_contract():
    out = subprocess.run([sys.executable, os.path.join(HERE, "bench.py"), "--full", "--steps", "2", "--warmup", "1",
                          "--no-cpu-baseline"], capture_output=True, text=True, timeout=110, cwd=HERE)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["scaling"] == "weak" and d["higher_is_better"] is True
    assert abs(d["value"] - 8 * 1000.0 / d["ms_per_step"]) < 1e-6 * d["value"]  # B = 8 images per step
    assert d["dtype"].startswith("fp32")
    assert math.isfinite(d["final_loss"]) and 0.0 < d["final_loss"] < 10.0  # the timed steps trained
    # "roofline" is the dominant one of the two conv kernels (the most GPU time per step); both are
    # reported, each against its own bound, with per-launch shapes matching the hook's launch counts
    assert d["roofline"] is d[d["roofline_dominant"]] or d["roofline"] == d[d["roofline_dominant"]]
    direct = ("roofline_direct_fwd", "roofline_direct_pool", "roofline_direct_dgrad", "roofline_direct_wgrad")
    for name, bound, unit in (("roofline_gemm", "mfma", "TFLOP/s"), ("roofline_fused", "hbm", "GB/s"),
                              *((k, "mfma", "TFLOP/s") for k in direct)):
        r = d.get(name)
        assert r is not None, name  # (the launch tables leave the direct layers out: the fused
        # kernel's two C2 launches are priced again)
        assert r["bound"] == bound and r["unit"] == unit and 0 < r["frac"] < 1
        assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
        assert r["launches_per_step"] > 0 and r["avg_launch_ms"] > 0 and r["ms_per_step"] > 0
        if name in direct:  # per-role algorithmic bytes: the layer table reproduces the hook's launches
            assert r["algorithmic_bytes_per_launch"] and 0 < r["hbm_frac"] < 1, name
    assert d["roofline_gemm"]["hbm_view"] is not None
    # the box's streaming rate beside the HBM rooflines, and each HBM roofline against it
    hp = d["hbm_probe"]
    assert hp["unit"] == "GB/s" and 2000 < hp["achieved"] < 8000 and abs(hp["frac_of_8tbs"] - hp["achieved"] / 8000) < 1e-9
    for r in (d["roofline_fused"], d["roofline_loss"]["head_loss_fwd_kernel_live"]):
        assert abs(r["frac_of_hbm_probe"] - r["achieved"] / hp["achieved"]) < 1e-9
    assert d["roofline"]["ms_per_step"] == max(d[k]["ms_per_step"] for k in
                                               ("roofline_gemm", "roofline_fused") + direct if d.get(k))


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """Without --full the line carries the headline only (no roofline, probe or baseline ran), --steps
    is the number of timed steps, and --dump-outputs writes the last step's arrays as float32 / float64
    .npy files of at most 64 MB in all."""
    import numpy as np
    dump = tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(HERE, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup",
                          "1", "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=110, cwd=HERE)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "final_loss"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "images/s" and d["dtype"].startswith("fp32") and d["ms_per_step"] > 0
    assert abs(d["value"] - 8 * 1000.0 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert d["roofline"] is None
    assert not [k for k in d if k.startswith("roofline_") or k in ("cpu_baseline", "hbm_probe", "distributed")]
    arrays = {p.stem: np.load(p) for p in dump.iterdir()}
    assert sorted(arrays) == ["grads_sample", "loss", "params_sample", "u"]
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert sum(p.stat().st_size for p in dump.iterdir()) <= 64 << 20
    assert arrays["u"].shape == (8, 1, 512, 512) and 0.0 <= arrays["u"].min() and arrays["u"].max() <= 1.0
    assert float(arrays["loss"]) == pytest.approx(d["final_loss"], rel=1e-6)
    assert np.abs(arrays["grads_sample"]).max() > 0 and np.abs(arrays["params_sample"]).max() > 0


def test_bench_inputs_are_the_same_every_run():
    """The batch depends on nothing but its fixed seed (and the rank)."""
    import torch
    b = _bench()
    b.H = b.W = 64
    x0, t0 = b.make_batch(0, "cpu")
    x1, t1 = b.make_batch(0, "cpu")
    assert torch.equal(x0, x1) and torch.equal(t0, t1) and x0.shape == (8, 1, 64, 64)


@pytest.mark.gpu
def test_bench_launches_n_ranks():
    """`bench.py --gpus 2` without a torchrun environment starts its own two ranks (here both on
    the one GPU over gloo: RCCL needs a GPU per rank) and reports the whole job."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(HERE, "bench.py"), "--full", "--gpus", "2", "--backend", "gloo",
                          "--steps", "2", "--warmup", "1", "--no-cpu-baseline"],
                         capture_output=True, text=True, timeout=110, cwd=HERE, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 16
    assert abs(d["value"] - 16 * 1000.0 / d["ms_per_step"]) < 1e-6 * d["value"]  # 2 ranks x 8 images
    assert "cpu_baseline" not in d
    # what the process group formed and the all-reduce time the backward left exposed, per rank
    dd = d["distributed"]
    assert dd["backend"] == "gloo" and dd["world_size_formed"] == 2 and dd["buckets"] >= 2
    ex = dd["exposed_allreduce_ms"]
    assert ex["steps"] == 2 and len(ex["mean_per_rank"]) == 2
    assert all(v >= 0.0 for v in ex["mean_per_rank"])
    assert ex["max_over_ranks"] == max(ex["mean_per_rank"]) and ex["worst_step_max_over_ranks"] >= ex["max_over_ranks"]
    # each rank's own step time (straggling): the line's ms_per_step is their maximum
    rm = d["ms_per_step_by_rank"]
    assert len(rm["per_rank"]) == 2 and all(v > 0 for v in rm["per_rank"])
    assert rm["min"] == min(rm["per_rank"]) and rm["max"] == max(rm["per_rank"])
    assert abs(rm["max"] - d["ms_per_step"]) <= 1e-9 * d["ms_per_step"]


@pytest.mark.gpu
def test_bench_other_config_reports_no_c2_counters():
    """A --config other than C2 must not carry C2's committed PMC counters as its own (VERDICT r5
    weak #11): traffic / MFMA-busy fields are null and the line says why."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "bench.py"), "--full", "--config", "c4-rd", "--steps", "2",
                          "--warmup", "1", "--no-cpu-baseline"], capture_output=True, text=True, timeout=110, cwd=HERE)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert "C2 only" in d["pmc_note"]
    g = d["roofline_gemm"]
    assert g["traffic"] is None and g["mfma_busy_frac"] is None and g["mfma_busy_by_kernel"] is None
    for k in ("roofline_fused", "roofline_direct_fwd", "roofline_direct_wgrad"):
        if d.get(k):
            assert d[k]["traffic"] is None, k
    assert d["roofline_loss"]["head_loss_fwd_kernel_live"]["traffic"] is None


def test_pmc_fields_only_for_the_profiled_config():
    """profiles/pmc_dominant.json holds C2's counters: read for C2, None for every other config."""
    b = _bench()
    assert b.PMC_CONFIG == "c2"
    for cfg in ("c4-rd", "c5"):
        assert b.load_pmc(b.DOMINANT_KERNEL, cfg) == (None, None, None)
        assert b.pmc_bytes("gemm_nt_h3_", cfg) is None
    traffic, busy, by_kernel = b.load_pmc("gemm_nt_h3_", "c2")
    assert traffic and 0 < busy < 1 and by_kernel
    assert b.pmc_bytes("gemm_nt_h3_", "c2") > 0


def test_bench_rejects_world_mismatch():
    """A rank whose WORLD_SIZE disagrees with --gpus exits non-zero before touching the GPU."""
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    out = subprocess.run([sys.executable, os.path.join(HERE, "bench.py"), "--gpus", "4", "--steps", "1"],
                         capture_output=True, text=True, timeout=300, cwd=HERE, env=env)
    assert out.returncode == 2 and "WORLD_SIZE=2 but --gpus 4" in out.stderr


def test_host_cpus_reports_quota():
    n, info = _bench().host_cpus()
    assert 1 <= n <= info["affinity_cpus"]
    if info["cgroup_quota_cpus"]:
        assert n <= info["cgroup_quota_cpus"]
