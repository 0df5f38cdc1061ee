"""bench.py prints ONE JSON line with the fields the driver's contract names, and its parity sample
(the CPU-baseline leg of --full) agrees with the GPU word for word; a plain run times the headline only and can write
its outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_has_the_contract_fields():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "1", "--warmup", "1", "--batch", "512",
                        "--cpu-seconds", "2"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for key, typ in [("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                     ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str),
                     ("data", str), ("config", dict), ("roofline", dict), ("cpu_baseline", dict)]:
        assert isinstance(d[key], typ), (key, d[key])
    assert d["vs_baseline"] is None and d["n_gpus"] == 1 and d["steps"] == 1 and d["scaling"] == "weak"
    assert d["unit"] == "PBS/s" and d["dtype"] == "f64" and "workload" in d["config"]
    roof = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in roof, key
    # "fp64": the f64 work runs on the VALU, whose peak equals the MFMA-f64 peak (VERDICT r1 asked for the relabel)
    assert roof["bound"] in ("hbm", "mfma", "fp64") and 0.0 < roof["frac"] < 1.0
    # the kernel named is the one that ran: 512 ciphertexts (two per CU) take the two-ciphertext paired shape, not the
    # four-ciphertext throughput kernel
    assert roof["kernel"].startswith("blind_rotate2p2_kernel"), roof["kernel"]
    for leg in ("gate", "cmux", "circuit_bootstrap", "add32", "pcie_inclusive", "device_group", "evaluation_pool"):
        assert isinstance(d.get(leg), dict), (leg, d.get("leg_errors"))
    assert len(r.stdout.strip().splitlines()) == 1, r.stdout[:500]     # nothing else on stdout (librccl's banner goes to stderr)
    grp = d["device_group"]
    assert grp["members"] == 2 and grp["same_words_as_single_context"] is True and grp["key_bytes_replicated_per_member"] > 0
    assert d["pcie_inclusive"]["same_words_as_device_path"] is True
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    # traffic / busy fractions are this run's own rocprofv3 --pmc passes when the profiler is on the box, else the
    # committed passes (attached only for the same kernel and batch — not this batch size — so then traffic is null)
    if roof.get("counters"):
        assert roof["traffic"] == roof["counters"]["hbm_bytes_per_launch"] > 0
        assert 0.0 < roof["counters"]["valu_busy_frac"] < 1.0
    else:
        assert "live_counters" in (d.get("leg_errors") or {}) or roof["traffic"] is None
    cpu = d["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample", "cpus_visible", "cfs_quota_cpus"):
        assert key in cpu, key
    assert cpu["kind"] in ("port", "reference") and cpu["cores"] >= 1 and cpu["value"] > 0
    assert cpu["cores"] <= cpu["cpus_visible"] and (cpu["cfs_quota_cpus"] is None or cpu["cores"] <= cpu["cfs_quota_cpus"] + 1)
    assert cpu["gpu_outputs_bit_equal_on_sample"] is True


@pytest.mark.gpu
def test_single_process_bench_line_over_a_device_group():
    """`bench.py --gpus N --single-process`: the same line shape from ONE host process driving a device group (here two members
    on the one GPU), keys replicated inside the library."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--single-process", "--devices", "0,0",
                        "--full", "--steps", "1", "--warmup", "1", "--batch", "256", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.strip().splitlines()
    assert len(out) == 1, r.stdout[:500]
    d = json.loads(out[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["unit"] == "PBS/s" and d["value"] > 0
    assert d["config"]["devices"] == [0, 0] and d["config"]["global_batch"] == 512
    assert d["rccl"]["members"] == 2 and d["rccl"]["broadcast_bytes"] > 0 and d["rccl"]["world_size"] >= 1
    assert d["pcie_inclusive"]["same_words_as_device_path"] is True
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in d["roofline"], key


@pytest.mark.gpu
def test_plain_bench_line_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """Without --full: --steps timed steps of the headline and nothing else; --dump-outputs writes the last step's GLWE
    ciphertexts as float64 torus values, the same words in two runs with the same arguments."""
    def run(out_dir):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "512",
                            "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        out = r.stdout.strip().splitlines()
        assert len(out) == 1, r.stdout[:500]
        return json.loads(out[0])

    d = run(tmp_path / "a")
    for key, typ in [("metric", str), ("value", float), ("unit", str), ("higher_is_better", bool), ("dtype", str),
                     ("ms_per_step", float)]:
        assert isinstance(d[key], typ), (key, d[key])
    assert d["unit"] == "PBS/s" and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["steps"] == 3 and d["warmup"] == 1 and d["config"]["batch_per_gpu"] == 512
    assert abs(d["value"] * d["ms_per_step"] / 1e3 / 512 - 1.0) < 0.01    # value = 512 bootstraps per ms_per_step
    assert d["cpu_baseline"] is None and d["pcie_inclusive"] is None and d["roofline"]["counters"] is None
    for leg in ("gate", "cmux", "circuit_bootstrap", "pbs_univariate", "add32", "device_group", "evaluation_pool",
                "mul8_gate_pool", "leg_errors"):
        assert leg not in d, leg
    assert sorted(os.listdir(tmp_path / "a")) == ["glwe_out.npy"]
    a = np.load(tmp_path / "a" / "glwe_out.npy")
    assert a.dtype == np.float64 and a.shape == (512, 4096) and a.nbytes <= 64 << 20
    assert np.all(a >= -0.5) and np.all(a < 0.5) and np.count_nonzero(a) > a.size // 2
    run(tmp_path / "b")
    assert np.array_equal(a, np.load(tmp_path / "b" / "glwe_out.npy"))
