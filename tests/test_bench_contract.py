"""bench.py without a GPU: the module imports, its expectations come from the oracle fixture (28 levels, 319 228 361 states), the flags of
the driver's contract parse, the CPU-baseline leg runs the oracle and reports the cores it used, and without a HIP device the bench fails
loudly instead of falling back to anything."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_expectations_come_from_the_oracle_fixture():
    sys.path.insert(0, ROOT)
    import bench
    E = bench.EXPECT
    assert (E["distinct"], E["depth"], len(E["levels"])) == (319228361, 28, 28) and E["fixture"].startswith("oracle_levels_config2")
    assert E["checksums"] and E["viol_fp"] == int("8f264756864213e1", 16)
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        base = json.load(f)
    assert "distinct states/sec" in base["metric"]


def test_flags_of_the_contract_parse():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--workload", "--no-config3", "--no-cpu-baseline", "--full", "--dump-outputs"):
        assert flag in r.stdout


def test_cpu_baseline_leg_and_loud_failure_without_a_gpu():
    sys.path.insert(0, ROOT)
    import bench
    cb = bench.cpu_baseline(1.5)
    assert cb["kind"] == "port" and cb["unit"] == "distinct states/s" and cb["value"] > 1e4 and 1 <= cb["cores"] <= (os.cpu_count() or 1)
    assert "oracle/vsr_oracle_mt" in cb["sample"]
    import vsr_tlaplus_amd as vt
    if vt.load().vsrmc_device_count() == 0:                       # this container: the product path must refuse, not fall back
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-config3"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and not any(l.startswith("{") for l in r.stdout.splitlines()), r.stdout[-500:]


def test_dumped_outputs_are_exact_float64(tmp_path):
    """--dump-outputs: 64-bit fingerprints and record words survive as two exact 32-bit halves, every array is written as float64."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    big = (1 << 64) - 3
    row = dict(level=2, n_new=5, generated=9, deadlocks=1, max_bag=3, viol_mask=0, act_generated=list(range(16)), fp_xor=big, fp_sum=7)
    rows = [(row, "level"), (row, "deep"), (dict(row, n_new=0, viol_mask=1), "probe")]
    tr = [("Initial predicate", np.array([1, big], dtype=np.uint64)), ("SendDVC", np.array([1 << 40], dtype=np.uint64))]
    out = bench.run_outputs(rows, tr, 100, 3, big)
    bench.dump_outputs(out, str(tmp_path))
    got = {n: np.load(str(tmp_path / (n + ".npy"))) for n in out}
    assert all(a.dtype == np.float64 for a in got.values())
    w = got["trace_words"]
    assert [int(h) << 32 | int(lo) for h, lo in w] == [1, big, 1 << 40] and list(got["trace_offsets"]) == [0, 2, 3]
    assert list(got["trace_actions"]) == [0, 4]
    assert list(got["fp_checksums"][1]) == [big >> 32, big & 0xFFFFFFFF, 0, 7] and not got["fp_checksums"][0].any()
    assert list(got["levels"][2]) == [2, 0, 9, 0, 0, 1] and got["act_generated"].shape == (3, 15)
    assert int(got["summary"][3]) << 32 | int(got["summary"][4]) == big
