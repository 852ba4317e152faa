"""bench.py on the GPU, each run a fresh child process: a plain run measures the timed steps only and --dump-outputs writes
what the last timed step computed (float32 .npy, identical inputs from run to run); --full adds the per-kernel figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 256
DUMPED = ("params", "state", "grads", "adam_m", "adam_v", "stats", "features")


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + [str(a) for a in args],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def load_dump(d):
    out = {}
    for name in DUMPED:
        a = np.load(os.path.join(d, name + ".npy"))
        assert a.dtype == np.float32, (name, a.dtype)
        assert np.all(np.isfinite(a)), name
        out[name] = a
    return out


def synthetic_waveforms():
    # bench.py sets a GPU_MAX_HW_QUEUES default at import; this process does not keep it
    saved = os.environ.get("GPU_MAX_HW_QUEUES")
    import bench
    if saved is None:
        os.environ.pop("GPU_MAX_HW_QUEUES", None)
    else:
        os.environ["GPU_MAX_HW_QUEUES"] = saved
    return bench.synthetic_batch(B, 0, bench.N_CLASSES)[0]


def test_plain_run_dumps_the_last_step(tmp_path):
    d1, d2 = tmp_path / "a", tmp_path / "b"
    out = run_bench("--steps", 3, "--warmup", 1, "--batch", B, "--dump-outputs", d1)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "clips/s" and out["dtype"] == "f32"
    assert out["roofline"] is None and out["extra"] is None and out["cpu_baseline"] is None and out["kernel_ms_per_step"] == {}
    a = load_dump(d1)
    assert a["features"].shape == (B, 30, 20)
    assert a["params"].size == a["grads"].size == a["adam_m"].size == a["adam_v"].size
    assert abs(float(a["stats"][0]) / B - out["config"]["final_loss"]) < 1e-3
    assert np.abs(a["grads"]).max() > 0 and np.abs(a["adam_v"]).max() > 0
    # the features are those of bench.py's seeded synthetic batch (the last step featurizes the same waveforms as every step)
    from oracle import featurizer_oracle as fo
    want = fo.featurize_batch(synthetic_waveforms())
    assert float(np.abs(a["features"] - want).max()) < 1e-3
    # same arguments -> same outputs: the features bit for bit, the rest up to the order of the step's atomic sums (the last
    # timed step starts from the run's seeded starting point, so the trajectory of the steps before it does not matter)
    run_bench("--steps", 3, "--warmup", 1, "--batch", B, "--dump-outputs", d2)
    b = load_dump(d2)
    np.testing.assert_array_equal(a["features"], b["features"])
    for name in DUMPED:
        err = float(np.abs(a[name] - b[name]).max())
        assert err <= 1e-4 * float(np.abs(a[name]).max()), (name, err)


def test_full_run_adds_the_per_kernel_figures():
    out = run_bench("--full", "--no-extra", "--no-cpu-baseline", "--profile-steps", 2, "--steps", 3, "--warmup", 1, "--batch", B)
    assert out["full"] is True and out["steps"] == 3
    assert out["roofline"]["kernel"] in out["kernel_ms_per_step"] and out["kernel_ms_per_step_serial"]
    assert "dense_head_mfma" in out["extra"] and out["cpu_baseline"] is None
