"""bench.py's plain run and --dump-outputs: the line a plain run prints, and the dumped tensor against a forward on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_output_samples_a_large_tensor_at_fixed_indices(tmp_path, monkeypatch):
    """Above DUMP_MAX_ELEMS the dump is the same seeded sample in every call (sorted flat indices), float32; below it the whole tensor."""
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    t = torch.arange(5 * 40 * 8, dtype=torch.float32).reshape(5, 40, 8).to(torch.bfloat16)   # bf16-exact only below 256: compare through float()
    a = np.load(bench.dump_output(str(tmp_path / "a"), "out", t))
    b = np.load(bench.dump_output(str(tmp_path / "b"), "out", t))
    assert a.dtype == np.float32 and a.shape == (1000,) and np.array_equal(a, b)
    flat = t.float().reshape(-1).numpy()
    assert np.all(np.diff(a) >= 0) and set(a.tolist()) <= set(flat.tolist()) and len(set(a.tolist())) > 100
    small = t[:1]   # 320 elements: written whole, in its own shape
    s = np.load(bench.dump_output(str(tmp_path / "c"), "small", small))
    assert s.dtype == np.float32 and s.shape == (1, 40, 8) and np.array_equal(s, small.float().numpy())


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_what_the_last_step_wrote(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: one JSON line with the headline keys and nothing that needs a run of
    its own (roofline / cpu_baseline null, no validation block), and DIR/out.npy bit-equal to a forward over the same seeded inputs."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["full"] is False
    assert line["unit"] == "TFLOP/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["ms_per_step"] > 0 and line["value"] > 100.0
    assert abs(line["value"] - 4.0 * 16 * 8192.0 * 8192.0 * 64 / (line["ms_per_step"] * 1e-3) / 1e12) < 0.01 * line["value"]
    assert line["roofline"] is None and line["cpu_baseline"] is None and "validation" not in line and "c5" not in line["extra"]
    out = np.load(tmp_path / "out.npy")
    assert out.dtype == np.float32 and out.shape == (16, 8192, 64) and out.nbytes <= 64 << 20

    import bench
    import flashattention_c_amd as fa
    dev = torch.device("cuda", 0)
    q, k, v = bench.make_inputs(16, 8192, 64, "bf16", dev, seed=0)
    ref = fa.forward(q, k, v, False, scale=1.0)
    assert np.array_equal(out, ref.float().cpu().numpy())
