"""bench.py: what `--dump-outputs` writes (CPU), and a plain run with `--dump-outputs` on the device (GPU)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_probe", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_step_outputs_are_float_bounded_and_a_fixed_sample():
    import torch
    bench = _bench_module()
    B, G, M = 300, 100, 3
    g = torch.Generator().manual_seed(1)
    r = {"agent_id": torch.randint(-1, M, (B,), dtype=torch.int32, generator=g),
         "reward": torch.rand(B, dtype=torch.float64, generator=g),
         "terminal": torch.randint(0, 2, (B,), dtype=torch.uint8, generator=g),
         "now": torch.rand(B, dtype=torch.float64, generator=g) * 1e3,
         "status": torch.randint(0, 5, (B,), dtype=torch.int32, generator=g),
         "state": torch.rand((B, 4, G, G), dtype=torch.float32, generator=g)}
    table = torch.rand((B, M + 3), dtype=torch.float64, generator=g)
    a, b = bench.step_outputs(torch, r, table), bench.step_outputs(torch, r, table)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert sorted(a) == sorted(b) == ["agent_id", "now", "reward", "rollout_table", "state", "state_rows", "status", "terminal"]
    for k, x in a.items():
        assert x.dtype in (np.float32, np.float64), k
        np.testing.assert_array_equal(x, b[k])
    for k in ("agent_id", "reward", "terminal", "now", "status"):
        np.testing.assert_array_equal(a[k], r[k].numpy().astype(np.float64))
    rows = a["state_rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_STATE_ROWS and len(set(rows.tolist())) == len(rows) and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(a["state"], r["state"].numpy()[rows])
    np.testing.assert_array_equal(a["rollout_table"], table.numpy())


@pytest.mark.gpu
def test_plain_bench_run_line_and_repeatable_outputs(tmp_path):
    """A plain run prints the headline line without the --full figures; two runs with the same arguments dump the same outputs."""
    lines = []
    for i in range(2):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", "64", "--steps", "3", "--warmup", "2",
               "--dump-outputs", str(tmp_path / str(i))]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        lines.append(json.loads(p.stdout.strip().splitlines()[-1]))
    line = lines[0]
    assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["steps"] == 3
    assert line["value"] > 0 and line["ms_per_step"] > 0 and "dtype" in line and "metric" in line
    assert not {"kernels", "roofline", "extended", "blocking", "cpu_baseline"} & set(line)
    assert lines[0]["env_steps_timed"] == lines[1]["env_steps_timed"]
    names = sorted(os.listdir(tmp_path / "0"))
    assert names == sorted(os.listdir(tmp_path / "1"))
    assert names == sorted(k + ".npy" for k in ("agent_id", "reward", "terminal", "now", "status", "state", "state_rows", "rollout_table"))
    for n in names:
        a, b = np.load(tmp_path / "0" / n), np.load(tmp_path / "1" / n)
        assert a.dtype in (np.float32, np.float64), n
        np.testing.assert_array_equal(a, b, err_msg=n)
    assert np.load(tmp_path / "0" / "state.npy").shape == (64, 4, 100, 100)
