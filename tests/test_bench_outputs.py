"""bench.py's plain run and --dump-outputs: the plain line carries the headline without the --full measurements, --steps
sets the timed steps, and the outputs of the last timed step are written as float32 / float64 .npy files under 64 MB,
identical for identical arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMIT = 64 * 10 ** 6


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_fits_the_budget_and_repeats(tmp_path):
    """dump_outputs on outputs of the bench shape (B = 32, T' = 400, D = 1048): the whole stays under 64 MB, only float32 /
    float64 arrays are written, small arrays are kept whole, and the sampled positions repeat from call to call."""
    import bench
    g = torch.Generator().manual_seed(3)
    B, Tg = 32, 400
    out = {"z_mel": torch.randn(B, 160, Tg, generator=g),
           "log_s_list": [torch.randn(B, Tg, 80 - 2 * (i // 2), generator=g).transpose(1, 2) for i in range(8)],
           "log_det_W_list": [torch.tensor(0.1 * i) for i in range(8)],
           "context_w_spkvec": torch.randn(B, Tg, 1048, generator=g).transpose(1, 2)}
    losses = {"loss_mel": (torch.tensor(36.5), 1.0), "loss_prior_mel": (torch.tensor(0.25), 0.0)}
    m = torch.nn.Sequential(torch.nn.Linear(1024, 1024), torch.nn.Linear(1024, 3))
    for p in m.parameters():
        p.grad = torch.randn(p.shape, generator=g)
    shapes = [bench.dump_outputs(str(tmp_path / d), out, losses, m) for d in ("a", "b")]
    assert shapes[0] == shapes[1]
    assert _dir_bytes(tmp_path / "a") < LIMIT
    assert shapes[0]["z_mel"] == [B, 160, Tg] and shapes[0]["log_det_W"] == [8] and shapes[0]["grad_norms"] == [4]
    assert shapes[0]["context_w_spkvec"][0] < B * 1048 * Tg             # the one array that had to be sampled
    for f in os.listdir(tmp_path / "a"):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64), f
        assert np.array_equal(a, b), f
    z = np.load(tmp_path / "a" / "z_mel.npy")
    assert np.array_equal(z, out["z_mel"].numpy())
    gn = np.load(tmp_path / "a" / "grad_norms.npy")
    assert np.allclose(gn, [float(p.grad.double().norm()) for p in m.parameters()], rtol=1e-12)
    assert float(np.load(tmp_path / "a" / "loss_mel.npy")[0]) == 36.5


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_same_outputs_twice(tmp_path):
    """Two plain runs with the same arguments: the result line holds the headline fields and none of the --full ones, its
    step count is --steps, and both runs write the same outputs of their last timed step."""
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                            "--batch", "8", "--frames", "400", "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        lines.append(json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]))
    res = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["value"] > 0 and res["higher_is_better"] is True
    assert abs(res["value"] - 8 * 400 / (res["ms_per_step"] * 1e-3)) < 1e-6 * res["value"]
    for k in ("roofline", "cpu_baseline", "parity_vs_cpu", "exact_split_mode", "throughput_mode", "saturation",
              "roofline_hbm", "roofline_mfma", "process_group_overhead_ms"):
        assert k not in res, k
    a, b = tmp_path / "a", tmp_path / "b"
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and {"z_mel.npy", "loss_mel.npy", "grad_norms.npy", "grad_sample.npy"} <= set(names)
    assert _dir_bytes(a) < LIMIT
    for f in names:
        x, y = np.load(a / f), np.load(b / f)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape, f
        assert np.array_equal(np.isnan(x), np.isnan(y)) and not np.isinf(x).any(), f     # NaN: a parameter without .grad
        x, y = x[~np.isnan(x)].astype(np.float64), y[~np.isnan(y)]
        assert x.size == 0 or np.abs(x - y).max() <= 1e-6 * max(np.abs(y).max(), 1e-30), f
    assert abs(float(np.load(a / "loss_mel.npy")[0]) - res["loss_mel"]) <= 1e-6 * abs(res["loss_mel"])
