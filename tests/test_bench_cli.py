"""bench.py's command line: a plain run is the headline step alone, `--steps` is the number of timed steps, and
`--dump-outputs DIR` writes what the last timed step computed (CPU: the flags and the writer; GPU: one small plain run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY_KEYS = ("projector", "joint", "sinkhorn", "rasteriser", "kernel_families", "roofline", "cpu_baseline")


def _bench(args, **kw):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, **kw)


def test_bench_refuses_zero_steps_and_a_dump_of_another_workload():
    r = _bench(["--steps", "0"], timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr and '"metric"' not in r.stdout
    r = _bench(["--workload", "projector", "--dump-outputs", "unused"], timeout=300)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr and '"metric"' not in r.stdout


def test_dump_outputs_writes_the_last_step(tmp_path):
    """The writer on a CPU regression step (the oracle's stock-op encoder and Sinkhorn term stand in for the HIP ones)."""
    sys.path.insert(0, ROOT)
    import oracle
    import bench
    from emlight_amd.RegressionNetwork.data import synthetic_batch
    from emlight_amd.RegressionNetwork.engine import RegressionTrainer
    anchors, crop = 16, (32, 32)
    torch.manual_seed(0)
    M = oracle.anchor_cost_matrix(anchors)
    tr = RegressionTrainer(anchors=anchors, crop_hw=crop, blur=.05, device="cpu",
                           model=oracle.OracleDenseNet(anchors=anchors, crop_hw=crop),
                           sam_loss=lambda x, y: oracle.samples_loss(x, y, M, blur=.05))
    batch = synthetic_batch(2, anchors, crop, seed=1234)
    result = tr.step(batch)
    bench.dump_outputs(str(tmp_path), result, tr.last_pred, tr.model)
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert set(got) == {"loss", "loss_dist_emloss", "loss_dist_l2loss", "loss_intensity_loss", "loss_rgb_loss",
                        "loss_ambient_loss", "pred_distribution", "pred_intensity", "pred_rgb_ratio", "pred_ambient",
                        "grads_sample", "params_sample"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert float(got["loss"]) == pytest.approx(float(result[0]), rel=1e-6)
    np.testing.assert_array_equal(got["pred_distribution"], tr.last_pred["distribution"].detach().numpy())
    n = sum(p.numel() for p in tr.model.parameters())
    assert got["params_sample"].size == min(n, bench.DUMP_SAMPLE) and np.abs(got["grads_sample"]).max() > 0


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_bench_line_and_dump(tmp_path):
    """A plain run: the headline keys, exactly `--steps` timed steps, none of the `--full` objects; its dump holds the last
    timed step's outputs, float32, well under 64 MB."""
    r = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4", "--dump-outputs", str(tmp_path)], timeout=550)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert all(k in j for k in HEADLINE_KEYS) and not any(k in j for k in FULL_ONLY_KEYS), sorted(j)
    assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["value"] == pytest.approx(4 * 1e3 / j["ms_per_step"], rel=1e-2)
    files = sorted(os.listdir(tmp_path))
    assert "loss.npy" in files and "pred_distribution.npy" in files and "grads_sample.npy" in files
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in files) < 64 << 20
    d = np.load(os.path.join(tmp_path, "pred_distribution.npy"))
    assert d.shape == (4, 128) and d.dtype == np.float32 and np.isfinite(d).all()
