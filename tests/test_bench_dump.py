"""bench.py's --dump-outputs and --steps on the CPU: what dump_outputs writes (float32 / float64 .npy files, a fixed and seeded
sample of a large array, at most 64 MB in all) from a stand-in trainer, and the argument check of --steps."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Step:
    """what bench.Trainer holds after a step with keep_outputs on"""

    def __init__(self, bench, n_rows):
        g = torch.Generator().manual_seed(3)
        out = {"outputs": {"sem_cls_logits": torch.randn(1, 8, 19, generator=g), "box_corners": torch.randn(1, 8, 8, 3, generator=g),
                           "angle_class": torch.zeros(1, 8, dtype=torch.int64), "_query_reference": torch.randn(1, 8, 6, generator=g)},
               "aux_outputs": [{"sem_cls_logits": torch.randn(1, 8, 19, generator=g)}], "seed_xyz": torch.randn(1, 16, 3, generator=g)}
        self.loss = torch.tensor(-1.25)
        self.last_outputs = bench.step_outputs(out)
        self.last_feature_grads = [torch.randn(n_rows, 256, generator=g), None]


def test_dump_outputs_files(tmp_path):
    import bench
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(1024, 1100), torch.nn.BatchNorm1d(1100))  # 1.1 M parameters: sampled
    step = _Step(bench, 3000)                                                               # 768 k gradient entries: whole
    bench.dump_outputs(str(tmp_path / "a"), step, model)
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert names == ["aux0_sem_cls_logits", "backbone_features_grad", "loss", "model_state", "outputs_box_corners",
                     "outputs_sem_cls_logits", "seed_xyz"]  # (integer and `_`-prefixed entries are not outputs of the model)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in names}
    assert all(x.dtype in (np.float32, np.float64) for x in got.values())
    assert sum(x.nbytes for x in got.values()) <= 64 << 20
    assert got["loss"].dtype == np.float64 and got["loss"].tolist() == [-1.25]
    np.testing.assert_array_equal(got["outputs_box_corners"], step.last_outputs["outputs_box_corners"].numpy())
    np.testing.assert_array_equal(got["backbone_features_grad"], step.last_feature_grads[0].reshape(-1).numpy())
    state = torch.cat([v.reshape(-1).float() for v in model.state_dict().values() if v.is_floating_point()])
    assert state.numel() > bench.DUMP_SAMPLE and got["model_state"].shape == (bench.DUMP_SAMPLE,)
    idx = np.sort(np.random.default_rng(2).choice(state.numel(), bench.DUMP_SAMPLE, replace=False))
    np.testing.assert_array_equal(got["model_state"], state.numpy()[idx])
    # the same step dumped again: the same sample, file for file
    bench.dump_outputs(str(tmp_path / "b"), step, model)
    for n in names:
        np.testing.assert_array_equal(np.load(tmp_path / "b" / f"{n}.npy"), got[n])


def test_dump_outputs_samples_a_large_gradient(tmp_path):
    import bench
    step = _Step(bench, 5000)  # 1.28 M entries
    bench.dump_outputs(str(tmp_path), step, torch.nn.Linear(4, 4))
    g = np.load(tmp_path / "backbone_features_grad.npy")
    flat = step.last_feature_grads[0].reshape(-1).numpy()
    idx = np.sort(np.random.default_rng(1).choice(flat.size, bench.DUMP_SAMPLE, replace=False))
    np.testing.assert_array_equal(g, flat[idx])


def test_steps_must_be_positive():
    """ms_per_step is the timed span over --steps: zero steps is refused before anything starts"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
