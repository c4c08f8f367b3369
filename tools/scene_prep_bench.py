#!/usr/bin/env python3
"""Times the scene preparation for a C2-like batch (1 scene x 40k points, 64 boxes) and a C5-like batch
(4 scenes x 20k points, 64 boxes), colours on:

  * the numpy restatement (tests/scene_prep_restatement.py) per scene, on one core, in this process, which never opens the GPU;
  * the device, in a child process under ``timeout``: the two launches alone between HIP events (buffers allocated before,
    three windows of 2000 pairs each, so the spread shows; where the host enqueues slower than the device runs, the figure is
    the enqueue rate and says so), a whole ``prepare_scenes`` call ended by a synchronise, and the largest float32-ulp
    difference of the device against tests/golden/scene_prep.npz.

    python tools/scene_prep_bench.py [--out profiles/scene_prep_bench.txt]
"""
import os
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):   # one core for numpy, before it loads
    os.environ[_v] = "1"
import subprocess  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_prep_restatement as SR  # noqa: E402

BATCHES = (("C2-like", (40000,)), ("C5-like", (20000,) * 4))
MEAN = np.full((18, 3), 0.8)


def batch(sizes, seed=0):
    rng = np.random.default_rng(seed)
    B, G = len(sizes), 64
    return {"points": rng.uniform([-4, -3, 0, 0, 0, 0], [4, 3, 3, 255, 255, 255], (sum(sizes), 6)).astype(np.float32),
            "offsets": np.cumsum([0] + list(sizes)).astype(np.int32),
            "boxes": np.concatenate([rng.uniform([-4, -3, 0], [4, 3, 3], (B, G, 3)), rng.uniform(0.2, 2, (B, G, 3))], 2).astype(np.float32),
            "box_counts": np.full(B, G, np.int64), "box_classes": rng.integers(0, 18, (B, G))}


def host_leg(emit):
    from vdetr_amd.scene_prep import draw_augment_params
    for name, sizes in BATCHES:
        c = batch(sizes)
        p = draw_augment_params(len(sizes), 5.0, 0.4, 0.4, np.random.RandomState(0))
        run = lambda: SR.prepare_batch(c["points"], c["offsets"], c["boxes"], c["box_counts"], c["box_classes"], p, MEAN, color_mean=-1.0)  # noqa: E731
        run()
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(10):
                run()
            times.append((time.perf_counter() - t0) / 10 / len(sizes) * 1e3)
        emit(f"numpy restatement, one core, {name} ({len(sizes)} x {sizes[0]} points): {min(times):.2f} ms per scene "
             f"(5 windows of 10 batches: {min(times):.2f} .. {max(times):.2f}) = {1e3 / min(times):.0f} scenes/s per core")


def device_leg():
    import torch
    from test_scene_prep_restatement import CASES, golden, params_of
    from vdetr_amd import scene_prep as SP
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    assert torch.cuda.is_available(), "the device leg needs a GPU"
    cfg = ScannetDatasetConfig()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    print(f"device: {torch.cuda.get_device_name(0)}")
    worst = 0.0
    for name in CASES:
        c = golden()[name]
        color = float(c["color_mean"]) if bool(c["use_color"]) else None
        out = SP.prepare_scenes(up(c["points"]), c["offsets"], up(c["boxes"]), up(c["box_counts"]), up(c["box_classes"]), params_of(c),
                                cfg, choices=c.get("choices"), color_mean=color)
        got = {k: v.cpu().numpy() for k, v in out.items() if k != "point_clouds"}
        got["out_points"] = torch.cat(out["point_clouds"]).cpu().numpy()
        w = 0.0
        for k in SR.FLOAT_KEYS + ("out_points",):
            u = SR.ulps(got[k], c[k])
            u[np.abs(got[k].astype(np.float64) - c[k].astype(np.float64)) <= 1e-9] = 0
            w = max(w, float(u.max()))
        print(f"device against the reference fixture, case {name}: largest difference {w:.2f} float32 ulps")
        worst = max(worst, w)
    print(f"largest float32-ulp difference against tests/golden/scene_prep.npz: {worst:.2f}")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, sizes in BATCHES:
        c = batch(sizes)
        p = SP.draw_augment_params(len(sizes), 5.0, 0.4, 0.4, np.random.RandomState(0))
        args = (up(c["points"]), c["offsets"], up(c["boxes"]), up(c["box_counts"]), up(c["box_classes"]), p, cfg)
        seen, real = [], SP._launch_pair
        SP._launch_pair = lambda *a: (seen.append(a), real(*a))[1]
        try:
            keep = SP.prepare_scenes(*args, color_mean=-1.0)             # noqa: F841  (its buffers are what the pairs below write)
        finally:
            SP._launch_pair = real
        pair = seen[0]
        for _ in range(50):
            real(*pair)
        torch.cuda.synchronize()
        windows, host = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            e0.record()
            for _ in range(2000):
                real(*pair)
            e1.record()
            host.append((time.perf_counter() - t0) / 2000 * 1e6)
            torch.cuda.synchronize()
            windows.append(e0.elapsed_time(e1) / 2000 * 1e3)
        bound = "host enqueue" if min(host) > 0.9 * min(windows) else "device"
        print(f"{name}: the two launches {min(windows):.1f} us per batch between events (3 windows of 2000: {min(windows):.1f} .. "
              f"{max(windows):.1f}; host enqueue {min(host):.1f} us per pair: {bound}-bound) = {min(windows) / len(sizes):.1f} us per scene")
        for _ in range(20):
            SP.prepare_scenes(*args, color_mean=-1.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            SP.prepare_scenes(*args, color_mean=-1.0)
        torch.cuda.synchronize()
        call = (time.perf_counter() - t0) / 200 * 1e6
        print(f"{name}: prepare_scenes, whole call (uploads of the parameters, 14 allocations, two launches), host clock to a "
              f"synchronise: {call:.0f} us per batch = {call / len(sizes):.0f} us per scene")


def main():
    if "--device-leg" in sys.argv:
        device_leg()
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "scene_prep_bench.txt")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    host_leg(emit)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--device-leg"], capture_output=True, text=True)
    for s in r.stdout.splitlines():
        emit(s)
    if r.returncode != 0:
        emit(f"device leg ended with status {r.returncode}: not measured")
        sys.stderr.write(r.stderr[-4000:])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
