#!/usr/bin/env python3
"""Times the cuboid crop and the sampling for a C2-like batch (1 scene x 40k points, 64 boxes) and a C5-like
batch (4 scenes x 20k points, 64 boxes), min_points at a quarter of a scene (uniform synthetic clouds: a mix of early, late and no acceptance):

  * the numpy restatement (tests/cuboid_restatement.py) per scene, on one core, in this process, which never opens the GPU;
  * the device, in a child process under ``timeout``: the six launches alone between HIP events (buffers allocated and the
    sample drawn before; three windows of 500 so the spread shows; where the host enqueues slower than the device runs, the
    figure is the enqueue rate and says so) and a whole ``crop_and_sample`` call, which ends in its own read-back, on the
    host clock, with the share of it that is the host drawing the attempts.

    python tools/cuboid_bench.py [--out profiles/cuboid_bench.txt]
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
import cuboid_restatement as CR  # noqa: E402

BATCHES = (("C2-like", (40000,)), ("C5-like", (20000,) * 4))
SEEDS = 8


def batch(sizes, seed=0):
    rng = np.random.default_rng(seed)
    B, G = len(sizes), 64
    return {"points": rng.uniform([-4, -3, 0], [4, 3, 3], (sum(sizes), 3)).astype(np.float32), "offsets": np.cumsum([0] + list(sizes)).astype(np.int32),
            "boxes": np.concatenate([rng.uniform([-4, -3, 0], [4, 3, 3], (B, G, 3)), rng.uniform(0.2, 2, (B, G, 3))], 2),
            "box_counts": np.full(B, G, np.int64), "box_classes": rng.integers(0, 18, (B, G))}


def host_leg(emit):
    for name, sizes in BATCHES:
        c = batch(sizes)
        n, mp = sizes[0], sizes[0] // 4
        times, trials = [], []
        for seed in range(SEEDS):                                      # the attempts gone through vary with the stream
            rs = [np.random.RandomState(100 * seed + b) for b in range(len(sizes))]
            t0 = time.perf_counter()
            w = CR.crop_and_sample_batch(c["points"], c["offsets"], c["boxes"], c["box_counts"], c["box_classes"], rs, n, mp)
            times.append((time.perf_counter() - t0) / len(sizes) * 1e3)
            trials += w["trial"].tolist()
        emit(f"numpy restatement, one core, {name} ({len(sizes)} x {n} points, min_points {mp}): {np.mean(times):.2f} ms per scene "
             f"(mean of {SEEDS} streams: {min(times):.2f} .. {max(times):.2f}; accepted attempts {trials})")


def device_leg():
    import torch
    from vdetr_amd import scene_prep as SP
    assert torch.cuda.is_available(), "the device leg needs a GPU"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    print(f"device: {torch.cuda.get_device_name(0)}")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, sizes in BATCHES:
        c = batch(sizes)
        n, mp = sizes[0], sizes[0] // 4
        args = (up(c["points"]), c["offsets"], up(c["boxes"]), up(c["box_counts"]), up(c["box_classes"]))
        gens = lambda seed: [np.random.RandomState(100 * seed + b) for b in range(len(sizes))]  # noqa: E731
        seen, crop, compose = [], SP._launch_crop, SP._launch_compose
        SP._launch_crop = lambda *a: (seen.append(a), crop(*a))[1]
        SP._launch_compose = lambda *a: (seen.append(a), compose(*a))[1]
        try:
            keep = SP.crop_and_sample(*args, gens(0), n, min_points=mp)  # its buffers are what the launches below read and write
        finally:
            SP._launch_crop, SP._launch_compose = crop, compose
        six = lambda: (crop(*seen[0]), compose(*seen[1]))  # noqa: E731  (seen holds the workspace and every tensor of the call)
        for _ in range(20):
            six()
        torch.cuda.synchronize()
        windows, host = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            e0.record()
            for _ in range(500):
                six()
            e1.record()
            host.append((time.perf_counter() - t0) / 500 * 1e6)
            torch.cuda.synchronize()
            windows.append(e0.elapsed_time(e1) / 500 * 1e3)
        bound = "host enqueue" if min(host) > 0.9 * min(windows) else "device"
        print(f"{name}: the six launches {min(windows):.1f} us per batch between events (3 windows of 500: {min(windows):.1f} .. "
              f"{max(windows):.1f}; host enqueue {min(host):.1f} us: {bound}-bound) = {min(windows) / len(sizes):.1f} us per scene; "
              f"accepted attempts {keep['trial'].tolist()}")
        t0 = time.perf_counter()
        for seed in range(SEEDS):
            for r, m in zip(gens(seed), sizes):
                SP.draw_cuboid_trials(m, r)
        draw = (time.perf_counter() - t0) / SEEDS * 1e6
        for seed in range(3):
            SP.crop_and_sample(*args, gens(seed), n, min_points=mp)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for seed in range(SEEDS * 4):
            SP.crop_and_sample(*args, gens(seed % SEEDS), n, min_points=mp)
        torch.cuda.synchronize()
        call = (time.perf_counter() - t0) / (SEEDS * 4) * 1e6
        print(f"{name}: crop_and_sample, whole call (attempts drawn on the host {draw:.0f} us of it, uploads, six launches, the "
              f"read-back, the sample drawn on the host), host clock: {call:.0f} us per batch = {call / len(sizes):.0f} us per scene")


def main():
    if "--device-leg" in sys.argv:
        device_leg()
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "cuboid_bench.txt")
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
