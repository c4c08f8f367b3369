#!/usr/bin/env python3
"""Times the colour augmentations, the height channel and the SUN RGB-D colour step for one full scan (1 x 150k
rows) and a batch (4 x 50k rows), every gate firing:

  * the numpy restatement (tests/color_aug_restatement.py) per scene, on one core, in this process, which never opens the GPU,
    with the share of it that is drawing the random numbers;
  * the device, in a child process under ``timeout``: the launches alone between HIP events (buffers allocated and the
    parameters uploaded before; three windows of 200 so the spread shows; where the host enqueues slower than the device runs,
    the figure is the enqueue rate and says so) and whole ``augment_colors`` / ``append_height`` / ``sunrgbd_color_augment``
    calls on the host clock, draws and uploads included.

    python tools/color_aug_bench.py [--out profiles/color_aug_bench.txt]
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
import color_aug_restatement as CA  # noqa: E402

BATCHES = (("one scan", (150000,)), ("batch", (50000,) * 4))
EVERY = dict(color_drop=0.2, color_contrastp=1.0, color_jitterp=1.0, hue_sat="0.5_0.2_1.0")
REPEATS = 5


def batch(sizes, seed=0):
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    cloud = np.concatenate([rng.uniform([-4, -3, 0], [4, 3, 3], (n, 3)), rng.integers(0, 256, (n, 3))], 1).astype(np.float32)
    return cloud, np.cumsum([0] + list(sizes)).astype(np.int32)


def clock(fn, repeats=REPEATS):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return min(times)


def host_leg(emit):
    for name, sizes in BATCHES:
        cloud, off = batch(sizes)
        part = cloud[off[0]:off[1]]
        n = sizes[0]
        colour = clock(lambda: CA.color_augment_scene(part, np.random.RandomState(1), **EVERY))
        rs = np.random.RandomState(1)
        draws = clock(lambda: (rs.random(n), rs.random(), rs.random(), rs.random(), rs.randn(n, 3), rs.random(3)))
        height = clock(lambda: CA.append_height_scene(part))
        unit = part.copy()
        unit[:, 3:6] = unit[:, 3:6] / 255.0 - 0.5
        sun = clock(lambda: CA.sunrgbd_scene(unit.copy(), np.random.RandomState(2)))
        emit(f"numpy restatement, one core, {name} ({len(sizes)} x {n} rows), per scene: four colour augmentations {colour:.2f} ms "
             f"(drawing alone {draws:.2f} ms), height {height:.2f} ms, sunrgbd colour {sun:.2f} ms (best of {REPEATS})")


def device_leg():
    import torch
    from vdetr_amd import scene_prep as SP
    assert torch.cuda.is_available(), "the device leg needs a GPU"
    print(f"device: {torch.cuda.get_device_name(0)}")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def launches(what, count, fn, per):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        windows, host = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            e0.record()
            for _ in range(200):
                fn()
            e1.record()
            host.append((time.perf_counter() - t0) / 200 * 1e6)
            torch.cuda.synchronize()
            windows.append(e0.elapsed_time(e1) / 200 * 1e3)
        bound = "host enqueue" if min(host) > 0.9 * min(windows) else "device"
        print(f"{what}: the {count} {min(windows):.1f} us per batch between events (3 windows of 200: {min(windows):.1f} .. "
              f"{max(windows):.1f}; host enqueue {min(host):.1f} us: {bound}-bound) = {min(windows) / per:.1f} us per scene")

    def grab(name):
        seen, real = [], getattr(SP, name)
        setattr(SP, name, lambda *a: (seen.append(a), real(*a))[1])
        return seen, real

    for name, sizes in BATCHES:
        cloud, off = batch(sizes)
        B = len(sizes)
        pts = torch.from_numpy(cloud).cuda()
        gens = lambda: [np.random.RandomState(10 + b) for b in range(B)]  # noqa: E731
        draw = lambda rs: [SP.draw_color_augment(n, r, **EVERY) for n, r in zip(sizes, rs)]  # noqa: E731
        seen, real = grab("_launch_colors")
        try:
            coloured = SP.augment_colors(pts, off, draw(gens()))
        finally:
            SP._launch_colors = real
        launches(f"{name}, augment_colors", "three launches", lambda: real(*seen[0]), B)
        seen, real = grab("_launch_height")
        try:
            tall = SP.append_height(coloured, off)
        finally:
            SP._launch_height = real
        launches(f"{name}, append_height", "nine launches", lambda: real(*seen[0]), B)
        unit = tall.clone()
        unit[:, 3:6] = unit[:, 3:6] / 255.0 - 0.5
        seen, real = grab("_launch_sunrgbd")
        try:
            SP.sunrgbd_color_augment(unit, off, [SP.draw_sunrgbd_color(n, r) for n, r in zip(sizes, gens())])
        finally:
            SP._launch_sunrgbd = real
        launches(f"{name}, sunrgbd_color_augment", "one launch", lambda: real(*seen[0]), B)

        def whole(fn):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPEATS):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / REPEATS * 1e3
        drawing = clock(lambda: draw(gens()))
        colours = whole(lambda: SP.augment_colors(pts, off, draw(gens())))
        height = whole(lambda: SP.append_height(coloured, off))
        sun = whole(lambda: SP.sunrgbd_color_augment(unit, off, [SP.draw_sunrgbd_color(n, r) for n, r in zip(sizes, gens())]))
        print(f"{name}: whole calls on the host clock, draws and uploads included, per batch: draw_color_augment + augment_colors "
              f"{colours:.2f} ms (drawing on the host {drawing:.2f} ms of it), append_height {height:.2f} ms, draw_sunrgbd_color + "
              f"sunrgbd_color_augment {sun:.2f} ms")


def main():
    if "--device-leg" in sys.argv:
        device_leg()
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "color_aug_bench.txt")
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
