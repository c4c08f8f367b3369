#!/usr/bin/env python3
"""Times the device NMS (1024 boxes per scene, 18 classes) next to the numpy oracle, then the rotated NMS on rotated scenes:
python tools/nms_bench.py [--rot-out FILE]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import nms_oracle as NO  # noqa: E402
from vdetr_amd.nms import batched_nms_3d  # noqa: E402

rng = np.random.default_rng(0)
B, K = 4, 1024
center = rng.uniform([1, 1, 1], [9, 7, 4], (B, K, 1, 3))
half = rng.uniform(0.15, 1.0, (B, K, 1, 3))
sg = np.array([(1, 1, 1), (1, 1, -1), (-1, 1, -1), (-1, 1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1), (-1, -1, 1)])[None, None]
corners = (center + half * sg).astype(np.float32)
score = rng.random((B, K)).astype(np.float32)
cls = rng.integers(0, 18, (B, K)).astype(np.int32)
c, s, k = (torch.from_numpy(a).cuda() for a in (corners, score, cls))
for _ in range(3):
    keep = batched_nms_3d(c, s, k)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20):
    keep = batched_nms_3d(c, s, k)
e1.record()
torch.cuda.synchronize()
gpu_us = e0.elapsed_time(e1) / 20 * 1e3
t0 = time.perf_counter()
want = [NO.nms_3d(NO.extents_with_score(corners[b], score[b], cls[b]), 0.25, same_class=True) for b in range(B)]
cpu_ms = (time.perf_counter() - t0) * 1e3
ok = all(set(np.nonzero(keep[b].cpu().numpy())[0]) == set(want[b]) for b in range(B))
print(f"nms3d {B} scenes x {K} boxes: device {gpu_us:.1f} us (sort + kernel), numpy oracle {cpu_ms:.1f} ms, kept {int(keep.sum())}, identical {ok}")
# components
def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
print(f"  stable sort alone: {timeit(lambda: torch.sort(s, dim=1, stable=True)):.1f} us")
import ctypes
from vdetr_amd import _lib as L
order = torch.sort(s, dim=1, stable=True)[1].contiguous()
keep8 = torch.empty((B, K), dtype=torch.uint8, device="cuda")
nb = L.lib().vdetr_nms3d_workspace_bytes(B, K)
ws = L.workspace(nb, s.device)
print(f"  kernel alone: {timeit(lambda: L.lib().vdetr_nms3d_f32(L.ptr(c), L.ptr(s), L.ptr(k), None, L.ptr(order), B, K, 0.25, 0, L.ptr(keep8), L.ptr(ws), nb, L.stream_ptr())):.1f} us")


# ---- the rotated leg, written to profiles/nms_rot_bench.txt or to `--rot-out FILE` ------------------------------
def rotated_leg(B, K, out, cpu_scenes=1):
    """C5-like scenes (SUN RGB-D: 10 classes, boxes with a yaw): most predictions are jittered copies of a dozen objects, the
    rest are loose boxes.  Times the rotated call, the axis-aligned call on the same inputs and the numpy restatement."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import rot_nms_restatement as RN
    rng = np.random.default_rng(B * K)
    corners, cls = np.empty((B, K, 8, 3), np.float32), np.empty((B, K), np.int32)
    for b in range(B):
        objs = [(rng.uniform(0.4, 2.0, 3), rng.uniform(-3.1, 3.1), rng.uniform([0, 0, 0], [6, 1.5, 5]), rng.integers(0, 10)) for _ in range(12)]
        for k in range(K):
            if rng.random() < 0.8:
                size, yaw, ctr, c = objs[rng.integers(0, 12)]
                j = rng.choice([0.05, 0.15, 0.3])
                size, yaw, ctr = size * (1 + rng.normal(0, j, 3)).clip(0.5, 1.5), yaw + rng.normal(0, j), ctr + rng.normal(0, j, 3) * size
                c = c if rng.random() < 0.9 else rng.integers(0, 10)
            else:
                size, yaw, ctr, c = rng.uniform(0.4, 2.0, 3), rng.uniform(-3.1, 3.1), rng.uniform([0, 0, 0], [6, 1.5, 5]), rng.integers(0, 10)
            corners[b, k], cls[b, k] = RN.box(size, yaw, ctr), c
    score = rng.random((B, K)).astype(np.float32)
    c, s, k = (torch.from_numpy(a).cuda() for a in (corners, score, cls))
    rot_us = timeit(lambda: batched_nms_3d(c, s, k, rotated=True), n=50)
    plain_us = timeit(lambda: batched_nms_3d(c, s, k), n=50)
    rot_us2 = timeit(lambda: batched_nms_3d(c, s, k, rotated=True), n=50)     # alternated: the spread of the same call
    plain_us2 = timeit(lambda: batched_nms_3d(c, s, k), n=50)
    keep, plain = batched_nms_3d(c, s, k, rotated=True).cpu().numpy(), batched_nms_3d(c, s, k).cpu().numpy()
    t0 = time.perf_counter()
    want = [RN.nms_rotated(corners[b], score[b], cls[b], None, 0.25)[0] for b in range(cpu_scenes)]
    cpu_ms = (time.perf_counter() - t0) * 1e3 / cpu_scenes
    ok = all(np.array_equal(keep[b], want[b]) for b in range(cpu_scenes))
    # pairs (r, s > r) that pass the kernel's pre-tests (same class, heights overlap) and so reach the clip
    top, bottom = corners[:, :, 0, 1].astype(np.float64), corners[:, :, 4, 1].astype(np.float64)
    reach = (cls[:, :, None] == cls[:, None, :]) & (np.minimum(top[:, :, None], top[:, None, :]) - np.maximum(bottom[:, :, None], bottom[:, None, :]) > 0)
    frac = (reach.sum() - B * K) / 2 / (B * K * (K - 1) / 2)
    line = (f"nms3d_rot {B} scenes x {K} boxes: rotated call {rot_us:.1f} / {rot_us2:.1f} us, axis-aligned call on the same boxes "
            f"{plain_us:.1f} / {plain_us2:.1f} us (sort + 3 kernels each), numpy restatement {cpu_ms:.0f} ms per scene, kept {int(keep.sum())} "
            f"(axis-aligned {int(plain.sum())}), first {cpu_scenes} scene(s) identical to the restatement {ok}, pairs that reach the clip "
            f"{100 * frac:.2f} % of K(K-1)/2")
    print(line)
    out.write(line + "\n")


path = sys.argv[sys.argv.index("--rot-out") + 1] if "--rot-out" in sys.argv else os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "nms_rot_bench.txt")
with open(path, "w") as fh:
    rotated_leg(4, 1024, fh)
    rotated_leg(1, 4096, fh)
