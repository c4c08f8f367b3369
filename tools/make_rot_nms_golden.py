#!/usr/bin/env python3
"""Generates tests/golden/nms3d_rot.npz: rotated boxes drawn with the reference's ``get_3d_box``, the pairwise matrix of
the reference's own ``box3d_iou`` (utils/box_util.py:122-147, called on ``corners.astype(float)`` as utils/eval_det.py:151-153
does) and the keep masks of a plain Python greedy NMS over that function (build container only, like oracle/make_golden.py,
whose import recipe it reuses).  The reference has no working rotated NMS; DESIGN.md 6.3 defines the one pinned here.

    python tools/make_rot_nms_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as MG  # noqa: E402

VARIANTS = {  # name -> (same class only, threshold, old type)
    "samecls_0.25": (True, 0.25, False), "samecls_0.5": (True, 0.5, False), "any_0.25": (False, 0.25, False),
    "any_0.5": (False, 0.5, False), "samecls_old_0.25": (True, 0.25, True), "samecls_old_0.5": (True, 0.5, True),
    "any_old_0.5": (False, 0.5, True)}


def greedy(B, corners, score, cls, valid, same_class, thr, old_type):
    """nms.py:78-162 on the non-empty boxes (ap_calculator.py:209-219) with the rotated overlap; the visiting order is a
    stable arg-sort, as the device path defines it."""
    c = corners.astype(float)
    idx = np.nonzero(valid)[0]
    remaining = list(idx[np.argsort(score[idx], kind="stable")])
    keep = np.zeros(len(score), bool)
    while remaining:
        i = remaining.pop()
        keep[i] = True
        rest = []
        for j in remaining:
            with np.errstate(all="ignore"):
                if old_type:
                    r1 = [(c[i][k, 0], c[i][k, 2]) for k in range(3, -1, -1)]
                    r2 = [(c[j][k, 0], c[j][k, 2]) for k in range(3, -1, -1)]
                    _, area = B.convex_hull_intersection(r1, r2)
                    inter = area * max(0.0, min(c[i][0, 1], c[j][0, 1]) - max(c[i][4, 1], c[j][4, 1]))
                    o = inter / B.box3d_vol(c[j])
                else:
                    o = B.box3d_iou(c[i], c[j])[0]
            if same_class:
                o = o * (cls[i] == cls[j])
            if not o > thr:
                rest.append(j)
        remaining = rest
    return keep


def scene(B, rng, K, yaw0=False, special=False, room=(5, 2, 4)):
    """Clusters of jittered copies (overlaps on both sides of both thresholds) and loose boxes in a room."""
    boxes = []
    if special:
        a = 0.7
        for d in (0.0, 1e-7, 0.0):                     # nearly coincident: same centre and size, yaw apart by 1e-7 and by 0
            boxes.append(((1.2, 0.8, 1.0), a + d, (2.0, 1.0, 2.0)))
        for x in (0.0, 1.0, 2.0):                      # touching without overlapping: shared faces, side by side ...
            boxes.append(((1.0, 0.5, 1.0), 0.0, (x, 0.5, 0.25)))
        boxes.append(((1.0, 0.5, 1.0), 0.0, (0.0, 1.5, 0.25)))   # ... and stacked
    while len(boxes) < K:
        size, yaw = rng.uniform(0.4, 2.0, 3), 0.0 if yaw0 else rng.uniform(-3.1, 3.1)
        center = rng.uniform([0, 0, 0], room)
        boxes.append((size, yaw, center))
        for _ in range(rng.integers(0, 4)):
            jit = rng.choice([0.05, 0.15, 0.3])
            boxes.append((size * (1 + rng.normal(0, jit, 3)).clip(0.5, 1.5), 0.0 if yaw0 else yaw + rng.normal(0, jit),
                          center + rng.normal(0, jit, 3) * size))
    boxes = boxes[:K]
    corners = np.stack([B.get_3d_box(np.asarray(s, float), y, np.asarray(p, float)) for s, y, p in boxes]).astype(np.float32)
    score = (rng.integers(0, 40, K) / 40).astype(np.float32) if special else rng.random(K).astype(np.float32)
    cls = rng.integers(0, 3, K).astype(np.int32)
    if special:
        cls[:7] = 0
    return corners, score, cls


def main():
    MG.import_reference()
    import utils.box_util as B  # noqa  (reference)
    rng = np.random.default_rng(63)
    arrays = {}
    # c0: 64 rotated boxes with the hand-made groups; c1: all yaw 0; c2, c3: a batch of two scenes with a valid mask
    cases = [scene(B, rng, 64, special=True, room=(8, 2.5, 6)), scene(B, rng, 32, yaw0=True), scene(B, rng, 24), scene(B, rng, 24)]
    valid = [np.ones(64, bool), np.ones(32, bool), rng.random(24) > 0.3, rng.random(24) > 0.3]
    for ci, ((corners, score, cls), v) in enumerate(zip(cases, valid)):
        arrays[f"c{ci}:corners"], arrays[f"c{ci}:score"], arrays[f"c{ci}:cls"], arrays[f"c{ci}:valid"] = corners, score, cls, v
        arrays[f"c{ci}:keep"] = np.stack([greedy(B, corners, score, cls, v, *VARIANTS[n]) for n in VARIANTS])   # [variant, K]
        print(ci, dict(zip(VARIANTS, arrays[f"c{ci}:keep"].sum(1).tolist())))
    c = cases[0][0].astype(float)
    with np.errstate(all="ignore"):
        arrays["c0:iou"] = np.array([[B.box3d_iou(c[i], c[j])[0] for j in range(64)] for i in range(64)], np.float64)
    arrays["ncases"], arrays["variants"] = np.array(len(cases)), np.array(list(VARIANTS))
    MG.save("nms3d_rot", **arrays)


if __name__ == "__main__":
    main()
