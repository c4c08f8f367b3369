#!/usr/bin/env python3
"""Generates tests/golden/ap_sizes.npz: a few scans in the form ``eval_store.DetectionStore.append`` takes (keep, corners,
scores, cls, gt_corners, gt_cls, gt_present; the per-class scoring form, scores [B,K,C]) and, from the reference's own
``eval_det_multiprocessing`` (utils/eval_det.py:244-302) with ``size`` in S, M, L at 0.25 and 0.5, every class's AP and last
recall (build container only, like oracle/make_golden.py, whose import recipe it reuses).  The first pin of the size split of
``--test_size`` to the reference.

Two quirks of the reference are kept out of the recording, and asserted: every ground-truth class has an unfiltered detection
(``ret_values[i]`` of eval_det.py:293-295 shifts otherwise), and no two detections of one class and size share a score (its
``np.argsort`` is not stable).

    python tools/make_ap_sizes_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as MG  # noqa: E402

B, K, C, G = 4, 20, 3, 6
SIZES = ("S", "M", "L")
THRESHOLDS = (0.25, 0.5)
EDGES = {"S": (0.35, 0.55), "M": (0.58, 0.74), "L": (0.8, 1.3)}     # edge lengths whose products stay inside one volume class


def inputs(get_3d_box):
    """Scan 0 is axis-aligned and holds the rows on the bounds (extents 1, 1, float32(bound) with the minimum corner at the
    origin: the three differences are exact), scan 1 is axis-aligned, scan 2 rotated (box3d_vol_batch is then not l w h),
    scan 3 has no present ground truth.  Detections: jittered copies of the ground truth, then loose boxes."""
    rng = np.random.default_rng(89)
    corners, gt_corners = np.zeros((B, K, 8, 3), np.float32), np.zeros((B, G, 8, 3), np.float32)
    gt_cls, present = rng.integers(0, C, (B, G)), np.ones((B, G), bool)
    present[3] = False
    present[1, 4:] = False
    for b in range(B):
        kinds = rng.permutation(np.resize(np.arange(3), G))
        g_size = np.stack([rng.uniform(*EDGES[SIZES[k]], 3) for k in kinds])
        g_yaw = rng.uniform(-0.6, 0.6, G) if b == 2 else np.zeros(G)
        g_ctr = rng.uniform([2, 0, 2], [9, 2, 8], (G, 3))
        src = np.concatenate((np.arange(G), rng.integers(0, G, 6), np.full(K - G - 6, -1)))
        jit = rng.choice([0.02, 0.08, 0.2], (K, 1))       # overlaps on both sides of both thresholds
        size = np.where(src[:, None] >= 0, g_size[src] * (1 + rng.normal(0, 0.3, (K, 3)) * jit), rng.uniform(0.35, 1.3, (K, 3)))
        yaw = np.where(src >= 0, g_yaw[src] + rng.normal(0, 0.04, K) * (b == 2), rng.uniform(-0.6, 0.6, K) * (b == 2))
        ctr = np.where(src[:, None] >= 0, g_ctr[src] + rng.normal(0, 1, (K, 3)) * jit * g_size[src], rng.uniform([2, 0, 2], [9, 2, 8], (K, 3)))
        if b == 0:      # on the bounds: ground-truth slots 0, 1 and detections 0, 1 (their copies)
            for j, bound in enumerate((0.17, 0.44)):
                g_size[j] = size[j] = (1.0, 1.0, float(np.float32(bound)))
                g_ctr[j] = ctr[j] = g_size[j][[0, 2, 1]] / 2
        gt_corners[b] = np.stack([get_3d_box(g_size[j], g_yaw[j], g_ctr[j]) for j in range(G)]).astype(np.float32)
        corners[b] = np.stack([get_3d_box(size[j], yaw[j], ctr[j]) for j in range(K)]).astype(np.float32)
    keep = rng.random((B, K)) < 0.85
    keep[0, :2] = True
    scores = rng.random((B, K, C)).astype(np.float32)
    return dict(keep=keep, corners=corners, scores=scores, cls=scores.argmax(-1).astype(np.int64), gt_corners=gt_corners,
                gt_cls=gt_cls.astype(np.int64), gt_present=present)


def reference_lists(z):
    """pred_all / gt_all as APCalculator.step leaves them: per scan the kept boxes class-major (ap_calculator.py:253-262)"""
    pred_all, gt_all = {}, {}
    for b in range(B):
        kept = np.nonzero(z["keep"][b])[0]
        pred_all[b] = [(c, z["corners"][b, k], z["scores"][b, k, c]) for c in range(C) for k in kept]
        gt_all[b] = [(int(z["gt_cls"][b, g]), z["gt_corners"][b, g]) for g in np.nonzero(z["gt_present"][b])[0]]
    return pred_all, gt_all


def size_of(vol):
    """the reference's comparisons (eval_det.py:89-104) on a float32 volume array -> 0, 1, 2 or 3 = no size"""
    lo, hi = 0.17, 0.44
    return np.where(vol < lo, 0, np.where(np.logical_and(vol > lo, vol < hi), 1, np.where(vol > hi, 2, 3)))


def main():
    MG.import_reference()
    from utils.box_util import get_3d_box  # noqa  (reference)
    from utils.eval_det import box3d_vol_batch, eval_det_multiprocessing, get_iou_obb  # noqa  (reference)
    z = inputs(get_3d_box)
    pred_all, gt_all = reference_lists(z)
    det_size = size_of(box3d_vol_batch(z["corners"][z["keep"]]))
    gt_size = size_of(box3d_vol_batch(z["gt_corners"][z["gt_present"]]))
    assert all((det_size == k).any() and (gt_size == k).any() for k in range(4)), (np.bincount(det_size), np.bincount(gt_size))
    assert z["keep"].any()                                   # per-class form: every class then has an unfiltered detection
    for c in range(C):
        for k in range(3):
            s = z["scores"][z["keep"]][det_size == k, c]
            assert len(np.unique(s)) == len(s), (c, k)
    arrays = dict(z)
    for size in SIZES:
        for thr in THRESHOLDS:
            rec, _, ap = eval_det_multiprocessing(pred_all, gt_all, ovthresh=thr, get_iou_func=get_iou_obb, size=size)
            keys = sorted(ap)
            last = [float(rec[c][-1]) if isinstance(rec[c], np.ndarray) and rec[c].size else 0.0 for c in keys]   # ap_calculator.py:466-471
            arrays[f"{size}:t{thr}:classes"] = np.array(keys, np.int64)
            arrays[f"{size}:t{thr}:ap"] = np.array([float(ap[c]) for c in keys], np.float64)
            arrays[f"{size}:t{thr}:recall"] = np.array(last, np.float64)
            print(size, thr, {c: (round(float(ap[c]), 4), round(r, 4)) for c, r in zip(keys, last)})
    print("detections per size (S, M, L, none):", np.bincount(det_size, minlength=4), "ground truth:", np.bincount(gt_size, minlength=4))
    MG.save("ap_sizes", **arrays)


if __name__ == "__main__":
    main()
