"""TEST INFRASTRUCTURE ONLY: numpy restatement of the rotated-box NMS: the reference's greedy loop
(utils/nms.py:78-162) with the overlap of boxes i and j taken from ``oracle.eval_oracle.box3d_iou`` (the restatement of the
reference's utils/box_util.py:122-147 that tests/golden/eval_det.npz pins), float64 on the float32 corners.

PINNED: tests/golden/nms3d_rot.npz holds the pairwise matrix of the reference's own ``box3d_iou`` and the keep masks of a plain
Python greedy loop over it (tools/make_rot_nms_golden.py); tests/test_oracle_nms_rot.py checks this file against them.

``nms_rotated`` skips the clip for pairs whose overlap is 0 without it: boxes whose heights do not overlap (the reference
multiplies the area by exactly 0), and boxes whose footprints' circumscribed circles are more than ``_SLACK`` apart (the clip
of two disjoint convex polygons leaves nothing, or a sliver of rounding size; either way the ratio is far below any threshold
this file accepts, see ``margin``).  ``prune=False`` is the plain loop; the CPU test compares the two.
"""
import numpy as np
from scipy.spatial import ConvexHull

from oracle import eval_oracle as EO

_SLACK = 1e-3
MARGIN = 1e-6


def box(size, yaw, center):
    """8 corners in the reference's order (upright camera frame: y is the height, corners 0-3 on top, footprint 3, 2, 1, 0
    counter-clockwise in (x, z)) as float32; ``size`` = (l, w, h)."""
    l, w, h = size
    x = np.array([l, l, -l, -l, l, l, -l, -l]) / 2
    y = np.array([h, h, h, h, -h, -h, -h, -h]) / 2
    z = np.array([w, -w, -w, w, w, -w, -w, w]) / 2
    c, s = np.cos(yaw), np.sin(yaw)
    return (np.stack([c * x + s * z, y, -s * x + c * z], 1) + np.asarray(center)).astype(np.float32)


def overlap(c1, c2, old_type=False):
    """float64 corners [8,3] -> box3d_iou(c1, c2), or for ``old_type`` the intersection volume over the volume of c2
    (nms.py:112-113 with the rotated intersection)."""
    if not old_type:
        with np.errstate(all="ignore"):
            return EO.box3d_iou(c1, c2)
    r1 = [(c1[i, 0], c1[i, 2]) for i in (3, 2, 1, 0)]
    r2 = [(c2[i, 0], c2[i, 2]) for i in (3, 2, 1, 0)]
    with np.errstate(all="ignore"):
        poly = EO.clip_polygon(r1, r2)
        area = 0.0
        if poly is not None:
            try:
                area = ConvexHull(poly).volume
            except Exception:
                area = 0.0
        inter = area * max(0.0, min(c1[0, 1], c2[0, 1]) - max(c1[4, 1], c2[4, 1]))
        return inter / EO.box3d_vol(c2)


def iou_matrix(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array([[overlap(x, y) for y in b] for x in a]).reshape(len(a), len(b))


def nms_rotated(corners, score, cls=None, valid=None, thr=0.25, old_type=False, prune=True):
    """corners [K,8,3] float32, score [K], cls [K] or None (class-agnostic), valid [K] bool or None -> (keep [K] bool,
    margin): the greedy loop over a STABLE ascending arg-sort of the score, taken from its end; ``margin`` is the smallest
    ``|overlap - thr|`` over every pair the loop evaluated (``inf`` if none): a scene is a fair test of a float64
    implementation only if it is well above float64 rounding, and callers assert ``margin >= MARGIN``."""
    c = np.asarray(corners, np.float32).astype(np.float64)
    K = len(c)
    assert thr >= MARGIN
    idx = np.arange(K) if valid is None else np.nonzero(np.asarray(valid))[0]
    remaining = idx[np.argsort(np.asarray(score)[idx], kind="stable")]
    centre = c[:, :4][:, :, [0, 2]].mean(1)
    radius = np.sqrt(((c[:, :4][:, :, [0, 2]] - centre[:, None]) ** 2).sum(-1)).max(1)
    keep = np.zeros(K, bool)
    margin = np.inf
    while remaining.size:
        i = remaining[-1]
        keep[i] = True
        rest = remaining[:-1]
        cand = np.ones(rest.size, bool) if cls is None else (np.asarray(cls)[rest] == cls[i])
        if prune:
            cand &= np.minimum(c[i, 0, 1], c[rest, 0, 1]) - np.maximum(c[i, 4, 1], c[rest, 4, 1]) > 0
            cand &= np.sqrt(((centre[rest] - centre[i]) ** 2).sum(-1)) <= radius[rest] + radius[i] + _SLACK
            if cand.size - cand.sum():
                margin = min(margin, thr)           # the pruned pairs overlap by 0
        dead = np.zeros(rest.size, bool)
        for n in np.nonzero(cand)[0]:
            o = overlap(c[i], c[rest[n]], old_type)
            dead[n] = o > thr
            if np.isfinite(o):
                margin = min(margin, abs(o - thr))
        remaining = rest[~dead]
    return keep, margin
