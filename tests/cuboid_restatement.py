"""numpy restatement of the cuboid crop and the sampling after it: what utils/random_cuboid.py:38-98 and
pc_util.random_sampling of the reference compute for one loaded scan at datasets/scannet.py:476-498, drawing from the generator
it is given.  tests/test_cuboid_restatement.py holds it against tests/golden/cuboid.npz (made by the reference's own loader,
tools/make_cuboid_golden.py) bit for bit, the generator's state included; the GPU tests use it at shapes the fixture lacks.

The dtypes are the point: the cloud is float32 and so is its range; the crop ranges are float64, so the half extents, the
bounds and the comparisons with the rows are float64; the boxes are compared in their own dtype with the float32 bounds of the
kept rows.  Beyond the reference's results it reports every attempt it went through (``attempts``), which is what the fixture
tool records from the reference by counting its calls."""
import numpy as np

ASPECT_REJECTED, COUNT_REJECTED, BOX_REJECTED, ACCEPTED = "aspect", "count", "box", "accepted"


def crop_and_sample_scene(points, boxes, random, num_points, min_points, aspect=0.8, min_crop=0.5, max_crop=1.0, max_trials=100,
                          filter_boxes=None):
    """points float32 [n,3+C]; boxes [g,6+] of the PRESENT boxes in the file's dtype; ``random``: ``np.random`` or a RandomState
    -> dict: ``trial`` (-1: fallback), ``kept_rows`` ascending int64, ``cloud`` = points[kept_rows], ``keep_boxes`` bool [g],
    ``choices`` (rows of the crop), ``rows`` = kept_rows[choices] (rows of the scan), ``attempts`` (the fate of each one gone
    through, with the count where it got that far)."""
    points = np.asarray(points)
    xyz = points[:, 0:3]
    n, g = len(points), len(boxes)
    if filter_boxes is None:
        filter_boxes = g > 0
    span = xyz.max(0) - xyz.min(0)
    out = {"trial": -1, "kept_rows": np.arange(n), "keep_boxes": np.ones(g, bool), "attempts": []}
    for t in range(max_trials):
        crop = min_crop + random.rand(3) * (max_crop - min_crop)
        faces = [crop[[0, 1]], crop[[0, 2]], crop[[1, 2]]]
        if not any(f.min() / f.max() >= aspect for f in faces):
            out["attempts"].append((ASPECT_REJECTED, -1))
            continue
        centre = xyz[random.choice(n)]
        half = span * crop / 2.0
        hi, lo = centre + half, centre - half
        inside = (xyz <= hi).all(1) & (xyz >= lo).all(1)
        count = int(inside.sum())
        if count < min_points:
            out["attempts"].append((COUNT_REJECTED, count))
            continue
        keep = np.ones(g, bool)
        if filter_boxes:
            kept_lo, kept_hi = xyz[inside].min(0), xyz[inside].max(0)
            keep = (boxes[:, 0:3] >= kept_lo).all(1) & (boxes[:, 0:3] <= kept_hi).all(1)
            if not keep.any():
                out["attempts"].append((BOX_REJECTED, count))
                continue
        out["attempts"].append((ACCEPTED, count))
        out.update(trial=t, kept_rows=np.flatnonzero(inside), keep_boxes=keep)
        break
    out["cloud"] = points[out["kept_rows"]]
    kept = len(out["kept_rows"])
    out["choices"] = random.choice(kept, num_points, replace=kept < num_points)
    out["rows"] = out["kept_rows"][out["choices"]]
    return out


def crop_and_sample_batch(points, offsets, boxes, box_counts, box_classes, randoms, num_points, min_points, filter_boxes=None, **kw):
    """the batch form with ``crop_and_sample``'s arguments as numpy arrays -> its results as numpy arrays"""
    B = len(offsets) - 1
    ret = {"choices": np.zeros((B, num_points), np.int32), "boxes": np.zeros_like(boxes), "box_counts": np.zeros(B, np.int64),
           "box_classes": np.zeros_like(box_classes), "trial": np.zeros(B, np.int64), "kept_points": np.zeros(B, np.int64),
           "kept_rows": []}
    for b in range(B):
        g = int(box_counts[b])
        s = crop_and_sample_scene(points[offsets[b]:offsets[b + 1]], boxes[b, :g], randoms[b], num_points, min_points,
                                  filter_boxes=None if filter_boxes is None else bool(filter_boxes[b]), **kw)
        k = int(s["keep_boxes"].sum())
        ret["choices"][b], ret["trial"][b], ret["kept_points"][b] = s["rows"], s["trial"], len(s["kept_rows"])
        ret["boxes"][b, :k], ret["box_classes"][b, :k], ret["box_counts"][b] = boxes[b, :g][s["keep_boxes"]], box_classes[b, :g][s["keep_boxes"]], k
        ret["kept_rows"].append(s["kept_rows"])
    return ret
