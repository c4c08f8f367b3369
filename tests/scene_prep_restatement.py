"""numpy restatement of the scene preparation: what datasets/scannet.py:510-626 of the reference computes for
one loaded scan, with the augmentation parameters handed in instead of drawn.  tests/test_scene_prep_restatement.py holds it
against tests/golden/scene_prep.npz (made by the reference itself, tools/make_scene_prep_golden.py) bit for bit; the GPU tests
use it at shapes the fixture does not hold.

The dtypes are the point.  A cloud is float32; it takes the rotation and the translation in float64 (their operands are
float64 arrays), rounded back on assignment, and the scale in float32 (its operand is a Python float); the boxes are float32
up to the rotation, float64 from there to the outputs; normalisation runs in float32; the corners are float64 sums of
float32 halves and centres.  Nothing here is one composed affine map."""
import numpy as np

MEAN_COLOR_RGB = np.array([109.8, 97.2, 83.8])
FLOAT_KEYS = ("gt_box_corners", "gt_box_centers", "gt_box_centers_normalized", "gt_box_sizes", "gt_box_sizes_normalized",
              "gt_box_sizes_residual_label", "point_cloud_dims_min", "point_cloud_dims_max")
EXACT_KEYS = ("gt_angle_class_label", "gt_angle_residual_label", "gt_box_angles", "gt_box_sem_cls_label", "gt_box_present")
DTYPES = {k: np.float32 for k in FLOAT_KEYS + EXACT_KEYS}
DTYPES.update(gt_angle_class_label=np.int64, gt_box_sem_cls_label=np.int64)


def rotz(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def colours(cloud, color_mean):
    """columns 3:6 of a float32 cloud, in place: None keeps them, negative centres on the mean colour in float64, otherwise
    [0, 255] -> [-0.5, 0.5] in float32 (a float32 array divided by a Python float stays float32)"""
    if color_mean is None:
        return
    if color_mean < 0:
        cloud[:, 3:6] = (cloud[:, 3:6] - MEAN_COLOR_RGB) / 256.0
    else:
        cloud[:, 3:6] = cloud[:, 3:6] / 255.0 - 0.5


def hull_of_turned_boxes(boxes, rot):
    """float32 [M,6] centre + size, turned about z -> float64 [M,6]: turned centres, twice the largest turned half-extent
    corner in x and y, z size unchanged"""
    centres = np.dot(boxes[:, 0:3], rot.T)
    hx, hy = boxes[:, 3] / 2.0, boxes[:, 4] / 2.0
    ex, ey = np.zeros((len(boxes), 4)), np.zeros((len(boxes), 4))
    for i, (sx, sy) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
        corner = np.zeros((len(boxes), 3))
        corner[:, 0], corner[:, 1] = sx * hx, sy * hy
        corner = np.dot(corner, rot.T)
        ex[:, i], ey[:, i] = corner[:, 0], corner[:, 1]
    return np.concatenate([centres, np.stack((2.0 * ex.max(1), 2.0 * ey.max(1), boxes[:, 5]), 1)], 1)


def corners_at_angle_zero(centres, sizes):
    """float32 [M,3] each -> float64 [M,8,3] in the camera frame (x, -z, y): with a zero heading the rotation of
    get_3d_box_batch_np is the identity, so a corner is the float64 sum of a signed float32 half size and the centre"""
    cam = centres.copy()
    cam[:, [0, 1, 2]] = cam[:, [0, 2, 1]]
    cam[:, 1] *= -1
    l2, w2, h2 = sizes[:, 0:1] / 2, sizes[:, 1:2] / 2, sizes[:, 2:3] / 2
    c = np.zeros((len(centres), 8, 3))
    c[:, :, 0] = np.concatenate((l2, l2, -l2, -l2, l2, l2, -l2, -l2), 1)
    c[:, :, 1] = np.concatenate((h2, h2, h2, h2, -h2, -h2, -h2, -h2), 1)
    c[:, :, 2] = np.concatenate((w2, -w2, -w2, w2, w2, -w2, -w2, w2), 1)
    c += cam[:, None, :]
    return c


def prepare_scene(points, boxes, classes, flip_x, flip_y, rot_angle, trans, scale, mean_size, max_obj=64, choices=None,
                  color_mean=None, augment=True):
    """points float32 [n,3+C]; boxes float32 [g,6] and classes [g] of the PRESENT boxes -> dict with ``point_clouds`` [n',3+C]
    and every tensor of a scene.  ``augment=False`` skips the whole block as the evaluation split does (identity parameters
    through the block give the same values)."""
    cloud = np.array(points, np.float32)
    colours(cloud, color_mean)
    if choices is not None:
        cloud = cloud[np.asarray(choices)]
    g = len(boxes)
    tb = np.zeros((max_obj, 6), np.float32)
    present = np.zeros(max_obj, np.float32)
    tb[:g], present[:g] = boxes, 1
    if augment:
        if flip_x:
            cloud[:, 0], tb[:, 0] = -1 * cloud[:, 0], -1 * tb[:, 0]
        if flip_y:
            cloud[:, 1], tb[:, 1] = -1 * cloud[:, 1], -1 * tb[:, 1]
        rot = rotz(rot_angle)
        cloud[:, 0:3] = np.dot(cloud[:, 0:3], rot.T)                   # float64 product, float32 on assignment
        tb = hull_of_turned_boxes(tb, rot)                             # float64 from here on
        trans = np.asarray(trans, np.float64)
        cloud[:, 0:3] = cloud[:, 0:3] + trans
        tb[:, 0:3] = tb[:, 0:3] + trans
        # the reference's scale is a Python float: numpy keeps a float32 array times a Python float in float32 (the scalar is
        # rounded to float32 first), while the float64 boxes stay float64
        cloud[:, 0:3] = cloud[:, 0:3] * float(scale)
        tb[:, :] = tb * float(scale)
    sizes = tb[:, 3:6]
    lo, hi = cloud.min(0)[:3], cloud.max(0)[:3]
    centres = tb.astype(np.float32)[:, 0:3]
    sizes32 = sizes.astype(np.float32)
    with np.errstate(all="ignore"):                                    # a one-point scene has no extent: inf and nan, as there
        one, zero = np.ones((1, 3), np.float32), np.zeros((1, 3), np.float32)
        cn = ((centres - lo[None]) * (one - zero)) / (hi[None] - lo[None]) + zero
        cn = cn * present[:, None]
        sn = sizes32 * (1.0 / (hi - lo))[None]
    cls = np.zeros(max_obj, np.int64)
    cls[:g] = classes
    residual = np.zeros((max_obj, 3), np.float32)
    residual[:g] = sizes[:g] - np.asarray(mean_size)[cls[:g]]
    zeros = np.zeros(max_obj, np.float32)
    return {"point_clouds": cloud, "point_cloud_dims_min": lo, "point_cloud_dims_max": hi,
            "gt_box_corners": corners_at_angle_zero(centres, sizes32).astype(np.float32), "gt_box_centers": centres,
            "gt_box_centers_normalized": cn.astype(np.float32), "gt_angle_class_label": np.zeros(max_obj, np.int64),
            "gt_angle_residual_label": zeros, "gt_box_sem_cls_label": cls, "gt_box_present": present, "gt_box_sizes": sizes32,
            "gt_box_sizes_normalized": sn.astype(np.float32), "gt_box_sizes_residual_label": residual, "gt_box_angles": zeros.copy()}


def prepare_batch(points, offsets, boxes, box_counts, box_classes, params, mean_size, max_obj=64, choices=None, color_mean=None,
                  augment=True):
    """the batch form with ``prepare_scenes``' arguments as numpy arrays -> the same dict (``point_clouds`` a list)"""
    scenes = []
    for b in range(len(offsets) - 1):
        n = int(box_counts[b])
        scenes.append(prepare_scene(points[offsets[b]:offsets[b + 1]], boxes[b, :n], box_classes[b, :n], params.flip_x[b], params.flip_y[b],
                                    params.rot_angle[b], params.trans[b], params.scale[b], mean_size, max_obj,
                                    None if choices is None else choices[b], color_mean, augment))
    out = {k: np.stack([s[k] for s in scenes]) for k in scenes[0] if k != "point_clouds"}
    out["point_clouds"] = [s["point_clouds"] for s in scenes]
    return out


def ulps(got, want):
    """|got - want| in float32 ulps of ``want`` where both are finite, with the absolute floor of the tests taken off first;
    positions where either is not finite must agree exactly (reported as inf otherwise)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    fin = np.isfinite(want) & np.isfinite(got)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    out = np.where(same, 0.0, np.inf)
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    out[fin] = diff[fin] / np.spacing(np.abs(want[fin])).astype(np.float64)
    return out


def within(got, want, nulp=2, floor=1e-9):
    """the tolerance of the device tests: the larger of ``nulp`` float32 ulps of the reference value and ``floor`` absolute;
    inf / nan must sit at the same places"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    fin = np.isfinite(want)
    if not np.array_equal(got[~fin], want[~fin], equal_nan=True) or not np.isfinite(got[fin]).all():
        return False
    diff = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    return bool((diff <= np.maximum(nulp * np.spacing(np.abs(want[fin])).astype(np.float64), floor)).all())
