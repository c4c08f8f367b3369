"""numpy restatement of the per-point steps around the cuboid crop: what datasets/scannet.py:436-464 and
:544-560 of the reference do to a loaded scan's colours and height, drawing from a legacy generator in the reference's order.
tests/test_color_aug_restatement.py holds it against tests/golden/color_aug.npz (made by the reference's own loader,
tools/make_color_aug_golden.py) bit for bit, generator state included; the GPU tests use it for ragged batches.

The dtypes are the point.  The cloud is float32.  The drop and the contrast stay in float32 (their operands are a bool vector,
float32 reductions and Python floats); the jitter adds a float64 array, so the sum and the clip are float64 and the assignment
rounds once; hue and saturation run in float64 on a copy and come back through uint8; the SUN RGB-D steps alternate: a Python
float operand keeps float32, a float64 array operand makes the step float64 and the in-place store rounds it."""
import numpy as np

import cuboid_restatement as CR
import scene_prep_restatement as SR

SETTINGS = dict(color_drop=0.0, color_contrastp=0.0, color_jitterp=0.0, hue_sat="0_0_0", coloraug_sunrgbd=False, use_height=False,
                color_mean=-1.0, use_random_cuboid=False, min_points=0, num_points=0, ratios=(5.0, 0.4, 0.4))
JITTER_STD = 0.005


def unit_remainder(a):
    """np.remainder(a, 1.0) spelled out: C fmod, then the sign of the divisor; a zero result is +0"""
    m = np.fmod(a, 1.0)
    m = np.where(m < 0, m + 1.0, m)
    return np.where(m == 0, 0.0, m)


def to_hsv(rgb):
    """float64 [n,3] -> hue in sixths-of-a-turn units folded to [0, 1], saturation, value (colorsys, vectorised)"""
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    top, bottom = np.max(rgb, 1), np.min(rgb, 1)
    coloured = top != bottom
    span = np.where(coloured, top - bottom, 1.0)
    sat = np.where(coloured, (top - bottom) / np.where(coloured, top, 1.0), 0.0)
    rc, gc, bc = (np.where(coloured, (top - ch) / span, 0.0) for ch in (r, g, b))
    hue = np.where(r == top, bc - gc, np.where(g == top, 2.0 + rc - bc, 4.0 + gc - rc))
    return unit_remainder(hue / 6.0), sat, top


def sextant_of(hue):
    """(uint8 sextant before the % 6, fraction within it) of a hue in [0, 1]"""
    six = hue * 6.0
    whole = six.astype(np.uint8)
    return whole, six - whole


def from_hsv(hue, sat, val):
    """-> uint8 [n,3] (colorsys.hsv_to_rgb, the grey case first, truncation at the end)"""
    whole, frac = sextant_of(hue)
    p, q, t = val * (1.0 - sat), val * (1.0 - sat * frac), val * (1.0 - sat * (1.0 - frac))
    which = whole % 6
    table = {0: (val, t, p), 1: (q, val, p), 2: (p, val, t), 3: (p, q, val), 4: (t, p, val), 5: (val, p, q)}
    out = np.empty((len(hue), 3))
    for k in range(3):
        col = table[0][k].copy()
        for i in range(1, 6):
            col = np.where(which == i, table[i][k], col)
        out[:, k] = np.where(sat == 0.0, val, col)
    return out.astype(np.uint8)


def color_augment_scene(cloud, random, color_drop=0.0, color_contrastp=0.0, color_jitterp=0.0, hue_sat="0_0_0", **_):
    """cloud float32 [n,6+] -> (a copy with columns 3:6 augmented, what happened: the gates and the intermediate facts the
    fixture's cases are asserted from)"""
    cloud = np.array(cloud, np.float32)
    rgb = cloud[:, 3:6]
    n = len(cloud)
    seen = {"dropped": 0, "contrast": False, "jitter": False, "hue": False, "nan_channels": 0, "clipped_low": 0, "clipped_high": 0}
    with np.errstate(all="ignore"):
        if color_drop > 0:
            keep = random.random(n) > color_drop
            rgb *= keep[:, None]
            seen["dropped"] = int((~keep).sum())
        if color_contrastp > 0 and random.random() < color_contrastp:
            low, high = rgb.min(0, keepdims=True), rgb.max(0, keepdims=True)
            stretch = 255 / (high - low)                               # float32: a Python int with a float32 array
            seen["constant_channels"] = int((high == low).sum())
            stretched = (rgb - low) * stretch
            b = random.random()
            rgb[:] = (1 - b) * rgb + b * stretched                     # Python floats: rounded to float32, float32 products and sum
            seen["contrast"] = True
            seen["nan_channels"] = int(np.isnan(rgb).all(0).sum())
        if color_jitterp > 0 and random.random() < color_jitterp:
            noise = random.randn(n, 3)
            noise *= JITTER_STD * 255
            moved = noise + rgb                                        # float64
            seen["clipped_low"], seen["clipped_high"] = int((moved < 0).sum()), int((moved > 255).sum())
            rgb[:] = np.clip(moved, 0, 255)
            seen["jitter"] = True
        hue_max, sat_max, hue_p = (float(v) for v in hue_sat.split("_"))
        if hue_p > 0 and random.random() < hue_p:
            hue, sat, val = to_hsv(rgb.astype(np.float64))
            turn = (random.random() - 0.5) * 2 * hue_max
            ratio = 1 + (random.random() - 0.5) * 2 * sat_max
            raw = turn + hue + 1
            hue2 = unit_remainder(raw)
            sat2 = np.clip(ratio * sat, 0, 1)
            seen.update(hue=True, sextants=sorted(set((sextant_of(hue2)[0][sat2 != 0] % 6).tolist())), grey=int((sat2 == 0).sum()),
                        wrapped=int((raw >= 2).sum() + (raw < 1).sum()))
            rgb[:] = from_hsv(hue2, sat2, val)
    return cloud, seen


def percentile_099(z):
    """np.percentile(z, 0.99) of a float32 vector, method "linear", as numpy 2.2 computes it: the quantile and the virtual
    index are float32 ((n - 1) * (float32(0.99) / float32(100))), the two neighbours are order statistics and the interpolation
    is numpy's two-sided lerp in float32.  A NaN anywhere gives NaN."""
    z = np.sort(np.asarray(z, np.float32))                             # NaN sorts to the end
    n = len(z)
    if np.isnan(z[-1]):
        return np.float32(np.nan)
    at = np.float32(n - 1) * (np.float32(0.99) / np.float32(100))
    below = int(np.floor(at))
    if at >= n - 1:
        return z[n - 1]
    a, b, w = z[below], z[below + 1], np.float32(np.float64(at) - below)
    with np.errstate(all="ignore"):
        return b - (b - a) * (np.float32(1) - w) if w >= 0.5 else a + (b - a) * w


def append_height_scene(cloud):
    cloud = np.asarray(cloud, np.float32)
    with np.errstate(all="ignore"):
        return np.concatenate([cloud, (cloud[:, 2] - percentile_099(cloud[:, 2]))[:, None]], 1)


def sunrgbd_scene(cloud, random):
    """scannet.py:545-560 on a float32 cloud whose colours are normalised; in place, returns what it drew"""
    rgb = cloud[:, 3:6]
    n = len(cloud)
    rgb += 0.5
    gain = 1 + 0.4 * random.random(3) - 0.2
    rgb *= gain
    shift = 0.1 * random.random(3) - 0.05
    rgb += shift
    wobble = 0.05 * random.random(n) - 0.025
    rgb += wobble[:, None]
    rgb[:] = np.clip(rgb, 0, 1)
    keep = random.random(n) > 0.3
    rgb *= keep[:, None]
    rgb -= 0.5
    return gain, shift, wobble, keep


def draw_pose(random, rot_ratio, trans_ratio, scale_ratio):
    """scannet.py:516-540: -> flip_x, flip_y, angle, translation, scale"""
    fx, fy = random.random() > 0.5, random.random() > 0.5
    angle = ((random.random() * np.pi / 18) - np.pi / 36) * rot_ratio / 5.0
    trans = (random.random(size=3) - 0.5) * trans_ratio / 0.5 if trans_ratio > 0.0 else np.zeros(3)
    scale = 1 + (random.random() - 0.5) * scale_ratio / 0.5 if scale_ratio > 0.0 else 1.0
    return fx, fy, angle, trans, scale


def loader_scene(vert, boxes7, random, s):
    """the reference's ``__getitem__`` from the loaded arrays to ``point_clouds`` for the settings ``s`` (a dict with SETTINGS'
    keys) -> (point_clouds float32, what the colour step saw)"""
    cloud, seen = color_augment_scene(vert[:, :6], random, **s)
    if s["use_height"]:
        cloud = append_height_scene(cloud)
    boxes = np.asarray(boxes7)[:, :6]
    choices = None
    if s["use_random_cuboid"]:
        got = CR.crop_and_sample_scene(cloud, boxes7, random, int(s["num_points"]), int(s["min_points"]))
        choices, boxes = got["rows"], np.asarray(boxes7)[got["keep_boxes"], :6]
    pose = draw_pose(random, *s["ratios"])
    out = SR.prepare_scene(cloud, boxes.astype(np.float32), np.zeros(len(boxes), np.int64), *pose, np.zeros((1, 3)), choices=choices,
                           color_mean=float(s["color_mean"]))["point_clouds"]
    if s["coloraug_sunrgbd"]:
        sunrgbd_scene(out, random)
    return out, seen
