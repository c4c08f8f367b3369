"""GPU: the colour augmentations, the height channel and the SUN RGB-D colour step (v-detr_amd/scene_prep.py ``augment_colors`` /
``append_height`` / ``sunrgbd_color_augment`` -> csrc/color_aug.hip) against the fixture made by the reference's own
loader (tests/golden/color_aug.npz) and against the numpy restatement, per scan and as one ragged batch.

Every operation is an IEEE basic operation on exactly defined inputs, so colours and heights are compared with NO tolerance
(NaN positions included).  Only the xyz columns of the run on through ``prepare_scenes`` carry the bound of
test_gpu_cuboid.py / test_gpu_scene_prep.py (the larger of 2 float32 ulps and 1e-9: DESIGN 6.4's derivation for the rotation's dot)."""
import numpy as np
import pytest
import torch

import color_aug_restatement as CA
from helpers import cfg, dev
import scene_prep_restatement as SR
from test_color_aug_restatement import CASES, COLOR_CASES, golden, settings_of, state_is

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 64


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def draw(n, rs, s):
    from vdetr_amd.scene_prep import draw_color_augment
    return draw_color_augment(n, rs, color_drop=s["color_drop"], color_contrastp=s["color_contrastp"], color_jitterp=s["color_jitterp"],
                              hue_sat=s["hue_sat"])


def device_loader(vert, boxes7, rs, s):
    """the whole device chain for one scan on one generator -> the final ``point_clouds`` (numpy)"""
    from vdetr_amd import scene_prep as SP
    n = len(vert)
    off = np.array([0, n])
    pts = SP.augment_colors(dev(vert[:, :6]), off, [draw(n, rs, s)])
    if s["use_height"]:
        pts = SP.append_height(pts, off)
    boxes = np.zeros((1, G, 6))
    classes = np.zeros((1, G), np.int64)
    boxes[0, :len(boxes7)], classes[0, :len(boxes7)] = boxes7[:, :6], SP.nyu40_to_class(boxes7[:, 6], cfg())
    boxes, counts, classes, choices = dev(boxes), dev(np.array([len(boxes7)])), dev(classes), None
    if s["use_random_cuboid"]:
        out = SP.crop_and_sample(pts, off, boxes, counts, classes, [rs], int(s["num_points"]), min_points=int(s["min_points"]))
        boxes, counts, classes, choices = out["boxes"], out["box_counts"], out["box_classes"], out["choices"]
    pose = SP.draw_augment_params(1, *s["ratios"], random=rs)
    fin = SP.prepare_scenes(pts, off, boxes.float(), counts, classes, pose, cfg(), choices=choices, color_mean=float(s["color_mean"]))
    if s["coloraug_sunrgbd"]:
        rows = len(fin["point_clouds"][0])
        SP.sunrgbd_color_augment(fin["point_clouds"], np.array([0, rows]), [SP.draw_sunrgbd_color(rows, rs)])
    return fin["point_clouds"][0].cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_device_chain_matches_the_reference_fixture(name):
    """draw_color_augment -> augment_colors -> [append_height] -> [crop_and_sample] -> draw_augment_params -> prepare_scenes ->
    [sunrgbd_color_augment] on one generator against the reference loader's final cloud and generator state"""
    c = golden()[name]
    s = settings_of(c)
    rs = np.random.RandomState(int(c["seed"]))
    got = device_loader(c["vert"], c["boxes7"], rs, s)
    want = c["out_points"]
    assert got.shape == want.shape
    assert same(got[:, 3:], want[:, 3:]), (name, int((~((got[:, 3:] == want[:, 3:]) | np.isnan(want[:, 3:]))).sum()))
    u = SR.ulps(got[:, :3], want[:, :3])
    print(f"{name} xyz: largest difference {float(u.max()):.2f} float32 ulps")
    assert SR.within(got[:, :3], want[:, :3])
    assert state_is(rs, c["state_keys"], c["state_pos"])


def ragged(names):
    g = golden()
    verts = [g[n]["vert"] for n in names]
    return np.concatenate(verts), np.cumsum([0] + [len(v) for v in verts]).astype(np.int32)


def test_ragged_batch_of_every_scan_equals_the_restatement():
    """one batch of all the fixture's scans, each with its own settings and generator: colours, then heights"""
    from vdetr_amd.scene_prep import append_height, augment_colors
    g = golden()
    points, off = ragged(COLOR_CASES)
    wide = np.concatenate([points, np.arange(len(points) * 2, dtype=np.float32).reshape(-1, 2)], 1)   # two more channels: W = 8
    mine = [np.random.RandomState(int(g[n]["seed"])) for n in COLOR_CASES]
    params = [draw(len(g[n]["vert"]), r, settings_of(g[n])) for n, r in zip(COLOR_CASES, mine)]
    src = dev(wide)
    out = augment_colors(src, off, params)
    assert src.cpu().numpy().tobytes() == wide.tobytes()              # the input is left alone
    got = out.cpu().numpy()
    assert got[:, :3].tobytes() == wide[:, :3].tobytes() and got[:, 6:].tobytes() == wide[:, 6:].tobytes()
    for b, n in enumerate(COLOR_CASES):
        theirs = np.random.RandomState(int(g[n]["seed"]))
        want, _ = CA.color_augment_scene(g[n]["vert"], theirs, **settings_of(g[n]))
        assert same(got[off[b]:off[b + 1], 3:6], want[:, 3:6]), n
        assert state_is(mine[b], *theirs.get_state()[1:3]), n
    assert np.isnan(got[:, 3:6]).any()                                 # the 255 / 0 channel is in the batch
    assert augment_colors(src, off, params).cpu().numpy().tobytes() == got.tobytes()      # two runs: the same bits

    tall = append_height(out, off)
    high = tall.cpu().numpy()
    assert high.shape == (len(points), 9) and high[:, :8].tobytes() == got.tobytes()
    for b, n in enumerate(COLOR_CASES):
        want = CA.append_height_scene(g[n]["vert"])[:, -1]
        assert same(high[off[b]:off[b + 1], 8], want), n
    assert append_height(out, off).cpu().numpy().tobytes() == high.tobytes()


def test_sunrgbd_step_on_a_ragged_batch_in_place():
    from vdetr_amd.scene_prep import draw_sunrgbd_color, sunrgbd_color_augment
    rng = np.random.default_rng(5)
    sizes = (1, 255, 256, 257, 700)
    off = np.cumsum((0,) + sizes).astype(np.int32)
    cloud = rng.uniform(-0.5, 0.5, (off[-1], 7)).astype(np.float32)
    cloud[3, 4], cloud[300, 3] = np.nan, np.inf
    mine, theirs = ([np.random.RandomState(70 + b) for b in range(len(sizes))] for _ in range(2))
    want = cloud.copy()
    with np.errstate(all="ignore"):
        for b, r in enumerate(theirs):
            CA.sunrgbd_scene(want[off[b]:off[b + 1]], r)
    packed = dev(cloud)
    views = list(torch.split(packed, list(sizes)))
    back = sunrgbd_color_augment(views, off, [draw_sunrgbd_color(n, r) for n, r in zip(sizes, mine)])
    assert back is views
    got = packed.cpu().numpy()
    assert same(got, want) and np.isnan(got[3, 4])
    assert got[:, :3].tobytes() == cloud[:, :3].tobytes() and got[:, 6].tobytes() == cloud[:, 6].tobytes()
    for m, t in zip(mine, theirs):
        assert state_is(m, *t.get_state()[1:3])
    again = dev(cloud)                                                 # the packed tensor itself, the same draws: the same bits
    sunrgbd_color_augment(again, off, [draw_sunrgbd_color(n, np.random.RandomState(70 + b)) for b, n in enumerate(sizes)])
    assert again.cpu().numpy().tobytes() == got.tobytes()


def height_batch():
    """columns that try the select: several tiles of 1024 rows, repeated values across the two statistics, both signs, both
    zeros, infinities, a NaN (the floor is NaN), one and two rows"""
    rng = np.random.default_rng(9)
    sizes = (1, 2, 1024, 1025, 4097, 300, 777, 5000)
    off = np.cumsum((0,) + sizes).astype(np.int32)
    cloud = rng.uniform(-3, 3, (off[-1], 4)).astype(np.float32)
    z = [cloud[off[b]:off[b + 1], 2] for b in range(len(sizes))]
    z[3][:] = np.round(z[3])                                           # seven values, many copies of each
    z[4][:4] = [-np.inf, np.inf, 0.0, -0.0]
    z[4][4:60] = -2.999                                                # the statistics 40 and 41 sit inside a run of copies
    z[5][17] = np.nan
    z[6][:] = -np.abs(z[6])                                            # negative keys only
    z[7][:] = np.float32(1.5)                                          # one value
    return cloud, off


def test_height_select_against_the_restatement_and_numpy():
    from vdetr_amd.scene_prep import append_height
    cloud, off = height_batch()
    src = dev(cloud)
    got = append_height(src, off).cpu().numpy()
    assert src.cpu().numpy().tobytes() == cloud.tobytes() and got[:, :4].tobytes() == cloud.tobytes()
    with np.errstate(all="ignore"):
        for b in range(len(off) - 1):
            part = cloud[off[b]:off[b + 1]]
            want = part[:, 2] - np.percentile(part[:, 2], 0.99)
            assert want.dtype == np.float32
            assert same(got[off[b]:off[b + 1], 4], want), b
            assert same(CA.append_height_scene(part)[:, 4], want), b
    assert np.isnan(got[off[5]:off[6], 4]).all()
    assert append_height(src, off).cpu().numpy().tobytes() == got.tobytes()


def test_no_scenes_and_bad_arguments():
    from vdetr_amd.scene_prep import append_height, augment_colors, draw_color_augment, draw_sunrgbd_color, sunrgbd_color_augment
    none = torch.zeros((0, 6), device=DEV)
    off0 = np.array([0])
    assert tuple(augment_colors(none, off0, []).shape) == (0, 6) and tuple(append_height(none, off0).shape) == (0, 7)
    assert sunrgbd_color_augment(none, off0, []) is none and sunrgbd_color_augment([], off0, []) == []
    rs = np.random.RandomState(0)
    cloud, off = torch.zeros((10, 6), device=DEV), np.array([0, 4, 10])
    with pytest.raises(ValueError, match="one ColorAugmentParams per scene"):
        augment_colors(cloud, off, [draw_color_augment(4, rs), draw_color_augment(5, rs)])
    with pytest.raises(ValueError, match="one SunrgbdColorParams per scene"):
        sunrgbd_color_augment(cloud, off, [draw_sunrgbd_color(4, rs)])
    with pytest.raises(ValueError, match="columns"):
        augment_colors(cloud[:, :5].contiguous(), off, [draw_color_augment(4, rs), draw_color_augment(6, rs)])
    with pytest.raises(ValueError, match="no points"):
        append_height(cloud, np.array([0, 0, 10]))
    with pytest.raises(ValueError, match="consecutive row blocks"):
        sunrgbd_color_augment([cloud[4:], cloud[:4]], np.array([0, 6, 10]), [draw_sunrgbd_color(6, rs), draw_sunrgbd_color(4, rs)])
