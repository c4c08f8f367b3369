"""GPU: the cuboid crop and the sampling (v-detr_amd/scene_prep.py ``crop_and_sample`` -> csrc/cuboid.hip) against
the fixture made by the reference's own loader (tests/golden/cuboid.npz) and against the numpy restatement at shapes the fixture
does not hold.

The accepted attempt, the kept rows, the kept boxes, ``choices`` and the generator's state are decisions, i.e. comparisons of
exactly defined values: identical, no tolerance.  Only the run on through ``prepare_scenes`` carries floats, with the bound of
test_gpu_scene_prep.py (the larger of 2 float32 ulps and 1e-9: DESIGN 6.4's derivation for the rotation's dot)."""
import numpy as np
import pytest
import torch

import cuboid_restatement as CR
from helpers import cfg, dev
import scene_prep_restatement as SR
from test_cuboid_restatement import CASES, batch_of, golden, state_is
from test_scene_prep_restatement import same_bits

pytestmark = pytest.mark.gpu


def run(a, randoms, num_points, min_points, **kw):
    """a batch dictionary (numpy) through crop_and_sample -> (numpy dict, the device dict)"""
    from vdetr_amd.scene_prep import crop_and_sample
    out = crop_and_sample(dev(a["points"]), a["offsets"], dev(a["boxes"]), dev(a["box_counts"]), dev(a["box_classes"]), randoms, num_points,
                          min_points=min_points, **kw)
    got = {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items() if k != "kept_rows"}
    got["kept_rows"] = [r.cpu().numpy() for r in out["kept_rows"]]
    return got, out


def assert_equal(got, want, what):
    for k in ("trial", "kept_points", "box_counts", "box_classes", "boxes", "choices"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
    assert got["choices"].dtype == np.int32 and got["boxes"].dtype == want["boxes"].dtype
    for b, (r, w) in enumerate(zip(got["kept_rows"], want["kept_rows"])):
        assert r.dtype == np.int32 and np.array_equal(r, w), (what, "kept_rows", b)


@pytest.mark.parametrize("name", CASES)
def test_device_matches_the_reference_fixture(name):
    from vdetr_amd.scene_prep import draw_augment_params, nyu40_to_class, prepare_scenes
    c = golden()[name]
    a = batch_of((name,), f64=name == "f64")
    rs = np.random.RandomState(int(c["seed"]))
    got, out = run(a, [rs], int(c["num_points"]), int(c["min_points"]))
    k = len(c["crop_boxes7"])
    assert got["trial"].tolist() == [int(c["trial"])] and got["kept_points"].tolist() == [len(c["crop_points"])]
    assert np.array_equal(got["kept_rows"][0], c["crop_rows"])
    assert got["box_counts"].tolist() == [k] and np.array_equal(got["boxes"][0, :k], c["crop_boxes7"][:, :6].astype(a["boxes"].dtype))
    assert np.array_equal(got["box_classes"][0, :k], nyu40_to_class(c["crop_boxes7"][:, 6], cfg()))
    assert not got["boxes"][0, k:].any() and not got["box_classes"][0, k:].any() and got["boxes"].shape == a["boxes"].shape
    assert np.array_equal(got["choices"][0], c["crop_rows"][c["choices"]])
    assert state_is(rs, c["state_sampled_keys"], c["state_sampled_pos"])
    cropped = dev(a["points"])[out["kept_rows"][0].long()].cpu().numpy()
    assert cropped.tobytes() == c["crop_points"].tobytes()

    # on through the augmentation and the targets: the reference's final outputs
    p = draw_augment_params(1, *c["ratios"], random=rs)
    assert state_is(rs, c["state_keys"], c["state_pos"])
    fin = prepare_scenes(dev(a["points"]), a["offsets"], out["boxes"].float(), out["box_counts"], out["box_classes"], p, cfg(),
                         choices=out["choices"])
    assert tuple(fin["point_clouds"][0].shape) == c["out_points"].shape
    worst = 0.0
    for key in SR.EXACT_KEYS:
        assert same_bits(fin[key][0].cpu().numpy(), c[key]), key
    for key, have in [(key, fin[key][0].cpu().numpy()) for key in SR.FLOAT_KEYS] + [("out_points", fin["point_clouds"][0].cpu().numpy())]:
        u = SR.ulps(have, c[key])
        u[np.abs(have.astype(np.float64) - c[key].astype(np.float64)) <= 1e-9] = 0
        worst = max(worst, float(u.max()) if u.size else 0.0)
        print(f"{name} {key}: largest difference {float(u.max()) if u.size else 0.0:.2f} float32 ulps")
        assert SR.within(have, c[key]), (key, worst)


def random_batch(seed, sizes, G, counts, f64):
    rng = np.random.default_rng(seed)
    B = len(sizes)
    boxes = np.concatenate([rng.uniform([-4, -3, 0], [4, 3, 3], (B, G, 3)), rng.uniform(0.2, 2.0, (B, G, 3))], 2)
    return {"points": rng.uniform([-4, -3, 0], [4, 3, 3], (sum(sizes), 3)).astype(np.float32), "offsets": np.cumsum([0] + list(sizes)).astype(np.int32),
            "boxes": boxes if f64 else boxes.astype(np.float32), "box_counts": np.array(counts, np.int64), "box_classes": rng.integers(0, 18, (B, G))}


def repeated_batch():
    """rows that sit exactly on a crop bound: z is one value in scene 0 (its range is 0, so every row lies on both z bounds),
    x takes four values, and half the rows are copies; scene 1 is one point 300 times (every range 0, every row inside);
    boxes centred exactly on points (on the bounds of what is kept, both ends inclusive) and away from them"""
    rng = np.random.default_rng(21)
    s0 = np.stack([rng.integers(0, 4, 400) * 0.75 - 1.0, rng.uniform(-3, 3, 400), np.full(400, 1.25)], 1).astype(np.float32)
    s0[200:] = s0[:200]
    s1 = np.tile(np.array([[0.5, -0.25, 2.0]], np.float32), (300, 1))
    s2 = rng.uniform(-1, 1, (257, 3)).astype(np.float32)
    s2[100:140] = s2[7]
    boxes = np.zeros((3, 4, 6), np.float32)
    boxes[..., 3:] = 0.5
    boxes[0, :3, :3] = [s0[5], s0[17] + np.float32(0.125), [0.5, 0.0, np.nextafter(np.float32(1.25), np.float32(2))]]
    boxes[1, :2, :3] = [s1[0], np.nextafter(s1[0], np.float32(9))]
    boxes[2, :4, :3] = [s2[7], s2[8], s2[9], s2[10]]
    return {"points": np.concatenate([s0, s1, s2]), "offsets": np.array([0, 400, 700, 957], np.int32), "boxes": boxes,
            "box_counts": np.array([3, 2, 4], np.int64), "box_classes": np.arange(12).reshape(3, 4) % 18}


@pytest.mark.parametrize("what,make,num_points,min_points", [
    ("1 / 256 / 5000 rows", lambda: random_batch(1, (1, 256, 5000), 8, (3, 0, 8), False), 300, 100),     # scene 0 falls back
    ("257 / 2 / 255 rows, float64 boxes", lambda: random_batch(2, (257, 2, 255), 5, (5, 1, 2), True), 64, 2),
    ("5000 / 1 / 257 rows", lambda: random_batch(3, (5000, 1, 257), 64, (64, 1, 0), False), 2500, 1),
    ("repeated points", repeated_batch, 128, 50)])
def test_shapes_against_the_restatement(what, make, num_points, min_points):
    a = make()
    B = len(a["offsets"]) - 1
    mine, theirs = ([np.random.RandomState(40 + b) for b in range(B)] for _ in range(2))
    got, out = run(a, mine, num_points, min_points)
    want = CR.crop_and_sample_batch(a["points"], a["offsets"], a["boxes"], a["box_counts"], a["box_classes"], theirs, num_points, min_points)
    print(what, "trial", got["trial"].tolist(), "kept", got["kept_points"].tolist(), "boxes", got["box_counts"].tolist())
    assert_equal(got, want, what)
    for m, t in zip(mine, theirs):
        assert state_is(m, *t.get_state()[1:3])
    if what == "repeated points":
        assert got["trial"][1] >= 0 and got["kept_points"][1] == 300 and got["box_counts"][1] == 1   # one point: all rows, the box on it
        assert got["trial"][0] >= 0 and got["box_counts"][0] < 3                                      # z one ulp above the plane: dropped


def test_filter_boxes_and_fewer_attempts():
    """``filter_boxes`` off keeps every box of an accepted crop; ``max_trials`` / the crop range / the aspect bound are the host's"""
    a = random_batch(4, (600, 700), 6, (6, 6), False)
    kw = dict(filter_boxes=np.array([False, True]), max_trials=7, aspect=0.9, min_crop=0.3, max_crop=0.8)
    mine, theirs = ([np.random.RandomState(50 + b) for b in range(2)] for _ in range(2))
    got, _ = run(a, mine, 100, 40, **kw)
    want = CR.crop_and_sample_batch(a["points"], a["offsets"], a["boxes"], a["box_counts"], a["box_classes"], theirs, 100, 40, **kw)
    assert_equal(got, want, "filter_boxes")
    assert got["trial"][0] >= 0 and got["box_counts"][0] == 6 and got["kept_points"][0] < 600
    for m, t in zip(mine, theirs):
        assert state_is(m, *t.get_state()[1:3])


def test_two_calls_from_equal_states_are_bit_identical():
    a = random_batch(5, (5000, 1, 700), 64, (40, 64, 0), False)
    runs = [run(a, [np.random.RandomState(60 + b) for b in range(3)], 1024, 300) for _ in range(2)]
    (first, _), (second, _) = runs
    for k in ("trial", "kept_points", "box_counts", "box_classes", "boxes", "choices"):
        assert first[k].tobytes() == second[k].tobytes(), k
    for r, s in zip(first["kept_rows"], second["kept_rows"]):
        assert r.tobytes() == s.tobytes()
    assert (first["trial"] >= 0).any()


def test_bad_arguments_are_rejected_on_the_host():
    from vdetr_amd.scene_prep import crop_and_sample
    a = random_batch(6, (10, 20), 2, (1, 2), False)
    rs = [np.random.RandomState(0), np.random.RandomState(1)]
    args = lambda **kw: [kw.get("points", dev(a["points"])), a["offsets"], kw.get("boxes", dev(a["boxes"])), dev(a["box_counts"]),  # noqa: E731
                         dev(a["box_classes"]), kw.get("randoms", rs), kw.get("num_points", 8)]
    with pytest.raises(ValueError, match="share a generator"):
        crop_and_sample(*args(randoms=[rs[0], rs[0]]), min_points=2)
    with pytest.raises(ValueError, match="share a generator"):
        crop_and_sample(*args(randoms=[np.random, np.random]), min_points=2)
    with pytest.raises(ValueError, match="generators for 2 scenes"):
        crop_and_sample(*args(randoms=rs[:1]), min_points=2)
    with pytest.raises(ValueError, match="num_points"):
        crop_and_sample(*args(num_points=0), min_points=2)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        crop_and_sample(*args(points=torch.from_numpy(a["points"])), min_points=2)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        crop_and_sample(*args(boxes=torch.from_numpy(a["boxes"])), min_points=2)
    with pytest.raises(ValueError, match="min_points"):
        crop_and_sample(*args(), min_points=0)
    with pytest.raises(ValueError, match="filter_boxes"):
        crop_and_sample(*args(), min_points=2, filter_boxes=np.array([True]))
    before = [r.get_state()[2] for r in rs]
    ok = crop_and_sample(*args(), min_points=2)
    assert ok["choices"].shape == (2, 8) and [r.get_state()[2] for r in rs] != before
