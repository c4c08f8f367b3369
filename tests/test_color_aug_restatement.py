"""CPU: the numpy restatement of the colour augmentations, the height channel and the SUN RGB-D colour step
(tests/color_aug_restatement.py) against the fixture that the reference's own loader produced (tests/golden/color_aug.npz,
tools/make_color_aug_golden.py), bit for bit and with the generator's state; the host draws of ``scene_prep`` against the same
states; and the cases the fixture has to hold, re-asserted so that a regenerated file cannot lose one."""
import os

import numpy as np
import pytest

import color_aug_restatement as CA
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "color_aug.npz")
CASES = ("drop", "contrast", "contrast_off", "jitter", "jitter_off", "hue", "hue_off", "all", "nan", "sunrgbd", "all_sunrgbd", "height1",
         "height2", "height101", "height257", "chain")
COLOR_CASES = tuple(c for c in CASES if c != "chain")                  # the cloud keeps every row, in order
_cache = {}


def golden():
    """-> {case name: {key: array}}; loaded once"""
    if not _cache:
        z = np.load(GOLDEN)
        for name in z["cases"]:
            _cache[str(name)] = {k.split(":", 1)[1]: z[k] for k in z.files if k.startswith(f"{name}:")}
    return _cache


def settings_of(c):
    s = {k: c[f"set_{k}"].item() if c[f"set_{k}"].ndim == 0 else tuple(c[f"set_{k}"].tolist()) for k in CA.SETTINGS}
    return s


def state_is(random, keys, pos):
    s = random.get_state()
    return np.array_equal(s[1], keys) and s[2] == int(pos)


def cases_present(name, c, s):
    """the case ``name`` of the fixture holds what DESIGN.md 6.5 says it holds, judged from the reference's own stream"""
    _, t = CA.color_augment_scene(c["vert"], np.random.RandomState(int(c["seed"])), **s)
    n = len(c["vert"])
    want_rows = {"drop": 255, "contrast": 256, "jitter": 257, "height1": 1, "height2": 2, "height101": 101, "height257": 257}
    assert n == want_rows.get(name, n) and n <= 5000
    if name == "drop":
        assert t["dropped"] > 0
    if name in ("contrast", "contrast_off"):
        assert t["contrast"] == (name == "contrast")
    if name in ("jitter", "jitter_off"):
        assert t["jitter"] == (name == "jitter")
    if name == "jitter":
        assert t["clipped_low"] > 0 and t["clipped_high"] > 0
    if name in ("hue", "hue_off"):
        assert t["hue"] == (name == "hue")
    if name in ("hue", "all"):
        assert t["sextants"] == [0, 1, 2, 3, 4, 5] and t["grey"] > 0
    if name == "hue":
        assert t["wrapped"] > 0
    if name in ("all", "all_sunrgbd", "chain"):
        assert t["contrast"] and t["jitter"] and t["hue"] and t["dropped"] > 0
    if name == "nan":
        assert t["contrast"] and t["constant_channels"] == 1 and t["nan_channels"] == 1 and t["dropped"] > 0
        assert np.isnan(c["out_points"][:, 5]).all() and not np.isnan(c["out_points"][:, :5]).any()
    if name.startswith("height"):
        lower, upper, gamma = percentile_plan(n)
        assert (lower, upper) == {1: (0, 0), 2: (0, 1), 101: (0, 1), 257: (2, 3)}[n]
        assert c["out_points"].shape == (n, 7)
        if n == 101:
            assert gamma >= 0.5                                        # the second branch of numpy's lerp
        if n == 257:
            assert 0 < gamma < 1
    if name == "chain":
        assert c["out_points"].shape == (1024, 7) and s["use_random_cuboid"] and s["coloraug_sunrgbd"] and s["use_height"]


def percentile_plan(n):
    from vdetr_amd.scene_prep import percentile_plan as plan
    return plan(n)


def test_fixture_holds_the_cases_of_the_design():
    g = golden()
    assert set(CASES) == set(g)
    for name in CASES:
        cases_present(name, g[name], settings_of(g[name]))
    assert os.path.getsize(GOLDEN) < 400 * 1024


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_bit_for_bit(name):
    c = golden()[name]
    rs = np.random.RandomState(int(c["seed"]))
    out, _ = CA.loader_scene(c["vert"], c["boxes7"], rs, settings_of(c))
    assert out.dtype == np.float32 and out.shape == c["out_points"].shape
    assert out.tobytes() == c["out_points"].tobytes()
    assert state_is(rs, c["state_keys"], c["state_pos"])


@pytest.mark.parametrize("name", COLOR_CASES)
def test_host_draws_replay_the_references_stream(name):
    """``draw_color_augment``, then ``draw_augment_params``, then ``draw_sunrgbd_color`` on one generator end in the recorded
    state; with ``np.random`` itself too"""
    from vdetr_amd.scene_prep import draw_augment_params, draw_color_augment, draw_sunrgbd_color
    c = golden()[name]
    s = settings_of(c)
    saved = np.random.get_state()
    try:
        for random in (np.random.RandomState(int(c["seed"])), np.random):
            if random is np.random:
                np.random.seed(int(c["seed"]))
            p = draw_color_augment(len(c["vert"]), random, color_drop=s["color_drop"], color_contrastp=s["color_contrastp"],
                                   color_jitterp=s["color_jitterp"], hue_sat=s["hue_sat"])
            _, t = CA.color_augment_scene(c["vert"], np.random.RandomState(int(c["seed"])), **s)
            assert (p.keep is not None) == (s["color_drop"] > 0) and (p.blend is not None) == t["contrast"]
            assert (p.noise is not None) == t["jitter"] and (p.hue_val is not None) == (p.sat_ratio is not None) == t["hue"]
            if p.keep is not None:
                assert p.keep.dtype == np.bool_ and int((~p.keep).sum()) == t["dropped"]
            if p.noise is not None:
                assert p.noise.dtype == np.float64 and p.noise.shape == (len(c["vert"]), 3)
            draw_augment_params(1, *s["ratios"], random=random)
            if s["coloraug_sunrgbd"]:
                q = draw_sunrgbd_color(len(c["out_points"]), random)
                assert q.brightness.shape == q.shift.shape == (3,) and q.jitter.shape == q.keep.shape == (len(c["vert"]),)
            assert state_is(random, c["state_keys"], c["state_pos"])
    finally:
        np.random.set_state(saved)


def test_probability_zero_leaves_the_stream_alone():
    from vdetr_amd.scene_prep import draw_color_augment
    rs = np.random.RandomState(3)
    before = rs.get_state()
    p = draw_color_augment(100, rs)
    assert state_is(rs, before[1], before[2]) and p.keep is None and p.blend is None and p.noise is None and p.hue_val is None
    draw_color_augment(100, rs, hue_sat=(0.5, 0.2, 1.0))              # the gate and two draws
    twin = np.random.RandomState(3)
    twin.random(3)
    assert state_is(rs, *twin.get_state()[1:3])


def test_percentile_is_numpys():
    """the restated percentile and the host's plan against np.percentile itself (numpy 2.2: a float32 column gives float32)"""
    from vdetr_amd.scene_prep import percentile_plan as plan
    rng = np.random.default_rng(7)
    for n in list(range(1, 320)) + [1000, 4999, 5000, 40000, 150000]:
        z = rng.uniform(-1, 3, n).astype(np.float32)
        want = np.percentile(z, 0.99)
        assert want.dtype == np.float32
        got = CA.percentile_099(z)
        assert np.float32(got).tobytes() == want.tobytes(), n
        lower, upper, gamma = plan(n)
        srt = np.sort(z)
        a, b = srt[lower], srt[upper]
        mine = b - (b - a) * (np.float32(1) - gamma) if gamma >= 0.5 else a + (b - a) * gamma
        assert np.float32(mine).tobytes() == want.tobytes(), n
    z = rng.uniform(-1, 3, 50).astype(np.float32)
    z[17] = np.nan
    assert np.isnan(np.percentile(z, 0.99)) and np.isnan(CA.percentile_099(z))


def test_ragged_batch_of_the_restatement():
    """scene by scene is the batch: every fixture scan through the colour step on its own generator"""
    g = golden()
    for name in COLOR_CASES:
        c, s = g[name], settings_of(g[name])
        a, _ = CA.color_augment_scene(c["vert"], np.random.RandomState(int(c["seed"])), **s)
        b, _ = CA.color_augment_scene(c["vert"], np.random.RandomState(int(c["seed"])), **s)
        assert a.tobytes() == b.tobytes() and np.array_equal(a[:, :3], c["vert"][:, :3])
