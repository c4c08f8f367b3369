"""CPU: the numpy restatement of the scene preparation (tests/scene_prep_restatement.py) against the fixture that the
reference's own loader produced (tests/golden/scene_prep.npz, tools/make_scene_prep_golden.py), bit for bit, and
``draw_augment_params`` against the draws recorded there: same parameters, same generator state afterwards."""
import os

import numpy as np
import pytest

import scene_prep_restatement as SR
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_prep.npz")
PARAM_KEYS = ("flip_x", "flip_y", "rot_angle", "trans", "scale")
_cache = {}


def golden():
    """-> {case name: {key: array}} plus "mean_size_arr"; loaded once"""
    if not _cache:
        z = np.load(GOLDEN)
        _cache["mean_size_arr"] = z["mean_size_arr"]
        for name in z["cases"]:
            _cache[str(name)] = {k.split(":", 1)[1]: z[k] for k in z.files if k.startswith(f"{name}:")}
    return _cache


CASES = ("aug", "aug_noratio", "eval", "choices", "color_mean", "color_unit")


def same_bits(got, want):
    """same dtype, same shape, same values; inf and nan at the same places (the sign of a zero is not looked at)"""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=want.dtype.kind == "f")


def params_of(c):
    from vdetr_amd.scene_prep import AugmentParams
    return AugmentParams(*(c[k] for k in PARAM_KEYS))


def restated(c, mean_size):
    color_mean = float(c["color_mean"]) if bool(c["use_color"]) else None
    return SR.prepare_batch(c["points"], c["offsets"], c["boxes"], c["box_counts"], c["box_classes"], params_of(c), mean_size,
                            choices=c.get("choices"), color_mean=color_mean, augment=bool(c["augment"]))


def test_fixture_holds_the_cases_of_the_design():
    g = golden()
    assert set(CASES) <= set(g)
    a = g["aug"]
    assert np.diff(a["offsets"]).tolist() == [1, 257, 5000] and sorted(a["box_counts"].tolist()) == [0, 5, 64]
    assert a["ratios"][1] > 0 and a["ratios"][2] > 0 and not g["aug_noratio"]["ratios"][1:].any()
    assert a["points"][1, 0] == 0 and a["points"][1, 1] == 0                       # the point on the z axis ...
    assert a["out_points"][1, 2] != 0 and a["rot_angle"][1] != 0                    # ... of a scene that is turned
    ch = g["choices"]["choices"]
    assert ch.shape == (2, 256) and len(np.unique(ch[0])) < 100 == np.diff(g["choices"]["offsets"])[0]
    assert g["color_mean"]["points"].shape[1] == 6 and g["color_mean"]["color_mean"] < 0 <= g["color_unit"]["color_mean"]
    assert not np.isfinite(a["gt_box_sizes_normalized"][0]).any()                   # one point: no extent, as the reference has it


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_bit_for_bit(name):
    g = golden()
    c = g[name]
    with np.errstate(all="ignore"):
        got = restated(c, g["mean_size_arr"])
    for k in SR.FLOAT_KEYS + SR.EXACT_KEYS:
        assert same_bits(got[k], c[k]), k
    assert same_bits(np.concatenate(got["point_clouds"]), c["out_points"])
    assert [len(p) for p in got["point_clouds"]] == np.diff(c["out_offsets"]).tolist()


def test_identity_parameters_give_the_evaluation_split():
    """augment=False skips the block; identity parameters through it give the same values"""
    g = golden()
    c = dict(g["eval"], augment=np.array(True))
    got = restated(c, g["mean_size_arr"])
    for k in SR.FLOAT_KEYS + SR.EXACT_KEYS:
        assert same_bits(got[k], c[k]), k
    assert same_bits(np.concatenate(got["point_clouds"]), c["out_points"])


@pytest.mark.parametrize("name", ("aug", "aug_noratio", "choices", "color_unit"))
def test_draw_augment_params_replays_the_references_draws(name):
    from vdetr_amd.scene_prep import draw_augment_params
    c = golden()[name]
    B = len(c["offsets"]) - 1
    state = np.random.get_state()
    try:
        np.random.seed(int(c["seed"]))
        p = draw_augment_params(B, *c["ratios"])
        after = np.random.get_state()
    finally:
        np.random.set_state(state)
    for k in PARAM_KEYS:
        assert same_bits(getattr(p, k), c[k]), k
    assert np.array_equal(after[1], c["state_keys"]) and after[2] == int(c["state_pos"])
    rs = np.random.RandomState(int(c["seed"]))                                      # a generator of the caller's own
    q = draw_augment_params(B, *c["ratios"], random=rs)
    assert all(same_bits(getattr(q, k), c[k]) for k in PARAM_KEYS) and rs.get_state()[2] == int(c["state_pos"])


def test_ratio_zero_skips_its_draws():
    g = golden()
    assert g["aug"]["state_pos"] - g["aug_noratio"]["state_pos"] == 3 * (3 + 1) * 2   # 3 scenes x (3 + 1) doubles of 2 words
    assert not g["aug_noratio"]["trans"].any() and (g["aug_noratio"]["scale"] == 1).all()


def test_identity_params_and_the_nyu40_table():
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    from vdetr_amd.scene_prep import AugmentParams, nyu40_to_class
    t = AugmentParams.identity(3).table()
    assert t.shape == (3, 8) and t.dtype == np.float64 and np.array_equal(t[0], [0, 0, 1, 0, 0, 0, 0, 1])
    g = golden()
    cfg = ScannetDatasetConfig()
    assert np.array_equal(cfg.mean_size_arr, g["mean_size_arr"])
    for name in CASES:
        c = g[name]
        for b, n in enumerate(c["box_counts"]):
            assert np.array_equal(nyu40_to_class(c["box_nyu40"][b, :n], cfg), c["box_classes"][b, :n])


def test_tolerance_helper():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2))
    assert SR.within(np.array([np.nextafter(up, np.float32(2))]), np.array([one]))       # 2 ulps
    assert not SR.within(np.array([np.float32(1 + 4 * 2.0 ** -23)]), np.array([one]))    # 4 ulps
    assert SR.within(np.array([np.float32(5e-10)]), np.array([np.float32(0)]))           # the absolute floor
    assert not SR.within(np.array([np.float32(1e-8)]), np.array([np.float32(0)]))
    assert SR.within(np.array([np.nan, np.inf], np.float32), np.array([np.nan, np.inf], np.float32))
    assert not SR.within(np.array([1.0, np.inf], np.float32), np.array([np.nan, np.inf], np.float32))
    assert SR.ulps(np.array([up]), np.array([one])).tolist() == [1.0]
