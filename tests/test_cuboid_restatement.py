"""CPU: the numpy restatement of the cuboid crop and the sampling (tests/cuboid_restatement.py) against the fixture that the
reference's own loader produced (tests/golden/cuboid.npz, tools/make_cuboid_golden.py), bit for bit and with the generator's
state; ``draw_cuboid_trials`` and its put-back against the same recorded states; and the cases the fixture has to hold,
re-asserted from its recorded fields so that a regenerated file cannot lose one."""
import os

import numpy as np
import pytest

import cuboid_restatement as CR
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "cuboid.npz")
CASES = ("late", "nobox", "fallback", "empty", "f64", "n255", "n256", "n257")
G = 64
_cache = {}


def golden():
    """-> {case name: {key: array}}; loaded once"""
    if not _cache:
        z = np.load(GOLDEN)
        for name in z["cases"]:
            _cache[str(name)] = {k.split(":", 1)[1]: z[k] for k in z.files if k.startswith(f"{name}:")}
    return _cache


def state_is(random, keys, pos):
    s = random.get_state()
    return np.array_equal(s[1], keys) and s[2] == int(pos)


def fates(c):
    """(aspect-rejected, count-rejected, box-rejected) attempts before the accepted one, from the recorded calls"""
    n = len(c["attempt_valid"]) if c["trial"] < 0 else int(c["trial"])
    valid, count = c["attempt_valid"][:n] == 1, c["attempt_count"][:n]
    return int((~valid).sum()), int((valid & (count < c["min_points"])).sum()), int((valid & (count >= c["min_points"])).sum())


def batch_of(names, f64=False):
    """fixture scenes as one batch of ``crop_and_sample`` arguments (numpy); the boxes in the file's float64 or as float32"""
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    from vdetr_amd.scene_prep import nyu40_to_class
    g = golden()
    B = len(names)
    a = {"points": np.concatenate([g[n]["points"] for n in names]), "offsets": np.cumsum([0] + [len(g[n]["points"]) for n in names]).astype(np.int32),
         "boxes": np.zeros((B, G, 6), np.float64 if f64 else np.float32), "box_counts": np.array([len(g[n]["boxes7"]) for n in names], np.int64),
         "box_classes": np.zeros((B, G), np.int64)}
    for b, n in enumerate(names):
        box = g[n]["boxes7"]
        a["boxes"][b, :len(box)] = box[:, :6]
        a["box_classes"][b, :len(box)] = nyu40_to_class(box[:, 6], ScannetDatasetConfig())
    return a


def test_fixture_holds_the_cases_of_the_design():
    g = golden()
    assert set(CASES) <= set(g)
    late = g["late"]
    aspect, count, box = fates(late)
    assert late["trial"] > 0 and aspect >= 1 and count >= 1                         # accepted late, after both kinds of rejection
    assert len(late["points"]) == 5000 and len(late["crop_points"]) > late["num_points"]   # ~20 tiles; sampled without replacement
    assert len(np.unique(late["choices"])) == late["num_points"]
    assert fates(g["nobox"])[2] >= 1 and g["nobox"]["trial"] > 0                     # enough points, no box: the loop went on
    fb = g["fallback"]
    assert fb["trial"] == -1 and len(fb["attempt_valid"]) == 100 and fb["min_points"] > len(fb["points"])
    assert np.array_equal(fb["crop_points"], fb["points"]) and np.array_equal(fb["crop_boxes7"], fb["boxes7"])
    assert g["empty"]["boxes7"].shape == (0, 7) and g["empty"]["trial"] >= 0 and not g["empty"]["literal_filter"]
    f64 = g["f64"]["boxes7"][:, :6]
    assert f64.dtype == np.float64 and (f64.astype(np.float32).astype(np.float64) != f64).all()
    assert 0 < len(g["f64"]["crop_boxes7"]) < len(f64)
    for n in (255, 256, 257):
        c = g[f"n{n}"]
        assert len(c["points"]) == n and c["trial"] >= 0 and len(c["crop_points"]) < c["num_points"]      # with replacement
    assert all(bool(g[n]["literal_filter"]) == (len(g[n]["boxes7"]) > 0) for n in CASES)   # the default agrees with the literal test
    for n in CASES:
        c = g[n]
        if c["trial"] >= 0:                                            # the accepted attempt's own count is the crop
            assert c["attempt_valid"][c["trial"]] == 1 and c["attempt_count"][c["trial"]] == len(c["crop_points"]) >= c["min_points"]


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_bit_for_bit(name):
    c = golden()[name]
    rs = np.random.RandomState(int(c["seed"]))
    got = CR.crop_and_sample_scene(c["points"], c["boxes7"], rs, int(c["num_points"]), int(c["min_points"]))
    assert got["trial"] == c["trial"]
    assert np.array_equal(got["kept_rows"], c["crop_rows"])
    assert got["cloud"].dtype == np.float32 and np.array_equal(got["cloud"], c["crop_points"])
    assert np.array_equal(c["boxes7"][got["keep_boxes"]], c["crop_boxes7"])
    assert np.array_equal(got["choices"], c["choices"])
    assert state_is(rs, c["state_sampled_keys"], c["state_sampled_pos"])
    went = len(c["attempt_valid"])
    assert len(got["attempts"]) == went
    assert [a[0] != CR.ASPECT_REJECTED for a in got["attempts"]] == (c["attempt_valid"] == 1).tolist()
    assert [a[1] for a in got["attempts"]] == c["attempt_count"].tolist()


def test_literal_filter_flag_changes_nothing_here():
    """``filter_boxes`` given as the reference's literal ``sum() > 0`` is the default for every scene of the fixture"""
    for name in CASES:
        c = golden()[name]
        a, b = (CR.crop_and_sample_scene(c["points"], c["boxes7"], np.random.RandomState(int(c["seed"])), int(c["num_points"]),
                                         int(c["min_points"]), filter_boxes=f) for f in (None, bool(c["literal_filter"])))
        assert a["trial"] == b["trial"] and np.array_equal(a["rows"], b["rows"])


@pytest.mark.parametrize("name", CASES)
def test_draw_cuboid_trials_and_the_put_back_replay_the_references_stream(name):
    """every attempt drawn ahead, the generator put back to the accepted one, the sample drawn: the recorded state; the
    drawn attempts up to there are the ones the reference went through"""
    from vdetr_amd.scene_prep import draw_cuboid_trials
    c = golden()[name]
    kept = len(c["crop_points"])
    saved = np.random.get_state()
    try:
        for random in (np.random.RandomState(int(c["seed"])), np.random):
            if random is np.random:
                np.random.seed(int(c["seed"]))
            t = draw_cuboid_trials(len(c["points"]), random)
            assert t.crop_range.shape == (100, 3) and t.crop_range.dtype == np.float64 and len(t.states) == 100
            went = len(c["attempt_valid"])
            assert t.valid[:went].tolist() == (c["attempt_valid"] == 1).tolist()
            assert ((t.center >= 0) == t.valid).all() and (t.center < len(c["points"])).all()
            if c["trial"] >= 0:                                        # the centre row of the accepted attempt lies in its crop
                assert t.center[c["trial"]] in c["crop_rows"]
            assert not state_is(random, c["state_sampled_keys"], c["state_sampled_pos"])
            t.rewind(int(c["trial"]))
            choices = random.choice(kept, int(c["num_points"]), replace=kept < c["num_points"])
            assert np.array_equal(choices, c["choices"])
            assert state_is(random, c["state_sampled_keys"], c["state_sampled_pos"])
    finally:
        np.random.set_state(saved)


def test_the_stream_goes_on_into_the_augmentation():
    """after the sampling ``draw_augment_params`` continues on the same generator and ends in the scene's recorded state"""
    from vdetr_amd.scene_prep import draw_augment_params
    for name in CASES:
        c = golden()[name]
        rs = np.random.RandomState(int(c["seed"]))
        CR.crop_and_sample_scene(c["points"], c["boxes7"], rs, int(c["num_points"]), int(c["min_points"]))
        draw_augment_params(1, *c["ratios"], random=rs)
        assert state_is(rs, c["state_keys"], c["state_pos"])


def test_batch_form_of_the_restatement():
    names = ("n257", "empty", "f64")
    g = golden()
    a = batch_of(names, f64=True)
    rs = [np.random.RandomState(int(g[n]["seed"])) for n in names]
    got = CR.crop_and_sample_batch(a["points"], a["offsets"], a["boxes"], a["box_counts"], a["box_classes"], rs, 256, 60)
    assert got["choices"].shape == (3, 256) and got["boxes"].dtype == np.float64
    c = g["empty"]                                                     # min_points 60 <= its own 100: found no later than recorded
    assert 0 <= got["trial"][1] <= c["trial"] and got["box_counts"].tolist()[1] == 0
    for b in range(3):
        k = got["box_counts"][b]
        assert not got["boxes"][b, k:].any() and got["kept_points"][b] == len(got["kept_rows"][b])
        assert np.isin(got["choices"][b], got["kept_rows"][b]).all()
