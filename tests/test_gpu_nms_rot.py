"""GPU: the rotated-box NMS and the all-pairs box3d_iou against the fixture made with the reference's own
box3d_iou (tests/golden/nms3d_rot.npz) and against the numpy restatement at sizes the fixture does not hold.  Keep masks are
decisions: identical.  Every generated scene first has to pass a condition on the ORACLE side: over all pairs the greedy loop
evaluates, ``|overlap - threshold| >= 1e-6`` (far above float64 rounding, far below the margins ordinary seeds give), so that
an exact comparison of the masks is a fair demand; no case is dropped or tolerated on the device side."""
import numpy as np
import pytest
import torch

import rot_nms_restatement as RN
from oracle import nms_oracle as NO
from test_oracle_nms_rot import VARIANTS, cases, same_kind

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rotated_scene(seed, K, classes, room, yaw=True):
    """K boxes of 0.4-1.2 m (a long thin one now and then) standing in a room x 1.5 x room space, repeated scores (the stable
    order decides)"""
    rng = np.random.default_rng(seed)
    size = rng.uniform(0.4, 1.2, (K, 3)) * np.where(rng.random((K, 1)) < 0.2, [2.5, 0.4, 1.0], 1.0)
    corners = np.stack([RN.box(size[k], rng.uniform(-3.1, 3.1) if yaw else 0.0, rng.uniform(0, [room, 1.5, room])) for k in range(K)])
    return corners, (rng.integers(0, 50, K) / 50).astype(np.float32), rng.integers(0, classes, K).astype(np.int32)


def test_box3d_iou_pairs_matches_reference_matrix_and_restatement():
    from vdetr_amd.nms import box3d_iou_pairs
    c = dict(cases())[0]
    got = box3d_iou_pairs(dev(c["corners"]), dev(c["corners"])).cpu().numpy()
    assert got.shape == (64, 64) and got.dtype == np.float64
    assert same_kind(got, c["iou"])                                  # the nearly coincident and the touching group included
    rng = np.random.default_rng(17)
    a = np.stack([RN.box(rng.uniform(0.3, 2, 3), rng.uniform(-3, 3) * (i % 4 != 0), rng.uniform(0, 2.5, 3)) for i in range(37)])
    b = np.stack([RN.box(rng.uniform(0.3, 2, 3), rng.uniform(-3, 3) * (i % 3 != 0), rng.uniform(0, 2.5, 3)) for i in range(50)])
    b[:5] = a[:5]                                                    # exact copies (rotated ones are ill-conditioned)
    got = box3d_iou_pairs(dev(a), dev(b)).cpu().numpy()
    want = RN.iou_matrix(a, b)
    assert (want > 0).mean() > 0.1
    assert same_kind(got, want)
    assert box3d_iou_pairs(dev(a[:0]), dev(b)).shape == (0, 50)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        box3d_iou_pairs(torch.from_numpy(a), torch.from_numpy(b))


def test_keep_masks_equal_the_fixture_through_every_entry_point():
    from vdetr_amd.nms import batched_nms_3d, nms_3d_rotated
    cs = dict(cases())
    for ci, c in cs.items():
        corners, score, cls, valid = (dev(c[k]) for k in ("corners", "score", "cls", "valid"))
        for name, (same, thr, old) in VARIANTS.items():
            keep = batched_nms_3d(corners[None], score[None], cls[None] if same else None, valid[None], thr, old, rotated=True)[0]
            assert np.array_equal(keep.cpu().numpy(), c["keep"][name]), (ci, name)
            if c["valid"].all():
                pick = nms_3d_rotated(corners, score, cls if same else None, thr, old).cpu().numpy()
                order = np.argsort(c["score"], kind="stable")[::-1]
                assert pick.tolist() == [i for i in order if c["keep"][name][i]], (ci, name)      # best first
    both = [cs[2], cs[3]]                                            # a batch of two scenes with a valid mask
    corners, score, cls, valid = (dev(np.stack([c[k] for c in both])) for k in ("corners", "score", "cls", "valid"))
    for name, (same, thr, old) in VARIANTS.items():
        keep = batched_nms_3d(corners, score, cls if same else None, valid, thr, old, rotated=True).cpu().numpy()
        assert np.array_equal(keep, np.stack([c["keep"][name] for c in both])), name


def config(**kw):
    from vdetr_amd.ap_calculator import get_ap_config_dict
    return get_ap_config_dict(remove_empty_box=False, per_class_proposal=False, rotated_nms=True, **kw)


def prediction_inputs(c, split_score):
    """the fixture's scene as parse_predictions' arguments; ``split_score``: objectness x angle probability == score exactly
    (the angle probability is a power of two), and the objectness alone ranks the boxes differently"""
    K = len(c["score"])
    rng = np.random.default_rng(K)
    angle = np.exp2(rng.integers(-2, 3, K)).astype(np.float32) if split_score else np.ones(K, np.float32)
    obj = c["score"] / angle
    assert np.array_equal(obj * angle, c["score"])
    sem = np.full((K, 3), 0.1, np.float32)
    sem[np.arange(K), c["cls"]] = 0.8
    return dev(c["corners"])[None], dev(sem)[None], dev(obj)[None], dev(angle)[None]


def test_prediction_masks_and_parse_predictions_with_rotated_nms():
    from vdetr_amd.ap_calculator import APCalculator, parse_predictions, prediction_masks
    for ci, c in list(cases())[:2]:                                  # the two scenes whose boxes are all valid
        for name, kw, split in (("samecls_0.25", dict(), False), ("samecls_0.5", dict(nms_iou=0.5, angle_nms=True), True),
                                ("samecls_old_0.5", dict(nms_iou=0.5, use_old_type_nms=True, angle_nms=True), True),
                                ("any_0.25", dict(cls_nms=False), False), ("any_old_0.5", dict(cls_nms=False, nms_iou=0.5, use_old_type_nms=True), False),
                                ("any_0.5", dict(cls_nms=False, nms_iou=0.5, no_nms=True), False)):   # rotated_nms is looked at first
            corners, sem, obj, angle = prediction_inputs(c, split)
            m = prediction_masks(corners, sem, obj, angle, None, config(**kw))
            assert np.array_equal(m["pred_mask"][0].cpu().numpy(), c["keep"][name]), (ci, name)
            want = c["keep"][name] & (obj[0].cpu().numpy() > 0)
            dets = parse_predictions(corners, sem, obj, angle, None, config(**kw))[0]
            assert len(dets) == want.sum()
            assert np.array_equal(np.stack([d[1] for d in dets]), c["corners"][want]), (ci, name)
            calc = APCalculator(None, ap_config_dict=config(**kw))
            calc.step(corners, sem, obj, angle, None, corners[:, :2], dev(c["cls"][:2].astype(np.int64))[None],
                      torch.ones((1, 2), device=DEV), None)
            assert np.array_equal(calc._flat_pred[0][0], c["corners"][want]), (ci, name)
    corners, sem, obj, angle = prediction_inputs(dict(cases())[0], False)
    with pytest.raises(ValueError, match="use_3d_nms"):
        prediction_masks(corners, sem, obj, angle, None, config(use_3d_nms=False))


@pytest.mark.parametrize("K,classes,room", [(1, 1, 1.0), (63, 2, 1.5), (64, 1, 1.0), (65, 3, 2.0), (300, 2, 2.0), (1000, 1, 10.0),
                                            (1500, 3, 5.0)])
def test_sizes_against_the_restatement(K, classes, room):
    """Word counts that are not powers of two, the last partial word, the walk over the relation in LDS (K <= 1024) and in the
    workspace (K > 1024)."""
    from vdetr_amd.nms import batched_nms_3d
    corners, score, cls = rotated_scene(K, K, classes, room)
    for thr, old in ((0.25, False), (0.5, True)) if K <= 300 else ((0.25, False),):
        want, margin = RN.nms_rotated(corners, score, cls, None, thr, old)
        print(f"K={K} thr={thr} old={old}: kept {want.sum()}, margin {margin:.3g}")
        assert margin >= RN.MARGIN                                   # the oracle-side condition, before the device is looked at
        assert K == 1 or 0 < want.sum() < K
        keep = batched_nms_3d(dev(corners)[None], dev(score)[None], dev(cls)[None], None, thr, old, rotated=True)[0].cpu().numpy()
        assert np.array_equal(keep, want)


def test_yaw0_scenes_give_the_axis_aligned_mask():
    from vdetr_amd.nms import batched_nms_3d
    for seed, K, classes, room in ((1, 200, 2, 3.0), (2, 700, 4, 5.0)):
        corners, score, cls = rotated_scene(seed, K, classes, room, yaw=False)
        rows = NO.extents_with_score(corners, score, cls)
        with np.errstate(all="ignore"):                              # oracle side: no axis-aligned IoU sits on the threshold
            lo, hi = rows[:, None, 0:3], rows[:, None, 3:6]
            ext = np.maximum(0, np.minimum(hi, hi.transpose(1, 0, 2)) - np.maximum(lo, lo.transpose(1, 0, 2))).prod(-1)
            vol = (rows[:, 3:6] - rows[:, 0:3]).prod(-1)
            assert np.abs(ext / (vol[:, None] + vol[None] - ext) - 0.25).min() >= RN.MARGIN
        args = (dev(corners)[None], dev(score)[None], dev(cls)[None], None, 0.25)
        plain, rot = batched_nms_3d(*args)[0].cpu().numpy(), batched_nms_3d(*args, rotated=True)[0].cpu().numpy()
        assert 0 < plain.sum() < K and np.array_equal(plain, rot)


def test_rotated_scene_where_the_two_rules_differ():
    """a long thin box at 45 degrees has a hull of about twice its footprint: the hull rule suppresses neighbours that the
    rotated rule (and the AP matcher after it) sees as separate boxes"""
    from vdetr_amd.nms import batched_nms_3d
    corners, score, cls = rotated_scene(5, 300, 2, 4.0)
    want, margin = RN.nms_rotated(corners, score, cls, None, 0.25)
    assert margin >= RN.MARGIN
    args = (dev(corners)[None], dev(score)[None], dev(cls)[None], None, 0.25)
    plain, rot = batched_nms_3d(*args)[0].cpu().numpy(), batched_nms_3d(*args, rotated=True)[0].cpu().numpy()
    assert np.array_equal(rot, want)
    assert (plain != rot).sum() > 0
    assert rot.sum() > plain.sum()                                   # the hull contains the box: it can only overlap more


def test_limits_and_cpu_tensors_raise():
    from vdetr_amd.nms import batched_nms_3d, nms_3d_rotated
    with pytest.raises((RuntimeError, ValueError)):
        batched_nms_3d(torch.zeros(1, 4097, 8, 3, device=DEV), torch.zeros(1, 4097, device=DEV), rotated=True)
    assert batched_nms_3d(torch.zeros(0, 5, 8, 3, device=DEV), torch.zeros(0, 5, device=DEV), rotated=True).shape == (0, 5)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        nms_3d_rotated(torch.zeros(4, 8, 3), torch.zeros(4))


def test_axis_aligned_path_is_unchanged_on_its_fixture():
    """rotated=False (the default): the masks of tests/golden/nms3d.npz, as before"""
    from test_oracle_nms import cases as plain_cases
    from vdetr_amd.nms import batched_nms_3d
    for ci, c in plain_cases():
        corners, score, cls = (dev(c[k]) for k in ("corners", "score", "cls"))
        for key, kw in (("pick_samecls", dict(classes=cls[None])), ("pick_any", dict()),
                        ("pick_samecls_old", dict(classes=cls[None], iou_threshold=0.5, old_type=True))):
            want = np.zeros(len(c["score"]), bool)
            want[c[key]] = True
            assert np.array_equal(batched_nms_3d(corners[None], score[None], rotated=False, **kw)[0].cpu().numpy(), want), (ci, key)
