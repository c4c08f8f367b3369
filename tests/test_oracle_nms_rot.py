"""CPU: the rotated-NMS restatement (tests/rot_nms_restatement.py) against the fixture made with the reference's own box3d_iou
(tools/make_rot_nms_golden.py), and its link to the axis-aligned oracle for boxes without yaw."""
import os

import numpy as np

import rot_nms_restatement as RN
from oracle import nms_oracle as NO

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "nms3d_rot.npz")
VARIANTS = {  # name in the fixture -> (same class only, threshold, old type)
    "samecls_0.25": (True, 0.25, False), "samecls_0.5": (True, 0.5, False), "any_0.25": (False, 0.25, False),
    "any_0.5": (False, 0.5, False), "samecls_old_0.25": (True, 0.25, True), "samecls_old_0.5": (True, 0.5, True),
    "any_old_0.5": (False, 0.5, True)}


def cases():
    z = np.load(GOLDEN)
    assert z["variants"].tolist() == list(VARIANTS)
    for ci in range(int(z["ncases"])):
        c = {k.split(":", 1)[1]: z[k] for k in z.files if k.startswith(f"c{ci}:")}
        c["keep"] = dict(zip(VARIANTS, c["keep"]))
        yield ci, c


def same_kind(got, want, rtol=1e-9, atol=1e-12):
    """equal within the tolerance where finite; non-finite entries of the same kind (nan / +inf / -inf) in the same places"""
    got, want = np.asarray(got), np.asarray(want)
    fin = np.isfinite(want)
    return (np.array_equal(fin, np.isfinite(got)) and np.allclose(got[fin], want[fin], rtol=rtol, atol=atol)
            and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]))


def test_restatement_reproduces_the_reference_matrix_and_masks():
    for ci, c in cases():
        for name, (same, thr, old) in VARIANTS.items():
            for prune in (True, False):
                keep, _ = RN.nms_rotated(c["corners"], c["score"], c["cls"] if same else None, c["valid"], thr, old, prune=prune)
                assert np.array_equal(keep, c["keep"][name]), (ci, name, prune)
            assert 0 < keep.sum() <= c["valid"].sum()
        if "iou" in c:
            assert same_kind(RN.iou_matrix(c["corners"], c["corners"]), c["iou"], rtol=0, atol=0), ci   # to the last bit


def test_fixture_holds_the_hand_made_groups():
    c = dict(cases())[0]
    iou = c["iou"]
    assert np.all(iou[:3, :3] > 0.9)                                   # nearly coincident: whatever the clip makes of it
    assert np.all(iou[3:7, 3:7][~np.eye(4, dtype=bool)] == 0.0)        # touching boxes do not overlap
    assert (iou[np.triu_indices(64, 1)] > 0.5).sum() > 10 and (iou == 0).mean() > 0.5
    yaw0 = dict(cases())[1]["corners"]
    assert np.all(yaw0[:, 0, 2] == yaw0[:, 3, 2]) and np.all(yaw0[:, 0, 0] == yaw0[:, 1, 0])


def yaw0_scene(seed, K, classes, room):
    rng = np.random.default_rng(seed)
    corners = np.stack([RN.box(rng.uniform(0.4, 1.2, 3), 0.0, rng.uniform(0, room, 3)) for _ in range(K)])
    return corners, (rng.integers(0, 50, K) / 50).astype(np.float32), rng.integers(0, classes, K).astype(np.int32)


def test_yaw0_equals_the_axis_aligned_oracle():
    """the link to the existing path: without yaw the box is its own hull, so both rules decide alike (away from the threshold)"""
    for ci, c in list(cases())[1:2] + [(10 + s, dict(zip(("corners", "score", "cls"), yaw0_scene(s, 120, 2, 2.5)))) for s in range(2)]:
        for same in (True, False):
            for thr, old in ((0.25, False), (0.5, True)):
                keep, margin = RN.nms_rotated(c["corners"], c["score"], c["cls"] if same else None, None, thr, old)
                assert margin >= RN.MARGIN
                rows = NO.extents_with_score(c["corners"], c["score"], c["cls"])
                want = np.zeros(len(keep), bool)
                want[NO.nms_3d(rows if same else rows[:, :7], thr, same_class=same, old_type=old, stable=True)] = True
                assert np.array_equal(keep, want), (ci, same, thr, old)
                assert 0 < keep.sum() < len(keep)


def test_pruned_and_plain_loops_agree_on_rotated_scenes():
    rng = np.random.default_rng(4)
    K = 90
    corners = np.stack([RN.box(rng.uniform(0.3, 1.5, 3), rng.uniform(-3, 3), rng.uniform(0, 3, 3)) for _ in range(K)])
    score, cls = rng.random(K).astype(np.float32), rng.integers(0, 2, K)
    for thr, old in ((0.25, False), (0.5, True)):
        a, ma = RN.nms_rotated(corners, score, cls, None, thr, old, prune=True)
        b, mb = RN.nms_rotated(corners, score, cls, None, thr, old, prune=False)
        assert np.array_equal(a, b) and min(ma, mb) >= RN.MARGIN and 0 < a.sum() < K
