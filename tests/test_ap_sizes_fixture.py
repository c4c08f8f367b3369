"""tests/golden/ap_sizes.npz (tools/make_ap_sizes_golden.py) holds what the size-split tests need, read with the host path's own
volume rule (eval_det._volumes / _size_filter, numpy): all three sizes on both sides, rows exactly on a bound, and the two
conditions under which the reference's recording is free of its own quirks."""
import os

import numpy as np

SIZES = ("S", "M", "L")


def _fixture():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "ap_sizes.npz"))


def test_fixture_covers_every_size_and_the_bounds():
    from vdetr_amd.eval_det import AREA_RNG, _size_filter, _volumes
    z = _fixture()
    det, gt = z["corners"][z["keep"]], z["gt_corners"][z["gt_present"]]
    assert det.dtype == np.float32 and gt.dtype == np.float32
    det_vol, gt_vol = _volumes(det), _volumes(gt)
    assert det_vol.dtype == np.float32
    det_in = np.stack([_size_filter(det_vol, s) for s in SIZES])
    gt_in = np.stack([_size_filter(gt_vol, s) for s in SIZES])
    assert det_in.any(1).all() and gt_in.any(1).all()                      # detections and ground truth in all three sizes
    assert (det_in.sum(0) <= 1).all() and (gt_in.sum(0) <= 1).all()        # a box is of at most one size
    for bound in AREA_RNG:                                                 # rows on both bounds, and they are of no size
        on_det, on_gt = det_vol == np.float32(bound), gt_vol == np.float32(bound)
        assert on_det.any() and on_gt.any(), bound
        assert not det_in[:, on_det].any() and not gt_in[:, on_gt].any(), bound
    assert int((~det_in.any(0)).sum()) == 2 and int((~gt_in.any(0)).sum()) == 2


def test_fixture_keeps_the_reference_quirks_out():
    from vdetr_amd.eval_det import _size_filter, _volumes
    z = _fixture()
    keep, scores = z["keep"], z["scores"]
    C = scores.shape[-1]
    assert keep.any() and set(np.unique(z["gt_cls"][z["gt_present"]])) <= set(range(C))   # per-class form: every class has detections
    vol = _volumes(z["corners"][keep])
    for size in SIZES:
        sel = _size_filter(vol, size)
        for c in range(C):
            s = scores[keep][sel, c]
            assert len(np.unique(s)) == len(s), (size, c)                  # no tie for the reference's unstable argsort
    for size in SIZES:
        for thr in (0.25, 0.5):
            assert list(z[f"{size}:t{thr}:classes"]) == list(range(C))
            assert z[f"{size}:t{thr}:ap"].shape == z[f"{size}:t{thr}:recall"].shape == (C,)
