"""CPU tests (no GPU): the criterion oracle with ``iou_type`` "diou" / "iou" -- oracle/criterion_oracle.py with its
pair_terms replaced by the restatement's (tests/rot_iou_restatement.py) -- against the reference's own criterion.py run in
those modes (fixtures written by tools/make_diou_golden.py)."""
import os

import numpy as np
import pytest
import torch

import rot_iou_restatement as R
from oracle import criterion_oracle as CO
from test_oracle_criterion import check_against_golden

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROT_CASES = [f"criterion_{k}_{c}" for k in ("diou", "iou") for c in ("aligned", "rotated", "norepeat")]
LEAVES = ("sem_cls_logits", "center_reg", "size_reg", "angle_logits", "angle_residual_normalized")


def load_rot_case(name, device="cpu"):
    """-> (outputs as the model returns them, targets, raw npz).  center_unnormalized / size_unnormalized are rebuilt from
    the leaves as the fixture's generator built them (center_reg * pre_size + pre_center, exp(size_reg) * pre_size), so
    their gradients reach center_reg / size_reg; angle_continuous is a leaf where the fixture differentiates it."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    nst = int(z["S"]) + 2
    stages = []
    for si in range(nst):
        st = {}
        for k in LEAVES + ("angle_continuous", "pre_box_center_unnormalized", "pre_box_size_unnormalized", "objectness_prob",
                           "box_corners"):
            t = torch.from_numpy(z[f"stage{si}:{k}"]).to(device)
            st[k] = t.requires_grad_(True) if (k in LEAVES or f"grad{si}:{k}" in z.files) else t
        st["center_unnormalized"] = st["center_reg"] * st["pre_box_size_unnormalized"] + st["pre_box_center_unnormalized"]
        st["size_unnormalized"] = torch.exp(st["size_reg"]) * st["pre_box_size_unnormalized"]
        st["sem_cls_prob"] = st["sem_cls_logits"]
        stages.append(st)
    targets = {k[len("target:"):]: torch.from_numpy(z[k]).to(device) for k in z.files if k.startswith("target:")}
    point_logits = torch.from_numpy(z["point_cls_logits"]).to(device).requires_grad_(True)
    outputs = {"outputs": stages[-1], "aux_outputs": stages[:-1], "seed_xyz": torch.from_numpy(z["seed_xyz"]).to(device),
               "enc_outputs": {"point_cls_logits": point_logits}}
    return outputs, targets, z


def check_rot_against_golden(z, outputs, loss, loss_dict, matches, rtol, atol):
    check_against_golden(z, outputs, loss, loss_dict, matches, rtol=rtol, atol=atol)
    for si, st in enumerate(outputs["aux_outputs"] + [outputs["outputs"]]):
        key = f"grad{si}:angle_continuous"
        if key in z.files:
            np.testing.assert_allclose(st["angle_continuous"].grad.cpu().numpy(), z[key], rtol=1e-3, atol=1e-6, err_msg=key)
        assert st["box_corners"].grad is None


@pytest.mark.parametrize("name", ROT_CASES)
def test_patched_oracle_matches_reference_criterion(name, monkeypatch):
    outputs, targets, z = load_rot_case(name)
    monkeypatch.setattr(CO, "pair_terms", R.pair_terms_for(str(z["iou_type"])))
    loss, loss_dict, assigns = CO.set_criterion(outputs, targets, repeat_num=int(z["repeat_num"]))
    loss.backward()
    nst = int(z["S"]) + 2
    matches = {nst - 1: assigns["outputs"], **{k: assigns[k] for k in range(nst - 1)}}
    check_rot_against_golden(z, outputs, loss, loss_dict, matches, rtol=1e-4, atol=1e-5)


def test_fixtures_exercise_the_new_terms():
    """the fixtures carry what is new: matched boxes with an angle gradient in the rotated ones"""
    for k in ("diou", "iou"):
        z = np.load(os.path.join(GOLDEN, f"criterion_{k}_rotated.npz"))
        assert np.abs(z["grad2:angle_continuous"]).max() > 0
        assert z["match2:mask"].sum() > 0


def test_iou_ext_entry_points_reject_bad_arguments():
    """vdetr_match_cost_ext_batch_f32 / vdetr_set_loss_ext_batch_f32: argument errors are status codes with a message"""
    import ctypes
    from vdetr_amd import _lib
    lib = _lib.lib()
    d = _lib.MatchDesc()
    d.B = d.P = d.G = d.C = d.A = 1
    e = _lib.IouExt(iou_kind=_lib.VDETR_IOU_DIOU)
    assert lib.vdetr_match_cost_ext_batch_f32(ctypes.byref(d), None, 1, None) == 1
    assert b"null extensions" in lib.vdetr_last_error()
    e.iou_kind = 7
    assert lib.vdetr_match_cost_ext_batch_f32(ctypes.byref(d), ctypes.byref(e), 1, None) == 1
    assert b"unknown iou_kind 7" in lib.vdetr_last_error()
    e.iou_kind = _lib.VDETR_IOU_DIOU
    assert lib.vdetr_match_cost_ext_batch_f32(ctypes.byref(d), ctypes.byref(e), 1, None) == 1
    assert b"needs center, size and angle" in lib.vdetr_last_error()
    ls = (_lib.SetLossDesc * 2)()
    for x in ls:
        x.B = x.P = x.C = x.A = x.G = 1
        x.center_reg = 8  # box terms present (never dereferenced: the check fails first)
    es = (_lib.IouExt * 2)(_lib.IouExt(iou_kind=_lib.VDETR_IOU_GIOU), _lib.IouExt(iou_kind=_lib.VDETR_IOU_IOU))
    assert lib.vdetr_set_loss_ext_batch_f32(ls, es, 2, None) == 1
    assert b"mixed iou kinds" in lib.vdetr_last_error()
    es[0].iou_kind = es[1].iou_kind = _lib.VDETR_IOU_DIOU
    assert lib.vdetr_set_loss_ext_batch_f32(ls, es, 2, None) == 1
    assert b"needs center, size and angle" in lib.vdetr_last_error()
    with pytest.raises(ValueError, match="iou_type"):
        from vdetr_amd.criterion import build_criterion, default_criterion_args
        build_criterion(default_criterion_args(iou_type="giou3d"), None)
