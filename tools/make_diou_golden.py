#!/usr/bin/env python3
"""Generates tests/golden/criterion_{diou,iou}_*.npz: the reference's own criterion.py run with ``--iou_type diou / iou``
on CPU (build container only, like oracle/make_golden.py, whose import recipe and synthetic inputs it reuses).

mmcv is absent, so the three rotated-IoU functions criterion.py imports from it (criterion.py:21-22) are replaced by the
fp64 restatement of tests/rot_iou_restatement.py (parity-unpinned, see its header).  Everything else -- the reference's
diff_diou_rotated_3d with its (x, y, w) centre term, the masking of absent slots, the matcher's cost and loss_giou --
is the reference's code, so the fixtures pin that composition.

    python tools/make_diou_golden.py
"""
import os
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import make_golden as MG  # noqa: E402
import rot_iou_restatement as R  # noqa: E402

DIFF = ("sem_cls_logits", "center_reg", "size_reg", "angle_logits", "angle_residual_normalized", "angle_continuous")
KEEP = DIFF + ("pre_box_center_unnormalized", "pre_box_size_unnormalized", "objectness_prob", "box_corners")


def patch_mmcv(C):
    """the reference module's three mmcv names -> the restatement (in float32 like the module's inputs)"""
    C.box2corners = R.box2corners
    C.oriented_box_intersection_2d = lambda c1, c2: (R.intersection_area(c1.double(), c2.double()).to(c1.dtype), None)
    C.diff_iou_rotated_3d = lambda b1, b2: R.rotated_iou_3d(b1.double(), b2.double()).to(b1.dtype)


def stage_with_angle(g, cfg, B, P, C, rotated, near):
    st = MG.synthetic_stage(g, cfg, B, P, C, rotated=rotated, near=near)
    if rotated:  # the decoded angle as a leaf that receives the gradient
        st["angle_continuous"] = ((torch.rand((B, P), generator=g) - 0.5) * 2.0).requires_grad_(True)
    return st


def main():
    T, PE, Cfg = MG.import_reference()
    C = MG.import_reference_criterion()
    patch_mmcv(C)
    cfg = Cfg()
    base = dict(cls_loss="focalloss_0.25", is_bilable=True, repeat_num=5, point_cls_loss_weight=0.05,
                matcher_giou_cost=2.0, matcher_cls_cost=3.0, matcher_center_cost=1.0, matcher_objectness_cost=0.0,
                matcher_size_cost=0.5, matcher_anglecls_cost=0.0, matcher_anglereg_cost=0.0, loss_giou_weight=2.0,
                loss_sem_cls_weight=3.0, loss_no_object_weight=0.0, loss_angle_cls_weight=0.1, loss_angle_reg_weight=0.5,
                loss_center_weight=1.0, loss_size_weight=0.5)
    # iou_type, case, B, tokens of the first stage, queries, later stages, gt slots, gt per scene, repeat_num, rotated
    for iou_type in ("diou", "iou"):
        for case, B, N0, P, S, G, counts, rep, rot in [("aligned", 2, 64, 40, 1, 8, (5, 3), 5, False),
                                                        ("rotated", 1, 48, 32, 1, 8, (6,), 5, True),
                                                        ("norepeat", 2, 40, 24, 1, 6, (4, 0), 1, True)]:
            name = f"criterion_{iou_type}_{case}"
            g = torch.Generator().manual_seed(sum(map(ord, name)))
            a = Namespace(**{**base, "repeat_num": rep, "iou_type": iou_type})
            crit = C.build_criterion(a, cfg)
            targets = MG.synthetic_targets(g, cfg, B, G, counts, cfg.num_semcls, rotated=rot)
            near = targets["gt_box_centers"][:, :max(counts[0], 1)]
            nc = cfg.num_semcls
            stages = [stage_with_angle(g, cfg, B, N0, 1, rot, near)] + [
                stage_with_angle(g, cfg, B, P, nc, rot, near) for _ in range(S + 1)]
            seed_xyz = torch.tensor([1.0, 1.0, 1.0]) + torch.rand((B, N0, 3), generator=g) * torch.tensor([8.0, 6.0, 3.0])
            seed_xyz[:, :G] = targets["gt_box_centers"]
            point_logits = (torch.randn((B, N0, nc), generator=g) - 1).requires_grad_(True)
            outputs = {"outputs": stages[-1], "aux_outputs": stages[:-1], "seed_inds": torch.zeros((B, N0), dtype=torch.int64),
                       "seed_xyz": seed_xyz, "enc_outputs": {"point_cls_logits": point_logits}}
            records = []
            hook = crit.matcher.register_forward_hook(lambda m, i, o: records.append(o))
            loss, loss_dict = crit(outputs, {k: v.clone() for k, v in targets.items()})
            hook.remove()
            loss.backward()
            arrays = {"loss": MG.np_(loss), "B": np.array(B), "N0": np.array(N0), "P": np.array(P), "S": np.array(S),
                      "repeat_num": np.array(rep), "iou_type": np.array(iou_type), "seed_xyz": MG.np_(seed_xyz),
                      "point_cls_logits": MG.np_(point_logits), "grad:point_cls_logits": MG.np_(point_logits.grad)}
            for k, v in targets.items():
                arrays["target:" + k] = MG.np_(v)
            for k, v in loss_dict.items():
                arrays["loss:" + k] = MG.np_(torch.as_tensor(v))
            order = [len(stages) - 1] + list(range(len(stages) - 1))
            for si, rec in zip(order, records):
                arrays[f"match{si}:inds"] = MG.np_(rec["per_prop_gt_inds"])
                arrays[f"match{si}:mask"] = MG.np_(rec["proposal_matched_mask"])
            for si, st in enumerate(stages):
                for k in KEEP:
                    arrays[f"stage{si}:{k}"] = MG.np_(st[k])
                    if st[k].grad is not None:
                        arrays[f"grad{si}:{k}"] = MG.np_(st[k].grad)
            MG.save(name, **arrays)


if __name__ == "__main__":
    main()
