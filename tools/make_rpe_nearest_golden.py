#!/usr/bin/env python3
"""Generates tests/golden/cross_attn_nearest.npz and cross_attn_nearest_rot.npz: the reference's own ``GlobalShareCrossAttention`` (models/vdetr_transformer.py:
656-758) with ``rpe_quant="nearest_4_10"`` on the CPU, eval mode, loss ``x.sum()`` (build container only, like
oracle/make_golden.py, whose import recipe and scene it reuses).  Two cases:

    plain   angle_type "",              B=2, nQ=5,  nK=7
    rot     angle_type "object_coords", B=1, nQ=16, nK=128, random yaw (query 0: yaw 0, it carries the delta-0 key)

Both contain a key whose delta to a vertex is exactly 0 and keys more than 8 m away on both sides (zero padding); every other
key is moved until no (query, key) pair has a look-up coordinate within 1e-4 of a cell boundary (tests/rpe_nearest_restatement.py:
clean_keys), so that a kernel whose coordinate differs by a few ulps from torch's picks the same cells.  Both cases use one
set of weights (oracle/param_fill.py, rounded to fp16-representable values and stored as float16: half the bytes, exact), kept
once as ``state:<name>`` in the first file; per case: the inputs, ``x``, ``attn`` and the gradients of cpb_mlps.*, q, k, v and
proj.  The weight gradients are dense fp32 matrices that do not compress, so each case is a file of its own (about 0.7 MB).

    python tools/make_rpe_nearest_golden.py
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import make_golden as MG  # noqa: E402
import rpe_nearest_restatement as R  # noqa: E402

MARGIN = 1e-4
CFG = SimpleNamespace(table_size=10, log_scale=512.0, max_value=4.0)
CASES = [("plain", "", 2, 5, 7), ("rot", "object_coords", 1, 16, 128)]


def main():
    T, _, Cfg = MG.import_reference()
    cfg = Cfg()
    arrays = {}
    state = None
    for name, angle_type, B, nQ, nK in CASES:
        g = torch.Generator().manual_seed(sum(map(ord, "cross_attn_nearest_" + name)))
        mod = T.GlobalShareCrossAttention(256, 4, attn_drop=0.1, proj_drop=0.1,
                                          args=MG.args_ns(angle_type=angle_type, rpe_quant="nearest_4_10"))
        MG.fill_module(mod)
        with torch.no_grad():
            for m in mod.cpb_mlps:  # as oracle/make_golden.py: a bias of O(1) and a table with structure
                m[0].weight.mul_(2.0)
                m[2].weight.mul_(1.5)
            for p in mod.parameters():
                p.copy_(p.half().float())
        mod.eval()
        if state is None:
            state = {k: v for k, v in mod.state_dict().items() if k != "relative_coords_table"}
            for k, v in state.items():
                assert torch.equal(v.half().float(), v)
                arrays["state:" + k] = MG.np_(v.half())
        xyz, center, size = MG.scene(g, B, nQ, nK, edge_cases=False)
        angle = (torch.rand((B, nQ), generator=g) * 2 - 1) * 3.1 if angle_type else torch.zeros((B, nQ))
        # query 0 carries the delta-0 key and stays unturned: in a turned frame the key's offsets to the NEIGHBOURS of its vertex
        # are 1e-8 instead of 0, i.e. on the cell boundary at 4.5 within rounding (exact zeros are exempt, see `fragile`)
        angle[:, 0] = 0.0
        corners = cfg.box_parametrization_to_corners(center, size, angle)
        ref_pts = T.convert_corners_camera2lidar(corners.clone())
        # the edge cases: delta == 0 to vertex 0 of query 0; beyond 8 m on the negative and on the positive side of every axis
        xyz[:, 0] = ref_pts[:, 0, 0]
        xyz[:, 1] = torch.tensor([30.0, 27.0, 14.0])
        xyz[:, 2] = torch.tensor([-25.0, -22.0, -9.0])
        cs = R.yaw_cos_sin(angle) if angle_type else None
        xyz = R.clean_keys(ref_pts, xyz, CFG, MARGIN, g, cs, keep=(0, 1, 2))
        assert not R.fragile(ref_pts, xyz, CFG, MARGIN, cs).any()
        pix = R.pix_coords(ref_pts.double(), xyz.double(), 10, cos_sin=None if cs is None else cs.double())
        far = pix[:, :, 1:3]
        assert (far[..., 2] < -0.5)[:, :, 0].all() and (far[..., 2] > 9.5)[:, :, 1].all()  # z: below / above the table
        assert ((far < -0.5) | (far > 9.5)).any(dim=-1).all() and (far < -0.5).any() and (far > 9.5).any()  # every vertex padded
        assert (ref_pts[:, 0, 0] == xyz[:, 0]).all()
        query = torch.randn((nQ, B, 256), generator=g).requires_grad_(True)
        key = torch.randn((nK, B, 256), generator=g).requires_grad_(True)
        x, attn = mod(query, key, ref_pts, angle if angle_type else None, xyz)
        x.sum().backward()
        case = dict(query=query, key=key, reference_point=ref_pts, reference_angle=angle, xyz=xyz, x=x, attn=attn)
        for k, v in case.items():
            arrays[f"{name}:{k}"] = MG.np_(v)
        arrays[f"{name}:angle_type"] = np.array(angle_type)
        for pname, p in mod.named_parameters():
            arrays[f"{name}:grad_param:{pname}"] = MG.np_(p.grad)
        MG.save("cross_attn_nearest" if name == "plain" else "cross_attn_nearest_" + name, **arrays)
        arrays = {}


if __name__ == "__main__":
    main()
