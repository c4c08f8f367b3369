"""CPU restatement (plain torch, any float dtype) of the 3DV-RPE bias with rpe_quant "nearest_*" and of the cross attention
around it.  Test infrastructure only.

The reference passes the interpolation of ``--rpe_quant`` to ``F.grid_sample(..., mode=...)`` (models/vdetr_transformer.py:
675,727).  On a 5-D input, ``mode="nearest"``, ``padding_mode="zeros"``, ``align_corners=False`` is, per axis,

    pix = ((g + 1) * T - 1) / 2,   r = rint(pix) (ties to even),   value = table[rz][ry][rx] if 0 <= r <= T-1 on all axes else 0

with x -> LAST table axis, z -> first.  This file writes that out with ``rint``, a range test and a gather; it does not call
``grid_sample`` (tests/test_rpe_nearest_restatement.py checks that the two are equal).

Nearest is discontinuous: a ``pix`` that lies on a cell boundary (a half-integer) lands in one cell or the other depending on the
last bits of the arithmetic, and the device's ``pix`` (hardware log2, fused multiply-add) differs from torch's by a few ulps.
``fragile`` finds such pairs, ``clean_keys`` re-draws keys until none is left.
"""
import math

import torch


def yaw_cos_sin(angle):
    """[B,nQ] -> [B,nQ,2]: the rotation operand of angle_type "object_coords" (vdetr_transformer.py:712-720)"""
    return torch.stack((torch.cos(angle), torch.sin(angle)), dim=-1)


def deltas(vertices, xyz, cos_sin=None):
    """d [B,nQ,nK,8,3] = P_i[q] - X[k], turned by the query's yaw where cos_sin is given (vdetr_transformer.py:711-720)"""
    d = vertices[:, :, None, :, :] - xyz[:, None, :, None, :]
    if cos_sin is not None:
        c, s = cos_sin[..., 0][:, :, None, None], cos_sin[..., 1][:, :, None, None]
        d = torch.stack((d[..., 0] * c - d[..., 1] * s, d[..., 0] * s + d[..., 1] * c, d[..., 2]), dim=-1)
    return d


def pix_coords(vertices, xyz, table_size, log_scale=512.0, max_value=4.0, cos_sin=None):
    """pix [B,nQ,nK,8,3] of every (query, key, vertex, axis) (vdetr_transformer.py:711-723 + grid_sample's unnormalisation)"""
    d = deltas(vertices, xyz, cos_sin)
    g = torch.sign(d) * torch.log2(torch.abs(d) * log_scale + 1.0) / math.log2(8) / max_value
    return ((g + 1.0) * table_size - 1.0) / 2.0


def rpe_bias_nearest(tables, vertices, xyz, log_scale=512.0, max_value=4.0, cos_sin=None):
    """rpe[B,H,nQ,nK] = sum_i T_i[rint(pix_i)] (0 where a cell is outside the table); tables [8,T,T,T,H]"""
    T, H = tables.shape[1], tables.shape[-1]
    pix = pix_coords(vertices, xyz, T, log_scale, max_value, cos_sin)
    r = torch.round(pix).long()  # torch.round: half to even, as std::nearbyint
    ok = ((r >= 0) & (r <= T - 1)).all(dim=-1)  # B,nQ,nK,8
    rc = r.clamp(0, T - 1)
    cell = (rc[..., 2] * T + rc[..., 1]) * T + rc[..., 0]  # z first, x last
    out = 0
    for i in range(8):
        flat = tables[i].reshape(T * T * T, H)
        out = out + flat[cell[..., i]] * ok[..., i, None].to(tables.dtype)
    return out.permute(0, 3, 1, 2)


def fragile(vertices, xyz, cfg, margin, cos_sin=None):
    """bool [B,nQ,nK]: any of the pair's 24 pix values (computed in fp64) lies within `margin` of a half-integer.
    cfg: an object with table_size, log_scale, max_value (attention.RPEConfig).
    One coordinate is exempt: a delta that is exactly 0 (a key ON a vertex).  Its pix is (T - 1) / 2 in every implementation
    — log2(1) = 0 and 0 * a + b = b are exact — which for an even T is the tie 4.5, resolved to the even cell by every rint."""
    cs = None if cos_sin is None else cos_sin.double()
    pix = pix_coords(vertices.double(), xyz.double(), cfg.table_size, cfg.log_scale, cfg.max_value, cs)
    frac = pix - torch.floor(pix)
    near = ((frac - 0.5).abs() <= margin) & (deltas(vertices.double(), xyz.double(), cs) != 0)
    return near.flatten(3).any(dim=-1)


def clean_keys(vertices, xyz, cfg, margin, generator, cos_sin=None, keep=(), spread=0.05, max_rounds=200):
    """xyz with every key that takes part in a fragile pair nudged (by up to `spread` m per round) until no pair is fragile.
    Keys listed in `keep` (per-batch indices of deliberate edge cases) are checked but never moved."""
    xyz = xyz.clone()
    for _ in range(max_rounds):
        bad = fragile(vertices, xyz, cfg, margin, cos_sin).any(dim=1)  # B,nK
        if not bad.any():
            return xyz
        assert not bad[:, list(keep)].any(), "a key that must stay is part of a fragile pair"
        noise = (torch.rand(xyz.shape, generator=generator, dtype=xyz.dtype) - 0.5) * 2 * spread
        xyz = torch.where(bad[..., None], xyz + noise, xyz)
    raise AssertionError("clean_keys: fragile pairs left")


def cross_attention_nearest(state, query, key, reference_point, reference_angle, xyz, cfg, num_heads=4):
    """GlobalShareCrossAttention.forward in eval mode (vdetr_transformer.py:701-758) with the nearest bias, from a state dict.
    Returns (x [nQ,B,C], attn [B,H,nQ,nK], tables [8,T,T,T,H]); differentiable with respect to every tensor of `state`."""
    T = cfg.table_size
    lin = torch.linspace(-cfg.max_value, cfg.max_value, T, dtype=torch.float32).to(query.dtype)
    coords = torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), dim=-1).reshape(-1, 3)
    tables = torch.stack([torch.relu(coords @ state[f"cpb_mlps.{i}.0.weight"].T + state[f"cpb_mlps.{i}.0.bias"])
                          @ state[f"cpb_mlps.{i}.2.weight"].T for i in range(8)]).reshape(8, T, T, T, num_heads)
    cs = yaw_cos_sin(reference_angle) if reference_angle is not None else None
    rpe = rpe_bias_nearest(tables, reference_point, xyz, cfg.log_scale, cfg.max_value, cs)
    kb, qb = key.permute(1, 0, 2), query.permute(1, 0, 2)
    B, nK, C = kb.shape
    nQ = qb.shape[1]
    k = kb @ state["k.weight"].T + state["k.bias"]
    v = kb @ state["v.weight"].T + state["v.bias"]
    q = (qb @ state["q.weight"].T + state["q.bias"]).reshape(B, nQ, num_heads, C // num_heads).permute(0, 2, 1, 3)
    attn = torch.softmax((q * (C // num_heads) ** -0.5) @ k[:, None].transpose(-2, -1) + rpe, dim=-1)
    x = (attn @ v[:, None]).transpose(1, 2).reshape(B, nQ, C)
    x = x @ state["proj.weight"].T + state["proj.bias"]
    return x.permute(1, 0, 2), attn, tables
