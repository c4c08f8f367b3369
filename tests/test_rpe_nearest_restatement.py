"""rpe_quant "nearest_*" without a GPU: the restatement (tests/rpe_nearest_restatement.py) against F.grid_sample and against the
reference's own module (tests/golden/cross_attn_nearest*.npz, tools/make_rpe_nearest_golden.py), the module's constructor and
the descriptor field."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rpe_nearest_restatement as R
from conftest import load_golden
from helpers import args_ns, assert_close, grad_atol, t

CFG = SimpleNamespace(table_size=10, log_scale=512.0, max_value=4.0)
MARGIN = 1e-4


def grid_sample_bias(tables, vertices, xyz, cos_sin=None, max_value=4.0):
    """eight F.grid_sample(mode="nearest") passes, composed as models/vdetr_transformer.py:710-731 composes them"""
    B, nQ = vertices.shape[:2]
    nK = xyz.shape[1]
    rpe = 0
    for i in range(8):
        d = R.deltas(vertices[:, :, i:i + 1], xyz, cos_sin)[:, :, :, 0]
        d = torch.sign(d) * torch.log2(torch.abs(d) * 512.0 + 1.0) / math.log2(8) / max_value
        tab = tables[i][None].permute(0, 4, 1, 2, 3)
        rpe = rpe + F.grid_sample(tab, d.reshape(1, 1, 1, -1, 3), mode="nearest", align_corners=False) \
            .reshape(-1, B, nQ, nK).permute(1, 0, 2, 3)
    return rpe


def scene(seed, B, nQ, nK, rot, T=10):
    g = torch.Generator().manual_seed(seed)
    tables = torch.randn(8, T, T, T, 4, generator=g)
    xyz = 1 + torch.rand(B, nK, 3, generator=g) * torch.tensor([8.0, 6.0, 3.0])
    xyz[:, 0] = torch.tensor([30.0, 27.0, 14.0])     # beyond 8 m on both sides: zero padding
    xyz[:, 1] = torch.tensor([-25.0, -22.0, -9.0])
    verts = (1 + torch.rand(B, nQ, 1, 3, generator=g) * torch.tensor([8.0, 6.0, 3.0])) + (torch.rand(B, nQ, 8, 3, generator=g) - 0.5) * 2
    cs = R.yaw_cos_sin((torch.rand(B, nQ, generator=g) * 2 - 1) * 3.1) if rot else None
    cfg = SimpleNamespace(table_size=T, log_scale=512.0, max_value=4.0)
    return tables, verts, R.clean_keys(verts, xyz, cfg, MARGIN, g, cs), cs


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("T", [10, 6])
def test_restatement_equals_grid_sample(rot, T):
    tables, verts, xyz, cs = scene(3 + T, 2, 9, 40, rot, T)
    got = R.rpe_bias_nearest(tables, verts, xyz, cos_sin=cs)
    ref = grid_sample_bias(tables, verts, xyz, cs)
    # one cell per vertex, added in the same order: the same floats
    assert torch.equal(got, ref)
    assert float((got != 0).float().mean()) > 0.9


def test_edge_cases_of_the_cell_choice():
    """pix -0.3 / -0.5 -> cell 0, -0.6 -> 0; 9.3 -> cell 9, 9.6 -> 0 (T = 10); ties go to the even cell"""
    T = 10
    table = torch.zeros(8, T, T, T, 4, dtype=torch.float64)
    table[0] = (torch.arange(T, dtype=torch.float64) + 1)[None, None, :, None]  # value = x cell + 1, vertex 0 only

    def bias_at(pix):
        g = (2 * pix + 1) / T - 1                       # pix = ((g + 1) T - 1) / 2
        d = math.copysign((2.0 ** (abs(g) * 12) - 1) / 512, g)  # g = sign(d) log2(512 |d| + 1) / 12
        verts = torch.zeros(1, 1, 8, 3, dtype=torch.float64)
        verts[0, 0, 0, 0] = d
        # y, z deltas are 0: pix 4.5 there (cell 4), a valid cell
        return float(R.rpe_bias_nearest(table, verts, torch.zeros(1, 1, 3, dtype=torch.float64))[0, 0, 0, 0])

    for pix, want in [(-0.3, 1), (-0.5, 1), (-0.6, 0), (9.3, 10), (9.6, 0), (3.2, 4), (3.7, 5)]:
        assert bias_at(pix) == want, (pix, bias_at(pix), want)
    # the same five through grid_sample itself, x coordinate given directly
    tab = table[0][None].permute(0, 4, 1, 2, 3).float()
    for pix, want in [(-0.3, 1), (-0.5, 1), (-0.6, 0), (9.3, 10), (9.6, 0)]:
        grid = torch.tensor([(2 * pix + 1) / T - 1, 0.0, 0.0]).reshape(1, 1, 1, 1, 3)
        assert float(F.grid_sample(tab, grid, mode="nearest", align_corners=False)[0, 0, 0, 0, 0]) == want, pix


def test_fragile_finds_boundary_pairs_and_clean_keys_removes_them():
    g = torch.Generator().manual_seed(5)
    verts = torch.rand(1, 3, 8, 3, generator=g) * 4
    xyz = torch.rand(1, 50, 3, generator=g) * 4
    # a key placed so that its x delta to vertex 0 of query 0 has pix = 6.5 exactly (fp64) is fragile; the others mostly are not
    d = (2.0 ** (((2 * 6.5 + 1) / 10 - 1) * 12) - 1) / 512
    xyz[0, 7, 0] = verts[0, 0, 0, 0] - d
    fr = R.fragile(verts, xyz, CFG, 1e-4)
    assert fr[0, 0, 7] and fr.float().mean() < 0.05
    assert not R.fragile(verts, R.clean_keys(verts, xyz, CFG, 1e-4, g), CFG, 1e-4).any()
    # a key ON a vertex: delta exactly 0, pix exactly 4.5 everywhere -> not fragile
    xyz2 = R.clean_keys(verts, xyz, CFG, 1e-4, g)
    xyz2[0, 3] = verts[0, 1, 2]
    assert not R.fragile(verts, xyz2, CFG, 1e-4)[0, 1, 3]


class Case(dict):
    """one case of the fixture, keys without their prefix; `.files` as an npz file has it (helpers.grad_atol)"""
    files = property(lambda self: list(self))


def _case(name):
    g0 = load_golden("cross_attn_nearest")
    g = g0 if name == "plain" else load_golden("cross_attn_nearest_" + name)
    state = {k[6:]: torch.from_numpy(g0[k].astype(np.float32)) for k in g0.files if k.startswith("state:")}
    return state, Case((k[len(name) + 1:], g[k]) for k in g.files if k.startswith(name + ":"))


@pytest.mark.parametrize("name", ["plain", "rot"])
def test_restatement_reproduces_the_reference_module(name):
    state, c = _case(name)
    rot = str(c["angle_type"]) == "object_coords"
    ref_pts, xyz = t(c["reference_point"]), t(c["xyz"])
    angle = t(c["reference_angle"]) if rot else None
    # the fixture's inputs are clean, and hold the edge cases
    assert not R.fragile(ref_pts, xyz, CFG, MARGIN, R.yaw_cos_sin(angle) if rot else None).any()
    assert (ref_pts[:, 0, 0] == xyz[:, 0]).all() and float(xyz[:, 1].min()) > 13 and float(xyz[:, 2].max()) < -8
    st = {k: v.double().requires_grad_(True) for k, v in state.items()}
    x, attn, _ = R.cross_attention_nearest(st, t(c["query"]).double(), t(c["key"]).double(), ref_pts.double(),
                                           angle.double() if rot else None, xyz.double(), CFG)
    x.sum().backward()
    assert_close(x, c["x"], 1e-3, 1e-5, "x")
    assert_close(attn, c["attn"], 1e-3, 1e-7, "attn")
    for k in c:
        if k.startswith("grad_param:"):
            assert_close(st[k[11:]].grad, c[k], 1e-3, grad_atol(c, k, 2e-4), k)
    # the fp32 restatement picks the same cells as the fp64 one on these inputs
    tab = torch.randn(8, 10, 10, 10, 4, generator=torch.Generator().manual_seed(1))
    cs = R.yaw_cos_sin(angle) if rot else None
    b32 = R.rpe_bias_nearest(tab, ref_pts, xyz, cos_sin=cs).double()
    b64 = R.rpe_bias_nearest(tab.double(), ref_pts.double(), xyz.double(), cos_sin=None if cs is None else cs.double())
    assert float((b32 - b64).abs().max()) < 1e-5  # (another cell would be a difference of order 1; 8 fp32 additions: 1e-6)


@pytest.mark.parametrize("quant", ["nearest_4_10", "nearest_4_6"])
def test_module_constructs_with_nearest(quant):
    from vdetr_amd.vdetr_transformer import GlobalShareCrossAttention
    mod = GlobalShareCrossAttention(256, 4, attn_drop=0.1, proj_drop=0.1, args=args_ns(rpe_quant=quant))
    ref = GlobalShareCrossAttention(256, 4, attn_drop=0.1, proj_drop=0.1, args=args_ns(rpe_quant=quant.replace("nearest", "bilinear")))
    assert list(mod.state_dict().keys()) == list(ref.state_dict().keys())
    assert mod.rpe_cfg.interp == "nearest" and ref.rpe_cfg.interp == "bilinear"
    assert mod.rpe_cfg.table_size == int(quant.split("_")[2]) and mod.relative_coords_table.shape == ref.relative_coords_table.shape
    if quant == "nearest_4_10":  # the fixture's state dict loads
        state, _ = _case("plain")
        mod.load_state_dict(state, strict=False)


def test_other_interpolations_are_refused_by_name():
    from vdetr_amd import attention as A
    from vdetr_amd.vdetr_transformer import GlobalShareCrossAttention
    with pytest.raises(NotImplementedError, match="bilinear.*nearest"):
        GlobalShareCrossAttention(256, 4, args=args_ns(rpe_quant="bicubic_4_10"))
    with pytest.raises(NotImplementedError, match="bilinear.*nearest"):
        A.RPEConfig(interp="bicubic")
    assert A.RPEConfig().interp == "bilinear" and A.RPEConfig(10, 512.0, 4.0, "nearest").interp == "nearest"


def test_descriptor_field():
    from vdetr_amd import _lib
    assert _lib.AttnDesc.rpe_interp.offset == 44 and _lib.AttnDesc.rpe_interp.size == 4
    assert ctypes.sizeof(_lib.AttnDesc) == 168 and _lib.AttnDesc.vertices.offset == 48
    assert (_lib.VDETR_RPE_BILINEAR, _lib.VDETR_RPE_NEAREST) == (0, 1)
    lib = _lib.lib()
    assert lib.vdetr_abi_version() == 3
    d = _lib.AttnDesc()
    assert d.rpe_interp == 0  # a zeroed descriptor is bilinear
    d.kind, d.B, d.H, d.nQ, d.nK, d.scale = _lib.VDETR_ATTN_SHARED_KV, 1, 4, 4, 4, 0.125
    d.rpe_interp = 2
    assert lib.vdetr_rpe_bias_f32(ctypes.byref(d), None, None) == 1  # VDETR_ERR_ARG, before anything touches a device
    assert b"rpe_interp" in lib.vdetr_last_error()
    assert lib.vdetr_attn_fwd_f32(ctypes.byref(d), None, None, None, None, None, None, None, 0, None) == 1
    assert b"rpe_interp" in lib.vdetr_last_error()
    d.rpe_interp = -1
    assert lib.vdetr_attn_bwd_table_f32(ctypes.byref(d), None, None, None, 0, None) == 1
    assert b"rpe_interp" in lib.vdetr_last_error()
    # the field comes from RPEConfig at the one place that fills descriptors
    from vdetr_amd import attention as A
    tab = torch.zeros(8, 10, 10, 10, 4)
    v, x = torch.zeros(1, 4, 8, 3), torch.zeros(1, 4, 3)
    for interp, want in (("bilinear", 0), ("nearest", 1)):
        dd = A._desc(_lib.VDETR_ATTN_SHARED_KV, 1, 4, 4, 4, 0.125, tab, A.RPEConfig(interp=interp), v, x, None, None, 0.0, None)
        assert dd.rpe_interp == want
