"""rpe_quant "nearest_*" on the GPU: the one-cell look-up in the forward kernels (attn_fwd_pipe.hip, attn_fwd.hip), the stand-alone
bias and both table-gradient kernels (attn_bwd.hip, attn_bwd_box4.hip), against the fp64 restatement
(tests/rpe_nearest_restatement.py) and the reference module's vectors (tests/golden/cross_attn_nearest*.npz).

Nearest is discontinuous, so every case but the random bias-level one runs on CLEAN inputs: no look-up coordinate within 1e-4 of a
cell boundary (the device's coordinate — hardware log2, fused multiply-add — is a few ulps, ~1e-6, off torch's)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rpe_nearest_restatement as R
from conftest import load_golden
from helpers import args_ns, assert_close, grad_atol, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 1e-4
SIGNS = torch.tensor([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]],
                     dtype=torch.float32)


def cfg_of(T=10):
    return SimpleNamespace(table_size=T, log_scale=512.0, max_value=4.0)


def scene(seed, B, nQ, nK, rot=False, T=10, clean=True, boxes=True):
    """keys in an 8 x 6 x 3 m room, two of them beyond 8 m on either side (zero padding), one ON a vertex (delta 0); boxes (with
    `rot`: boxes turned by the query's yaw, i.e. boxes in the look-up frame) or eight free vertices per query"""
    g = torch.Generator().manual_seed(seed)
    lo, ext = torch.tensor([1.0, 1.0, 1.0]), torch.tensor([8.0, 6.0, 3.0])
    xyz = lo + torch.rand((B, nK, 3), generator=g) * ext
    center = lo + torch.rand((B, nQ, 3), generator=g) * ext
    half = 0.1 + torch.rand((B, nQ, 3), generator=g)
    off = half[:, :, None, :] * SIGNS
    cs = None
    if rot:
        ang = (torch.rand((B, nQ), generator=g) * 2 - 1) * 3.1
        ang[:, 0] = 0.0  # the query of the delta-0 key stays unturned (tools/make_rpe_nearest_golden.py)
        cs = R.yaw_cos_sin(ang)
        c, s = cs[..., 0][:, :, None], cs[..., 1][:, :, None]
        off = torch.stack((off[..., 0] * c + off[..., 1] * s, -off[..., 0] * s + off[..., 1] * c, off[..., 2]), -1)
    verts = center[:, :, None, :] + off
    if not boxes:
        verts = verts + 0.3 * (torch.rand(verts.shape, generator=g) - 0.5)
    tables = torch.randn((8, T, T, T, 4), generator=g)
    xyz[:, 0] = verts[:, 0, 0]
    xyz[:, 1] = torch.tensor([30.0, 27.0, 14.0])
    xyz[:, 2] = torch.tensor([-25.0, -22.0, -9.0])
    if clean:
        xyz = R.clean_keys(verts, xyz, cfg_of(T), MARGIN, g, cs, keep=(0, 1, 2))
    return xyz, verts.contiguous(), tables, cs


# ---- the stand-alone bias against the fp64 restatement, random (NOT cleaned) keys --------------------------------------------------
# Fragile pairs (any of 24 coordinates within 1e-4 of a cell boundary, in fp64) are excluded, at most 0.5 % of the pairs.  Expected
# share for edge 10: 24 coordinates x 2e-4 = 0.48 %, less what lies outside the table.  Per case: (fragile pairs / pairs) counted with
# the restatement on the CPU; on the other pairs the fp32 restatement picks the fp64 one's cells in every case (0 differences).
BIAS_CASES = [
    # seed, B, nQ, nK, rot, T      fragile / pairs
    (1, 2, 5, 7, False, 10),     # 0 / 70
    (2, 2, 5, 7, True, 10),      # 0 / 70
    (3, 2, 37, 200, False, 10),  # 73 / 14800 = 0.49 %
    (4, 2, 37, 200, True, 10),   # 53 / 14800 = 0.36 %
    (5, 2, 37, 200, False, 6),   # 44 / 14800 = 0.30 %
]


@pytest.mark.parametrize("seed,B,nQ,nK,rot,T", BIAS_CASES)
def test_nearest_bias_kernel_vs_restatement(seed, B, nQ, nK, rot, T):
    from vdetr_amd import attention as A
    xyz, verts, tables, cs = scene(seed, B, nQ, nK, rot, T, clean=False, boxes=False)
    cfg = A.RPEConfig(T, 512.0, 4.0, "nearest")
    ref = R.rpe_bias_nearest(tables.double(), verts.double(), xyz.double(), cos_sin=None if cs is None else cs.double())
    fr = R.fragile(verts, xyz, cfg, MARGIN, cs)
    share = float(fr.float().mean())
    print(f"fragile pairs: {int(fr.sum())} / {fr.numel()} = {100 * share:.2f} %")
    assert share <= 0.005
    got = A.rpe_bias(tables.to(DEV), verts.to(DEV), xyz.to(DEV), cfg, None if cs is None else cs.to(DEV)).cpu().double()
    ok = ~fr[:, None].expand_as(ref)
    # 8 table values added in fp32: 8 roundings of at most 2^-24 of a partial sum <= 8 max|table|
    atol = 8 * 2.0 ** -24 * 8 * float(tables.abs().max())
    err = ((got - ref).abs() * ok).max()
    print(f"max |bias - restatement| on the other pairs: {float(err):.2e} (atol {atol:.2e})")
    assert float(err) <= atol
    assert float((ref != 0).double().mean()) > 0.5 and bool((ref[:, :, :, 1:3] == 0).all())  # the far keys: every vertex padded
    # nearest is not bilinear: the flag reaches the kernel
    bil = A.rpe_bias(tables.to(DEV), verts.to(DEV), xyz.to(DEV), A.RPEConfig(T, 512.0, 4.0), None if cs is None else cs.to(DEV)).cpu().double()
    assert float((bil - got).abs().max()) > 0.1


# ---- the reference module's vectors ----------------------------------------------------------------------------------------------
class Case(dict):
    files = property(lambda self: list(self))  # as an npz file has it (helpers.grad_atol)


def fixture_case(name):
    g0 = load_golden("cross_attn_nearest")
    g = g0 if name == "plain" else load_golden("cross_attn_nearest_" + name)
    state = {k[6:]: torch.from_numpy(g0[k].astype(np.float32)) for k in g0.files if k.startswith("state:")}
    return state, Case((k[len(name) + 1:], g[k]) for k in g.files if k.startswith(name + ":"))


@pytest.mark.parametrize("name", ["plain", "rot"])
def test_nearest_cross_attention_module_vs_reference_vectors(name):
    """forward (x, attn) and every stored gradient for the loss x.sum(), tolerances of test_gpu_attention.py's
    test_cross_attention_module_vs_reference_vectors"""
    from vdetr_amd.vdetr_transformer import GlobalShareCrossAttention
    state, c = fixture_case(name)
    angle_type = str(c["angle_type"])
    mod = GlobalShareCrossAttention(256, 4, attn_drop=0.1, proj_drop=0.1, args=args_ns(angle_type=angle_type, rpe_quant="nearest_4_10"))
    missing, unexpected = mod.load_state_dict(state, strict=False)
    assert set(missing) <= {"relative_coords_table"} and not unexpected
    mod = mod.eval().to(DEV)
    mod.return_attn = True
    query, key = t(c["query"], DEV, True), t(c["key"], DEV, True)
    angle = t(c["reference_angle"], DEV) if angle_type else None
    x, attn = mod(query, key, t(c["reference_point"], DEV), angle, t(c["xyz"], DEV))
    x.sum().backward()
    assert_close(x, c["x"], 1e-3, 1e-5, "x")
    assert_close(attn, c["attn"], 1e-3, 1e-7, "attn")
    grads = dict(("grad_param:" + n, p.grad) for n, p in mod.named_parameters())
    for k in c:
        if k.startswith("grad_param:"):
            assert_close(grads[k], c[k], 1e-3, grad_atol(c, k, 2e-4), k)


# ---- kernel agreement on clean inputs ----------------------------------------------------------------------------------------------
def reference_attention(q, k, v, tables, verts, xyz, cs, mask=None, keep=None, p=0.0):
    """fp64: softmax(0.125 q k^T + nearest bias (+ mask)) v with the heads sharing k / v; q, k, v, tables may require grad"""
    B, nQ = q.shape[:2]
    bias = R.rpe_bias_nearest(tables, verts.double(), xyz.double(), cos_sin=None if cs is None else cs.double())
    s = (q.reshape(B, nQ, 4, 64).permute(0, 2, 1, 3) * 0.125) @ k[:, None].transpose(-2, -1) + bias
    if mask is not None:
        s = s.masked_fill(mask[:, None], -100.0) if mask.dtype == torch.bool else s + mask[:, None].double()
    probs = torch.softmax(s, dim=-1)
    if keep is not None:
        probs = probs * keep.double() / (1.0 - p)
    return (probs @ v[:, None]).transpose(1, 2).reshape(B, nQ, 256)


def run_device(A, q, k, v, tables, verts, xyz, cs, wout, **kw):
    args = [x.to(DEV).requires_grad_(True) for x in (q, k, v, tables)]
    out = A.fused_attention(args[0], args[1], args[2], table=args[3], num_heads=4, scale=0.125, shared_kv=True,
                            rpe=A.RPEConfig(10, 512.0, 4.0, "nearest"), vertices=verts.to(DEV), xyz=xyz.to(DEV),
                            cos_sin=None if cs is None else cs.to(DEV), **kw)
    (out * wout.to(DEV)).sum().backward()
    return [out.detach().cpu()] + [a.grad.cpu() for a in args]


def run_reference(q, k, v, tables, verts, xyz, cs, wout, **kw):
    args = [x.double().requires_grad_(True) for x in (q, k, v, tables)]
    out = reference_attention(*args, verts, xyz, cs, **kw)
    (out * wout.double()).sum().backward()
    return [out.detach()] + [a.grad for a in args]


def operands(seed, B, nQ, nK, bf16_values=False):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(s, generator=g) for s in ((B, nQ, 256), (B, nK, 64), (B, nK, 64)))
    if bf16_values:
        q, k, v = (x.bfloat16().float() for x in (q, k, v))
    return q, k, v, torch.randn((B, nQ, 256), generator=g)


NAMES = ("out", "dq", "dk", "dv", "dtable")


def check_vs_reference(got, ref, what):
    """the tolerances test_gpu_attention.py applies against the fp64 oracle: out 1e-4 / 1e-5, gradients 1e-3 / 1e-4 of the largest entry"""
    for name, a, b in zip(NAMES, got, ref):
        if name == "out":
            assert_close(a, b.numpy(), 1e-4, 1e-5, f"{what} out")
        else:
            assert_close(a, b.numpy(), 1e-3, 1e-4 * float(b.abs().max()), f"{what} {name}")


@pytest.mark.parametrize("rot,nQ,nK", [(False, 64, 512), (True, 64, 512), (False, 37, 200)])
def test_nearest_kernels_agree(monkeypatch, rot, nQ, nK):
    """fwd_kernel 0 (persistent, split operands) and 2 (persistent, f32 matrix instructions) against 1 (grid); the box table-gradient
    kernel (bwd_kernel 0: chosen on the device; 2: vouched for) against the general one (1); all against the fp64 restatement.
    (37, 200): the last query quad and the last key tile are partial."""
    from vdetr_amd import attention as A
    B = 1
    xyz, verts, tables, cs = scene(20 + nQ + rot, B, nQ, nK, rot)
    q, k, v, wout = operands(7, B, nQ, nK)
    ref = run_reference(q, k, v, tables, verts, xyz, cs, wout)
    monkeypatch.setattr(A, "FWD_KERNEL", 1)
    monkeypatch.setattr(A, "BWD_KERNEL", 1)
    base = run_device(A, q, k, v, tables, verts, xyz, cs, wout)
    check_vs_reference(base, ref, "grid forward, general table gradient:")
    for fk in (0, 2):
        monkeypatch.setattr(A, "FWD_KERNEL", fk)
        got = run_device(A, q, k, v, tables, verts, xyz, cs, wout)
        # the same cells (one pix expression), so only the matrix products differ: 8e-6 relative for the split operands
        # (attn_fwd_pipe.hip), the f32 instructions in another order
        scale = float(base[0].abs().max())
        assert_close(got[0], base[0].numpy(), 1e-4, 2e-5 * scale, f"fwd_kernel {fk} out")
        check_vs_reference(got, ref, f"fwd_kernel {fk}:")
    monkeypatch.setattr(A, "FWD_KERNEL", 1)
    monkeypatch.setattr(A, "BWD_KERNEL", 0)  # boxes (in the look-up frame): the box kernel
    for boxes in ((False,) if rot else (False, True)):  # (True: bwd_kernel 2, the general kernel is not launched)
        got = run_device(A, q, k, v, tables, verts, xyz, cs, wout, vertices_are_boxes=boxes)
        for name, a, b in zip(NAMES[:4], got, base):
            assert torch.equal(a, b), f"{name} differs with the box table-gradient kernel"
        # both histograms are fixed point: 3e-4 of the largest entry, as test_box_backward_kernel_equals_general_kernel states
        assert float((got[4] - base[4]).abs().max()) <= 3e-4 * float(base[4].abs().max())
        check_vs_reference(got, ref, "box table gradient:")


def test_nearest_rounded_operand_forward(monkeypatch):
    """fwd_kernel 3 (operands rounded to bf16 in the kernel) against 1 on bf16-representable operands: what is left is P rounded
    to bf16 in front of PV — the 1e-2 the bf16 cases of test_gpu_attention.py state"""
    from vdetr_amd import attention as A
    B, nQ, nK = 1, 64, 512
    xyz, verts, tables, cs = scene(31, B, nQ, nK)
    q, k, v, wout = operands(8, B, nQ, nK, bf16_values=True)
    monkeypatch.setattr(A, "FWD_KERNEL", 1)
    base = run_device(A, q, k, v, tables, verts, xyz, cs, wout)
    monkeypatch.setattr(A, "FWD_KERNEL", 0)
    got = run_device(A, q, k, v, tables, verts, xyz, cs, wout, operand_bf16=True)
    assert_close(got[0], base[0].numpy(), 1e-2, 1e-2 * float(base[0].abs().max()), "fwd_kernel 3 out")
    assert not torch.equal(got[0], base[0])


@pytest.mark.parametrize("kind", ["bool", "float"])
def test_nearest_masks_through_the_grid_kernel(kind):
    from vdetr_amd import attention as A
    B, nQ, nK = 1, 64, 512
    xyz, verts, tables, cs = scene(41, B, nQ, nK)
    q, k, v, wout = operands(9, B, nQ, nK)
    g = torch.Generator().manual_seed(3)
    mask = torch.rand((B, nQ, nK), generator=g) < 0.3 if kind == "bool" else torch.randn((B, nQ, nK), generator=g)
    got = run_device(A, q, k, v, tables, verts, xyz, cs, wout, attn_mask=mask.to(DEV))
    check_vs_reference(got, run_reference(q, k, v, tables, verts, xyz, cs, wout, mask=mask), f"{kind} mask:")


def test_nearest_dropout_forward_and_backward_share_the_mask():
    from vdetr_amd import attention as A
    B, nQ, nK, p = 1, 64, 512, 0.1
    xyz, verts, tables, cs = scene(51, B, nQ, nK)
    q, k, v, wout = operands(10, B, nQ, nK)
    rng = A.begin_step(DEV)
    keep = A.dropout_keep_mask(B, 4, nQ, nK, True, p, rng, salt=5).cpu()
    assert abs(1.0 - float(keep.float().mean()) - p) < 0.01
    got = run_device(A, q, k, v, tables, verts, xyz, cs, wout, dropout_p=p, rng_state=rng, salt=5)
    check_vs_reference(got, run_reference(q, k, v, tables, verts, xyz, cs, wout, keep=keep, p=p), "dropout:")


def test_nearest_is_not_bilinear():
    """the same inputs in the two modes through the fused forward: a dispatch that ignored the flag would give equal outputs"""
    from vdetr_amd import attention as A
    B, nQ, nK = 1, 64, 512
    xyz, verts, tables, cs = scene(61, B, nQ, nK)
    q, k, v, _ = operands(11, B, nQ, nK)
    kw = dict(num_heads=4, scale=0.125, shared_kv=True, table=tables.to(DEV), vertices=verts.to(DEV), xyz=xyz.to(DEV))
    with torch.no_grad():
        near = A.fused_attention(q.to(DEV), k.to(DEV), v.to(DEV), rpe=A.RPEConfig(10, 512.0, 4.0, "nearest"), **kw)
        bil = A.fused_attention(q.to(DEV), k.to(DEV), v.to(DEV), rpe=A.RPEConfig(), **kw)
    assert float((near - bil).abs().max()) > 1e-2
