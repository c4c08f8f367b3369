"""The PointNet++ layers on the device: the composition in train mode against the reference's fixture, and the fused eval
forward (csrc/group_mlp.hip) against an fp64 torch evaluation of the composition on the same neighbour indices (folded BatchNorm
computed in fp64).  Tolerance everywhere: rtol 1e-3, atol 1e-4 x the reference's largest magnitude (the project's 1e-3 contract)."""
import numpy as np
import pytest
import torch

import pointnet2_modules_cases as K
from conftest import load_golden
from helpers import assert_close

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-3, 1e-4
DEV = "cuda:0"


def close(actual, expected, what):
    expected = expected.detach().cpu().double().numpy() if isinstance(expected, torch.Tensor) else np.asarray(expected, np.float64)
    scale = max(float(np.abs(expected).max()), 1e-30)
    err = float(np.abs(actual.detach().cpu().double().numpy() - expected).max())
    print(f"{what}: max abs err {err:.3e}, |ref| max {scale:.3e}")
    assert_close(actual, expected, RTOL, ATOL * scale, what)


# ---- the fp64 evaluation of the composition --------------------------------------------------------------------------------------
def mlp64(mlp, x, training=False):
    """a SharedMLP on x [B, C, ...] in fp64: 1x1 convolution, BatchNorm (running statistics, or the batch's), ReLU"""
    for block in mlp:
        conv = block.conv
        w = conv.weight.detach().double().reshape(conv.out_channels, conv.in_channels)
        x = torch.einsum("oi,bi...->bo...", w, x)
        shape = (1, -1) + (1,) * (x.dim() - 2)
        if conv.bias is not None:
            x = x + conv.bias.detach().double().reshape(shape)
        if hasattr(block, "bn"):
            bn = block.bn.bn
            if training:
                dims = [d for d in range(x.dim()) if d != 1]
                mean, var = x.mean(dims), x.var(dims, unbiased=False)
            else:
                mean, var = bn.running_mean.double(), bn.running_var.double()
            x = (x - mean.reshape(shape)) / torch.sqrt(var.reshape(shape) + bn.eps) * bn.weight.detach().double().reshape(shape) \
                + bn.bias.detach().double().reshape(shape)
        x = torch.relu(x)
    return x


def grouped64(grouper, xyz, new_xyz, features, idx):
    """QueryAndGroup's tensor [B, (3 +) C, M, S] in fp64 for the given neighbour indices"""
    bi = torch.arange(xyz.shape[0], device=xyz.device)[:, None, None]
    il = idx.long()
    gx = (xyz.double()[bi, il] - new_xyz.double()[:, :, None, :]).permute(0, 3, 1, 2)
    if grouper.normalize_xyz:
        gx = gx / grouper.radius
    if features is None:
        return gx
    gf = features.double().permute(0, 2, 1)[bi, il].permute(0, 3, 1, 2)
    return torch.cat([gx, gf], 1) if grouper.use_xyz else gf


def sa64(grouper, mlp, xyz, new_xyz, features, pooling="max", training=False):
    from vdetr_amd import pointnet2_utils as PU
    idx = PU.ball_query(grouper.radius, grouper.nsample, xyz, new_xyz)
    act = mlp64(mlp, grouped64(grouper, xyz, new_xyz, features, idx), training)
    return (act.max(-1)[0] if pooling == "max" else act.mean(-1)), idx


def fp64(module, unknown, known, unknow_feats, known_feats):
    from vdetr_amd import pointnet2_modules as PM
    idx, weight = PM._three_weights(unknown, known)
    bi = torch.arange(unknown.shape[0], device=unknown.device)[:, None, None]
    near = known_feats.double().permute(0, 2, 1)[bi, idx.long()]                      # [B, n, 3, C2]
    x = (near * weight.double()[..., None]).sum(2).permute(0, 2, 1)                   # [B, C2, n]
    if unknow_feats is not None:
        x = torch.cat([x, unknow_feats.double()], 1)
    return mlp64(module.mlp, x)


def scene(seed, B, N, C, isolated=4):
    """points of the unit cube with a few far outliers (FPS takes them first: balls of one point) and seeded features"""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(B, N, 3, generator=g)
    xyz[:, :isolated] += 5.0 + torch.arange(isolated, dtype=torch.float32)[None, :, None]
    feats = torch.randn(B, C, N, generator=g) if C else None
    return xyz.to(DEV), (feats.to(DEV) if C else None)


def randomise(module, seed, negative=True):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                w = torch.randn(m.weight.shape, generator=g)
                m.weight.copy_(w if negative else w.abs() + 0.1)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.5)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
            elif isinstance(m, torch.nn.Conv2d) and m.bias is not None:
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)


# case -> (B, N, M, S, C, mlp, radius, constructor extras, randomised BatchNorm?)
SA_CASES = {
    "i": (2, 300, 37, 16, 0, [0, 64, 128, 256], 0.3, dict(normalize_xyz=True), False),
    "ii": (1, 500, 64, 64, 3, [3, 32, 64], 0.35, dict(), False),
    "iii": (1, 400, 20, 16, 256, [256, 128, 128, 256], 0.25, dict(), False),
    "iv": (2, 200, 33, 32, 16, [16, 48], 0.45, dict(use_xyz=False, bn=False), True),
    "v": (2, 300, 37, 16, 0, [0, 64, 128, 256], 0.3, dict(normalize_xyz=True), True),
}


def sa_module(case, seed=0, **override):
    from vdetr_amd import pointnet2_modules as PM
    B, N, M, S, C, mlp, radius, extra, rand = SA_CASES[case]
    torch.manual_seed(seed)
    kw = dict(mlp=list(mlp), npoint=M, radius=radius, nsample=S, **extra)
    kw.update(override)
    module = PM.PointnetSAModuleVotes(**kw).to(DEV)
    if rand:
        randomise(module, seed + 1)
    xyz, feats = scene(seed + 2, B, N, C)
    return module, xyz, feats


def run_sa(module, xyz, feats, mode="infer"):
    if mode == "train":
        module.train()
    else:
        module.eval()
    if mode == "grad":
        return module(xyz, feats)
    with torch.no_grad():
        return module(xyz, feats)


def check_sa(module, xyz, feats, what, want_path, mode="infer"):
    ref = None
    if mode == "train":  # the batch's statistics do not depend on the running ones: reference first, the call then moves them
        new_xyz0, _ = _centres(module, xyz)
        ref, idx = sa64(module.grouper, module.mlp_module, xyz, new_xyz0, feats, module.pooling, True)
    new_xyz, got, inds = run_sa(module, xyz, feats, mode)
    assert module.last_paths == [want_path], (what, module.last_paths)
    if ref is None:
        ref, idx = sa64(module.grouper, module.mlp_module, xyz, new_xyz, feats, module.pooling, False)
    close(got, ref, what)
    return got, idx


def _centres(module, xyz):
    from vdetr_amd import pointnet2_modules as PM
    with torch.no_grad():
        return PM._sample_centres(xyz, module.npoint)


# ---- 1. train mode against the reference's fixture -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return load_golden("pointnet2_modules")


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_train_mode_matches_the_reference_fixture(name, golden):
    from vdetr_amd import pointnet2_modules as PM
    cls, _, names = K.CASES[name]
    module = getattr(PM, cls)(**K.fresh_kwargs(name))
    keys = [str(k) for k in golden[f"{name}/keys"]]
    module.load_state_dict({k: torch.from_numpy(golden[f"{name}/sd0/{k}"].copy()) for k in keys})
    module.to(DEV).train()
    inputs = {key: torch.from_numpy(golden[f"{name}/in/{key}"].copy()).to(DEV) for key in names if key is not None}
    n_out = 1 + sum(1 for k in golden.files if k.startswith(f"{name}/out/"))
    wout = [torch.from_numpy(golden[f"{name}/wout/{i}"]) if f"{name}/wout/{i}" in golden.files else None for i in range(n_out)]
    out, grads = K.run_case(module, inputs, names, wout)
    assert set(module.last_paths) == {"composition"}
    for i, o in enumerate(out):
        key = f"{name}/out/{i}"
        if o is None:
            assert key not in golden.files
        elif not o.is_floating_point() or not o.requires_grad:  # sampled indices and the centres gathered by them
            assert np.array_equal(o.detach().cpu().numpy(), golden[key]), key
        else:
            close(o, golden[key], key)
    for key, g in grads.items():
        close(g, golden[f"{name}/grad_in/{key}"], f"{name}: d {key}")
    for pname, p in module.named_parameters():
        close(p.grad, golden[f"{name}/grad_param/{pname}"], f"{name}: d {pname}")
    sd = module.state_dict()
    for k in keys:
        if "running_" in k:
            close(sd[k], golden[f"{name}/after_train/{k}"], f"{name}: {k}")


# ---- 2. the fused set abstraction against fp64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(SA_CASES))
def test_fused_set_abstraction_matches_fp64(case):
    module, xyz, feats = sa_module(case)
    _, idx = check_sa(module, xyz, feats, f"SA ({case})", "fused")
    S = idx.shape[-1]
    distinct = torch.tensor([[len(torch.unique(r)) for r in b] for b in idx.cpu()])
    assert (distinct == 1).any() and (distinct == S).any(), "the scene is meant to have balls of one point and overflowing ones"


def test_fused_set_abstraction_with_empty_balls():
    """centres with no point in reach: every slot of the ball query's row is index 0, and the kernel pools point 0's row"""
    from vdetr_amd import pointnet2_modules as PM
    module, xyz, feats = sa_module("ii")
    module.eval()
    g = torch.Generator().manual_seed(5)
    new_xyz = torch.rand(1, 21, 3, generator=g)
    new_xyz[:, ::3] += 50.0
    new_xyz = new_xyz.to(DEV)
    with torch.no_grad():
        layers = PM._sa_fusable(module, module.grouper, module.mlp_module, xyz, new_xyz, feats)
        assert layers is not None
        got = PM._sa_fused(module, 0, layers, module.grouper, xyz, new_xyz, feats)
    ref, idx = sa64(module.grouper, module.mlp_module, xyz, new_xyz, feats)
    assert (idx[:, ::3] == 0).all() and (idx[:, 1::3] != 0).any()
    close(got, ref, "SA (ii), empty balls")


# ---- 3. the fused feature propagation against fp64 -------------------------------------------------------------------------------
FP_CASES = {"i": (2, 130, 40, 16, 32, [48, 64, 32]), "ii": (1, 70, 3, 256, 256, [512, 256, 256]), "iii": (2, 130, 40, 0, 32, [32, 64, 32]),
            "iv": (1, 130, 2, 16, 32, [48, 64, 32])}


def fp_module(case, seed=0):
    from vdetr_amd import pointnet2_modules as PM
    B, n, m, C1, C2, mlp = FP_CASES[case]
    torch.manual_seed(seed)
    module = PM.PointnetFPModule(mlp=list(mlp)).to(DEV)
    randomise(module, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    unknown, known = torch.rand(B, n, 3, generator=g).to(DEV), torch.rand(B, m, 3, generator=g).to(DEV)
    known_feats = torch.randn(B, C2, m, generator=g).to(DEV)
    unknow_feats = torch.randn(B, C1, n, generator=g).to(DEV) if C1 else None
    return module, (unknown, known, unknow_feats, known_feats)


@pytest.mark.parametrize("case", sorted(FP_CASES))
def test_fused_feature_propagation_matches_fp64(case):
    module, args = fp_module(case)
    module.eval()
    with torch.no_grad():
        got = module(*args)
    assert module.last_paths == ["fused"]
    ref = fp64(module, *args)
    assert torch.isfinite(ref).all()
    close(got, ref, f"FP ({case})")


# ---- 4. the gate ------------------------------------------------------------------------------------------------------------------
def test_unsupported_calls_take_the_composition():
    for what, override, mode in [("nsample 6", dict(nsample=6), "infer"), ("avg pooling", dict(pooling="avg"), "infer"),
                                 ("train mode", dict(), "train"), ("autograd on", dict(), "grad"),
                                 ("width 40", dict(mlp=[3, 40]), "infer")]:
        module, xyz, feats = sa_module("ii", **override)
        check_sa(module, xyz, feats, f"gate: {what}", "composition", mode)
    module, args = fp_module("i")
    module.train()
    with torch.no_grad():
        module(*args)
    assert module.last_paths == ["composition"]
    module.eval()
    got = module(*args)  # autograd on
    assert module.last_paths == ["composition"]
    close(got, fp64(module, *args), "gate: FP with autograd on")


@pytest.mark.parametrize("case", sorted(SA_CASES))
def test_switch_off_takes_the_composition_and_agrees(case, monkeypatch):
    from vdetr_amd import pointnet2_modules as PM
    module, xyz, feats = sa_module(case)
    fused, _ = check_sa(module, xyz, feats, f"SA ({case}) fused", "fused")
    monkeypatch.setattr(PM, "FUSED", False)
    plain, _ = check_sa(module, xyz, feats, f"SA ({case}) composition", "composition")
    close(fused, plain, f"SA ({case}) fused vs composition")


def test_switch_off_feature_propagation(monkeypatch):
    from vdetr_amd import pointnet2_modules as PM
    for case in sorted(FP_CASES):
        module, args = fp_module(case)
        module.eval()
        with torch.no_grad():
            fused = module(*args)
            assert module.last_paths == ["fused"]
            monkeypatch.setattr(PM, "FUSED", False)
            plain = module(*args)
            assert module.last_paths == ["composition"]
            monkeypatch.setattr(PM, "FUSED", True)
        close(plain, fp64(module, *args), f"FP ({case}) composition")
        close(fused, plain, f"FP ({case}) fused vs composition")


# ---- 5. fresh weights -------------------------------------------------------------------------------------------------------------
def test_eval_forward_follows_an_optimizer_step_and_new_running_statistics():
    module, xyz, feats = sa_module("ii")
    before, _ = check_sa(module, xyz, feats, "before the step", "fused")  # fills the packed images
    opt = torch.optim.SGD(module.parameters(), lr=0.05)
    module.train()
    _, out, _ = module(xyz, feats)
    out.square().mean().backward()
    opt.step()
    with torch.no_grad():
        module(xyz, feats)  # another train-mode forward: the running statistics move again
    after, _ = check_sa(module, xyz, feats, "after the step", "fused")
    assert (after - before).abs().max().item() > 1e-3 * before.abs().max().item()
    fp, args = fp_module("i")
    fp.eval()
    with torch.no_grad():
        fp(*args)
    with torch.no_grad():
        for p in fp.parameters():
            p.mul_(1.25)
    with torch.no_grad():
        got = fp(*args)
    assert fp.last_paths == ["fused"]
    close(got, fp64(fp, *args), "FP after an in-place update")


# ---- 6. the multi-scale layers ----------------------------------------------------------------------------------------------------
def test_multi_scale_layers_fuse_every_scale():
    from vdetr_amd import pointnet2_modules as PM
    torch.manual_seed(3)
    xyz, feats = scene(11, 2, 300, 8)
    msg = PM.PointnetSAModuleMSG(npoint=29, radii=[0.15, 0.3], nsamples=[16, 32], mlps=[[8, 32, 64], [8, 48]]).to(DEV).eval()
    randomise(msg, 4)
    n0 = PM.FUSED_LAUNCHES
    with torch.no_grad():
        new_xyz, got = msg(xyz, feats)
    assert msg.last_paths == ["fused", "fused"] and PM.FUSED_LAUNCHES == n0 + 2
    ref = torch.cat([sa64(g, m, xyz, new_xyz, feats)[0] for g, m in zip(msg.groupers, msg.mlps)], 1)
    close(got, ref, "PointnetSAModuleMSG")
    votes = PM.PointnetSAModuleMSGVotes(npoint=29, radii=[0.15, 0.3], nsamples=[16, 32], mlps=[[8, 32, 64], [8, 48]]).to(DEV).eval()
    votes.load_state_dict(msg.state_dict())
    with torch.no_grad():
        vxyz, vgot, inds = votes(xyz, feats)
    assert votes.last_paths == ["fused", "fused"] and torch.equal(vxyz, new_xyz) and inds.shape == (2, 29)
    close(vgot, ref, "PointnetSAModuleMSGVotes")
