"""PointnetLFPModuleMSG on the device: the composition in train mode against the reference's fixture, and the eval forward with
the fused set-abstraction launches and the fused post-MLP launch (pw_mlp_kernel, csrc/group_mlp.hip) against an fp64 torch
evaluation of the composition on the same ball-query indices.  Tolerance everywhere: rtol 1e-3, atol 1e-4 x the reference's
largest magnitude (the project's 1e-3 contract)."""
import copy

import numpy as np
import pytest
import torch

import pointnet2_lfp_cases as K
from conftest import load_golden
from test_gpu_pointnet2_modules import ATOL, DEV, close, mlp64, randomise, sa64, scene

pytestmark = pytest.mark.gpu


# ---- the fp64 evaluation of the composition --------------------------------------------------------------------------------------
def lfp64(module, xyz2, xyz1, features2, features1, training=False):
    """per scale: fp64 set abstraction around xyz2 on the device's ball-query indices, concatenation, the shared post MLP (in train
    mode with each call's own batch statistics); then the concatenation over the scales"""
    outs = []
    for grouper, mlp in zip(module.groupers, module.mlps):
        pooled, _ = sa64(grouper, mlp, xyz1, xyz2, features1, "max", training)
        joint = pooled if features2 is None else torch.cat([pooled, features2.double()], 1)
        outs.append(mlp64(module.post_mlp, joint, training))
    return torch.cat(outs, 1)


# case -> sizes and constructor arguments.  What each is for:
#   i    148 rows: 32-row tiles straddle the scene boundary at 37 and the scale boundary at 74, the last tile is ragged; cin 20 is
#        padded to 32, width 48 to 64
#   ii   the longest contraction (512) and the widest LDS row
#   iii  no features2, three post layers, no BatchNorm
#   iv   five scales: two post launches (4 + 1)
LFP_CASES = {
    "i": dict(B=2, N1=300, N2=37, C1=8, C2=4, kw=dict(mlps=[[8, 16], [8, 16]], radii=[0.2, 0.4], nsamples=[16, 32], post_mlp=[20, 48])),
    "ii": dict(B=1, N1=400, N2=70, C1=8, C2=256, kw=dict(mlps=[[8, 64, 256]], radii=[0.25], nsamples=[16], post_mlp=[512, 256, 256])),
    "iii": dict(B=2, N1=200, N2=33, C1=8, C2=0, kw=dict(mlps=[[8, 32] for _ in range(3)], radii=[0.2, 0.3, 0.5], nsamples=[16, 32, 64],
                                                        post_mlp=[32, 64, 32, 16], bn=False)),
    "iv": dict(B=1, N1=200, N2=20, C1=4, C2=0, kw=dict(mlps=[[4, 16] for _ in range(5)], radii=[0.15, 0.2, 0.25, 0.3, 0.4], nsamples=[16] * 5,
                                                       post_mlp=[16, 16])),
}


def lfp_module(case, seed=0, **override):
    """(module with randomised BatchNorm (negative weights) and biases, (xyz2, xyz1, features2, features1)); every fifth centre lies
    far outside the scene: an empty ball"""
    from vdetr_amd import pointnet2_modules as PM
    c = LFP_CASES[case]
    kw = copy.deepcopy(c["kw"])
    kw.update(override)
    torch.manual_seed(seed)
    module = PM.PointnetLFPModuleMSG(**kw).to(DEV)
    randomise(module, seed + 1)
    xyz1, features1 = scene(seed + 2, c["B"], c["N1"], c["C1"])
    g = torch.Generator().manual_seed(seed + 3)
    xyz2 = torch.rand(c["B"], c["N2"], 3, generator=g)
    xyz2[:, ::5] += 50.0
    features2 = torch.randn(c["B"], c["C2"], c["N2"], generator=g).to(DEV) if c["C2"] else None
    return module, (xyz2.to(DEV), xyz1, features2, features1)


def infer(module, args):
    module.eval()
    with torch.no_grad():
        return module(*args)


# ---- 1. train mode against the reference's fixture -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return load_golden("pointnet2_lfp")


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_train_mode_matches_the_reference_fixture(name, golden):
    from vdetr_amd import pointnet2_modules as PM
    _, _, names = K.CASES[name]
    module = PM.PointnetLFPModuleMSG(**K.fresh_kwargs(name))
    keys = [str(k) for k in golden[f"{name}/keys"]]
    module.load_state_dict({k: torch.from_numpy(golden[f"{name}/sd0/{k}"].copy()) for k in keys})
    module.to(DEV).train()
    inputs = {key: torch.from_numpy(golden[f"{name}/in/{key}"].copy()).to(DEV) for key in names if key is not None}
    out, grads = K.run_case(module, inputs, names, [torch.from_numpy(golden[f"{name}/wout/0"])])
    nscales = len(module.groupers)
    assert module.last_paths == ["composition"] * (nscales + 1)
    close(out[0], golden[f"{name}/out/0"], f"{name}/out/0")
    for key, g in grads.items():
        close(g, golden[f"{name}/grad_in/{key}"], f"{name}: d {key}")
    gmax = max(float(np.abs(golden[k]).max()) for k in golden.files if k.startswith(f"{name}/grad_param/"))
    for pname, p in module.named_parameters():
        expected = golden[f"{name}/grad_param/{pname}"]
        if K.cancels_in_train_mode(name, pname):  # zero by construction: the fixture holds rounding noise, and so may the module
            assert float(np.abs(expected).max()) <= ATOL * gmax and p.grad.abs().max().item() <= ATOL * gmax, pname
        else:
            close(p.grad, expected, f"{name}: d {pname}")
    sd = module.state_dict()
    for k in keys:
        if "num_batches" in k:
            assert int(sd[k]) == int(golden[f"{name}/after_train/{k}"]) == (nscales if k.startswith("post_mlp.") else 1), k
        elif "running_" in k:
            close(sd[k], golden[f"{name}/after_train/{k}"], f"{name}: {k}")


# ---- 2. the fused eval forward against fp64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(LFP_CASES))
def test_fused_forward_matches_fp64(case):
    from vdetr_amd import pointnet2_modules as PM
    from vdetr_amd import pointnet2_utils as PU
    module, args = lfp_module(case)
    nscales = len(module.groupers)
    n0 = PM.FUSED_LAUNCHES
    got = infer(module, args)
    assert module.last_paths == ["fused"] * nscales + ["fused"] and PM.LAST_PATHS == module.last_paths
    assert PM.FUSED_LAUNCHES == n0 + nscales + (nscales + 3) // 4
    c = LFP_CASES[case]
    assert got.shape == (c["B"], nscales * c["kw"]["post_mlp"][-1], c["N2"])
    ref = lfp64(module, *args)
    assert torch.isfinite(ref).all()
    close(got, ref, f"LFP ({case})")
    idx = PU.ball_query(module.groupers[-1].radius, module.groupers[-1].nsample, args[1], args[0])
    assert (idx[:, ::5] == 0).all() and (idx[:, 1::5] != 0).any(), "every fifth centre is meant to have an empty ball"


# ---- 3. the two gates are independent ---------------------------------------------------------------------------------------------
def test_mixed_gates_agree_with_fp64():
    module, args = lfp_module("i", nsamples=[6, 32])
    got = infer(module, args)
    assert module.last_paths == ["composition", "fused", "fused"]
    close(got, lfp64(module, *args), "gate: nsample 6 on the first scale")
    module, args = lfp_module("i", post_mlp=[20, 40])
    got = infer(module, args)
    assert module.last_paths == ["fused", "fused", "composition"]
    close(got, lfp64(module, *args), "gate: post width 40")


def test_train_mode_autograd_and_the_switch_take_the_composition(monkeypatch):
    from vdetr_amd import pointnet2_modules as PM
    module, args = lfp_module("i")
    ref = lfp64(module, *args, training=True)  # the batch's statistics do not depend on the running ones the call then moves
    module.train()
    with torch.no_grad():
        got = module(*args)
    assert module.last_paths == ["composition"] * 3
    close(got, ref, "gate: train mode")
    module, args = lfp_module("i")
    module.eval()
    got = module(*args)  # autograd on
    assert module.last_paths == ["composition"] * 3 and got.requires_grad
    close(got, lfp64(module, *args), "gate: autograd on")
    monkeypatch.setattr(PM, "FUSED", False)
    got = infer(module, args)
    assert module.last_paths == ["composition"] * 3
    close(got, lfp64(module, *args), "gate: FUSED = False")


def test_switch_on_and_off_agree(monkeypatch):
    from vdetr_amd import pointnet2_modules as PM
    module, args = lfp_module("i")
    fused = infer(module, args)
    assert module.last_paths == ["fused"] * 3
    monkeypatch.setattr(PM, "FUSED", False)
    plain = infer(module, args)
    assert module.last_paths == ["composition"] * 3
    close(fused, plain, "LFP (i) fused vs composition")


def test_two_fused_calls_give_the_same_bits():
    module, args = lfp_module("i")
    a = infer(module, args)
    b = infer(module, args)
    assert module.last_paths == ["fused"] * 3 and torch.equal(a, b)


# ---- 4. fresh weights -------------------------------------------------------------------------------------------------------------
def test_eval_forward_follows_an_optimizer_step_and_new_running_statistics():
    module, args = lfp_module("i")
    before = infer(module, args)  # fills the packed images of the scales and of the post MLP
    assert module.last_paths == ["fused"] * 3
    close(before, lfp64(module, *args), "before the step")
    opt = torch.optim.SGD(module.parameters(), lr=0.05)
    module.train()
    module(*args).square().mean().backward()
    opt.step()
    with torch.no_grad():
        module(*args)  # another train-mode forward: the running statistics move again
    after = infer(module, args)
    assert module.last_paths == ["fused"] * 3
    close(after, lfp64(module, *args), "after the step")
    assert (after - before).abs().max().item() > 1e-3 * before.abs().max().item()
