"""pointnet2_modules / pytorch_utils against the reference's own modules (tests/golden/pointnet2_modules.npz, written by
tools/make_pointnet2_modules_golden.py): state-dict layout, sampled indices, train-mode outputs, running statistics, gradients and
eval-mode outputs, on CPU with the native ops routed to the C oracle (the host logic is what is under test)."""
import numpy as np
import pytest
import torch

import pointnet2_modules_cases as K
from conftest import load_golden
from helpers import assert_close

RTOL, ATOL = 5e-4, 1e-4  # atol is relative to the tensor's largest magnitude (test_host_vs_reference.py's form for fixture gradients)


@pytest.fixture(scope="module")
def golden():
    return load_golden("pointnet2_modules")


def close(actual, expected, what):
    expected = np.asarray(expected)
    assert_close(actual, expected, RTOL, ATOL * max(float(np.abs(expected).max()), 1e-30), what)


def build(name, golden, state="sd0"):
    from vdetr_amd import pointnet2_modules as PM
    cls, _, names = K.CASES[name]
    module = getattr(PM, cls)(**K.fresh_kwargs(name))
    keys = [str(k) for k in golden[f"{name}/keys"]]
    module.load_state_dict({k: torch.from_numpy(golden[f"{name}/{state}/{k}"].copy()) for k in keys})
    return module, names, keys


def golden_inputs(name, golden, names):
    return {key: torch.from_numpy(golden[f"{name}/in/{key}"].copy()) for key in names if key is not None}


def test_the_fixture_covers_the_listed_configurations(golden):
    assert sorted(str(c) for c in golden["cases"]) == sorted(K.CASES)
    for name in K.CASES:  # the seeded inputs of the case table are the fixture's
        for key in K.CASES[name][2]:
            if key is not None:
                assert np.array_equal(K.make_inputs(name)[key].numpy(), golden[f"{name}/in/{key}"]), (name, key)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_state_dict_layout(name, golden):
    from vdetr_amd import pointnet2_modules as PM
    module = getattr(PM, K.CASES[name][0])(**K.fresh_kwargs(name))
    sd = module.state_dict()
    keys = [str(k) for k in golden[f"{name}/keys"]]
    assert list(sd) == keys
    for k in keys:
        assert tuple(sd[k].shape) == golden[f"{name}/sd0/{k}"].shape, k
    if K.CASES[name][1].get("bn", True):
        assert not any(k.endswith("conv.bias") for k in keys)
    else:
        assert any(k.endswith("conv.bias") for k in keys) and not any(".bn." in k for k in keys)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_train_forward_backward_match_the_reference(name, golden, cpu_oracle_backend):
    module, names, keys = build(name, golden)
    module.train()
    n_out = sum(1 for k in golden.files if k.startswith(f"{name}/out/"))
    wout = [torch.from_numpy(golden[f"{name}/wout/{i}"]) if f"{name}/wout/{i}" in golden.files else None for i in range(n_out + 1)]
    out, grads = K.run_case(module, golden_inputs(name, golden, names), names, wout)
    for i, o in enumerate(out):
        key = f"{name}/out/{i}"
        if o is None:
            assert key not in golden.files
        elif not o.is_floating_point() or not o.requires_grad:  # sampled indices and the centres gathered by them: equal
            assert np.array_equal(o.detach().numpy(), golden[key]), key
        else:
            close(o, golden[key], key)
    for key, g in grads.items():
        close(g, golden[f"{name}/grad_in/{key}"], f"{name}: d {key}")
    for pname, p in module.named_parameters():
        close(p.grad, golden[f"{name}/grad_param/{pname}"], f"{name}: d {pname}")
    sd = module.state_dict()
    for k in keys:
        if "num_batches" in k:
            assert int(sd[k]) == int(golden[f"{name}/after_train/{k}"])
        elif "running_" in k:
            close(sd[k], golden[f"{name}/after_train/{k}"], f"{name}: {k}")
    from vdetr_amd import pointnet2_modules as PM
    assert set(PM.LAST_PATHS) == {"composition"} and module.last_paths == PM.LAST_PATHS


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_eval_forward_matches_the_reference(name, golden, cpu_oracle_backend):
    module, names, _ = build(name, golden, "sd1")
    module.eval()
    with torch.no_grad():
        out, _ = K.run_case(module, golden_inputs(name, golden, names), names)
    for i, o in enumerate(out):
        key = f"{name}/eval/{i}"
        if o is None:
            assert key not in golden.files
        elif not o.is_floating_point() or i == 0 and o.shape[-1] == 3 and len(out) > 1:
            assert np.array_equal(o.numpy(), golden[key]), key
        else:
            close(o, golden[key], key)
    assert set(module.last_paths) == {"composition"}  # CPU tensors never take the fused launch


def test_constructors_leave_the_callers_lists_alone():
    from vdetr_amd import pointnet2_modules as PM
    mlp, mlps, post = [4, 16, 32], [[4, 8], [4, 16]], [20, 12]
    PM.PointnetSAModuleVotes(mlp=mlp, npoint=7, radius=0.6, nsample=16)
    PM.PointnetSAModule(mlp=mlp, npoint=7, radius=0.6, nsample=16)
    PM.PointnetSAModuleMSG(npoint=5, radii=[0.5, 1.0], nsamples=[16, 32], mlps=mlps)
    PM.PointnetSAModuleMSGVotes(npoint=5, radii=[0.5, 1.0], nsamples=[16, 32], mlps=mlps)
    PM.PointnetFPModule(mlp=post)
    assert mlp == [4, 16, 32] and mlps == [[4, 8], [4, 16]] and post == [20, 12]
    two = [PM.PointnetSAModule(mlp=mlp, npoint=7, radius=0.6, nsample=16) for _ in range(2)]
    assert two[1].mlps[0].layer0.conv.in_channels == 7  # the reference would have made this 10


def test_votes_module_accepts_given_indices_and_returns_unique_counts(cpu_oracle_backend):
    from vdetr_amd import pointnet2_modules as PM
    torch.manual_seed(0)
    xyz, feats = torch.rand(2, 50, 3), torch.randn(2, 4, 50)
    inds = torch.arange(7, dtype=torch.int32).repeat(2, 1).contiguous()
    m = PM.PointnetSAModuleVotes(mlp=[4, 16], npoint=7, radius=0.3, nsample=16, sample_uniformly=True, ret_unique_cnt=True)
    new_xyz, new_feats, got_inds, cnt = m(xyz, feats, inds)
    assert got_inds is inds and torch.equal(new_xyz, xyz[:, :7]) and new_feats.shape == (2, 16, 7)
    assert cnt.shape == (2, 7) and (cnt >= 1).all() and (cnt <= 16).all()


def test_switch_and_path_record_are_module_attributes():
    from vdetr_amd import pointnet2_modules as PM
    assert PM.FUSED is True and isinstance(PM.LAST_PATHS, list) and isinstance(PM.FUSED_LAUNCHES, int)


def test_shared_mlp_blocks():
    from vdetr_amd import pytorch_utils as PT
    m = PT.SharedMLP([3, 8, 16], bn=True)
    assert list(m.state_dict())[:2] == ["layer0.conv.weight", "layer0.bn.bn.weight"]
    assert [type(c).__name__ for c in m.layer0.children()] == ["Conv2d", "BatchNorm2d", "ReLU"]
    pre = PT.SharedMLP([3, 8, 16], bn=True, preact=True, first=True)
    assert [n for n, _ in pre.layer0.named_children()] == ["conv"] and [n for n, _ in pre.layer1.named_children()] == ["bn", "activation", "conv"]
    assert pre.layer1.bn.bn.num_features == 8
    assert list(PT.FC(4, 6, bn=True).state_dict())[0] == "fc.weight" and "fc.bias" in PT.FC(4, 6).state_dict()
    assert "conv.bias" in PT.Conv1d(4, 6).state_dict() and "conv.bias" not in PT.Conv1d(4, 6, bn=True).state_dict()
    assert PT.BatchNorm1d(5)(torch.randn(4, 5, 9)).shape == (4, 5, 9)
