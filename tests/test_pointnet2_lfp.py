"""PointnetLFPModuleMSG against the reference's own module (tests/golden/pointnet2_lfp.npz, written by
tools/make_pointnet2_lfp_golden.py): state-dict order (post_mlp first), train-mode output, gradients, running statistics and the
batch count of the shared post MLP (one per scale), eval-mode output — on CPU with the native ops routed to the C oracle (the host
logic is what is under test).  Tolerance: rtol 1e-3, atol 1e-4 x the reference's largest magnitude."""
import numpy as np
import pytest
import torch

import pointnet2_lfp_cases as K
from conftest import load_golden
from helpers import assert_close

RTOL, ATOL = 1e-3, 1e-4


@pytest.fixture(scope="module")
def golden():
    return load_golden("pointnet2_lfp")


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


def scales(name):
    return len(K.CASES[name][1]["mlps"])


def test_the_fixture_covers_the_listed_configurations(golden):
    assert sorted(str(c) for c in golden["cases"]) == sorted(K.CASES)
    for name in K.CASES:
        for key in K.CASES[name][2]:
            if key is not None:
                assert np.array_equal(K.make_inputs(name)[key].numpy(), golden[f"{name}/in/{key}"]), (name, key)
        assert f"{name}/in/features2" in golden.files or K.CASES[name][2][2] is None


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_state_dict_layout(name, golden):
    from vdetr_amd import pointnet2_modules as PM
    module = PM.PointnetLFPModuleMSG(**K.fresh_kwargs(name))
    sd = module.state_dict()
    keys = [str(k) for k in golden[f"{name}/keys"]]
    assert list(sd) == keys
    assert keys[0] == "post_mlp.layer0.conv.weight"  # the shared MLP is registered before the scales
    for k in keys:
        assert tuple(sd[k].shape) == golden[f"{name}/sd0/{k}"].shape, k


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_train_forward_backward_match_the_reference(name, golden, cpu_oracle_backend):
    from vdetr_amd import pointnet2_modules as PM
    module, names, keys = build(name, golden)
    module.train()
    wout = [torch.from_numpy(golden[f"{name}/wout/0"])]
    out, grads = K.run_case(module, golden_inputs(name, golden, names), names, wout)
    assert len(out) == 1 and out[0].shape == (2, scales(name) * K.CASES[name][1]["post_mlp"][-1], 9)  # N2 points, not N1
    close(out[0], golden[f"{name}/out/0"], f"{name}/out/0")
    assert set(grads) == {key for key in names if key is not None and "feat" in key}
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
    counted = 0
    for k in keys:
        if "num_batches" in k:
            assert int(sd[k]) == int(golden[f"{name}/after_train/{k}"]), k
            if k.startswith("post_mlp."):  # the shared MLP saw one batch per scale
                assert int(sd[k]) == scales(name), k
                counted += 1
        elif "running_" in k:
            close(sd[k], golden[f"{name}/after_train/{k}"], f"{name}: {k}")
    assert counted == (len(K.CASES[name][1]["post_mlp"]) - 1 if K.CASES[name][1].get("bn", True) else 0)
    assert module.last_paths == ["composition"] * (scales(name) + 1) and PM.LAST_PATHS == module.last_paths


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_eval_forward_matches_the_reference(name, golden, cpu_oracle_backend):
    module, names, _ = build(name, golden, "sd1")
    module.eval()
    with torch.no_grad():
        out, _ = K.run_case(module, golden_inputs(name, golden, names), names)
    close(out[0], golden[f"{name}/eval/0"], f"{name}/eval/0")
    assert module.last_paths == ["composition"] * (scales(name) + 1)  # CPU tensors never take the fused launches


def test_constructor_leaves_the_callers_lists_alone():
    from vdetr_amd import pointnet2_modules as PM
    mlps, post = [[4, 16], [4, 16]], [20, 24]
    two = [PM.PointnetLFPModuleMSG(mlps=mlps, radii=[0.5, 1.0], nsamples=[16, 32], post_mlp=post) for _ in range(2)]
    assert mlps == [[4, 16], [4, 16]] and post == [20, 24]
    assert two[1].mlps[0].layer0.conv.in_channels == 7 and two[1].post_mlp.layer0.conv.in_channels == 20


def test_widths_are_checked_by_the_convolution_not_the_constructor(cpu_oracle_backend):
    from vdetr_amd import pointnet2_modules as PM
    module = PM.PointnetLFPModuleMSG(mlps=[[4, 16]], radii=[0.5], nsamples=[16], post_mlp=[21, 24])  # 16 + 4 != 21
    inputs = K.make_inputs("lfp_two")
    with pytest.raises(RuntimeError):
        module(inputs["xyz2"], inputs["xyz"], inputs["features2"], inputs["features"])
