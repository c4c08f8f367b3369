"""InstanceNorm of a sparse tensor on the GPU (csrc/sp_inorm.hip through sparse_ops.instance_norm and MinkowskiInstanceNorm)
against the float64 restatement, under the tolerance rule of tests/norm_cases.py (imported, not restated): FACTOR x the error of
the float32 restatements over its summation orders + FACTOR x ulp32 + the term of the columns whose variance is exactly 0."""
import numpy as np
import pytest
import torch

import norm_cases as NC
import sparse_modules_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("y", "dx", "dweight", "dbias")


def _segments(sizes):
    return torch.tensor(np.concatenate(([0], np.cumsum(sizes))), dtype=torch.int32)


def _run(case):
    from vdetr_amd import sparse_ops as S
    sizes = case["sizes"]
    x = case["x"].to(DEV).requires_grad_(True)
    w = case["gamma"][None].to(DEV).requires_grad_(True)   # [1, C], as MinkowskiInstanceNorm holds them
    b = case["beta"][None].to(DEV).requires_grad_(True)
    y = S.instance_norm(x, _segments(sizes).to(DEV), len(sizes), w, b, R.IN_EPS)
    y.backward(case["dy"].to(DEV))
    return {"y": y.detach().cpu(), "dx": x.grad.cpu(), "dweight": w.grad.cpu().reshape(-1), "dbias": b.grad.cpu().reshape(-1)}


@pytest.mark.parametrize("scenes,C", R.INORM_CASES)
def test_instance_norm_forward_backward(scenes, C):
    case = R.inorm_case(scenes, C)
    ref = R.inorm_reference(case)
    rests = R.inorm_restatements(case)
    got = _run(case)
    figures = NC.compare(got, ref, rests, NAMES, case["groups"], case["extra"], label=f"{scenes} C={C}")
    print(scenes, C, {k: f"{v[0]:.2e} (restatement {v[1]:.2e}, factor {v[2]:.2f})" for k, v in figures.items()})
    sizes = case["sizes"]
    if 1 in sizes:  # a scene with a single site gives the bias, exactly
        a = sum(sizes[:sizes.index(1)])
        assert torch.equal(got["y"][a], case["beta"]) and bool((got["dx"][a] == 0).all())
    again = _run(case)
    assert all(torch.equal(got[k], again[k]) for k in NAMES), "two runs must agree bit for bit"


def test_arguments_are_checked():
    from vdetr_amd import sparse_ops as S
    x = torch.zeros((10, 8), device=DEV)
    seg = torch.tensor([0, 10], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        S.instance_norm(x.cpu(), seg, 1)
    with pytest.raises(RuntimeError):
        S.instance_norm(x.double(), seg, 1)
    with pytest.raises(RuntimeError):
        S.instance_norm(x[:, ::2], seg, 1)
    with pytest.raises(RuntimeError):
        S.instance_norm(x, seg, 2)
    with pytest.raises(RuntimeError, match="C=6"):
        S.instance_norm(torch.zeros((10, 6), device=DEV), seg, 1)
    assert S.instance_norm(torch.zeros((0, 8), device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), 1).shape == (0, 8)


def _sparse_case(sizes, C, batch_ids):
    """a SparseTensor whose scenes have the given sizes (batch indices `batch_ids`), rows in site order"""
    rng = np.random.default_rng(sum(sizes))
    coords = []
    for b, n in zip(batch_ids, sizes):
        cells = rng.choice(20 ** 3, size=n, replace=False)
        coords.append(np.stack((np.full(n, b), cells // 400 - 10, (cells // 20) % 20 - 10, cells % 20 - 10), 1))
    sites = R.sort_sites(np.concatenate(coords))
    return sites


@pytest.mark.parametrize("sizes,batch_ids", [((260, 1, 90), (0, 1, 2)), ((120, 75), (0, 2))])
def test_module_matches_and_reads_nothing_back(sizes, batch_ids):
    """MinkowskiInstanceNorm on a batch with a single-site scene / with batch index 1 absent; forward and backward contain no
    device-to-host read (torch's sync debug mode, shown first to raise on a plain .item())"""
    from vdetr_amd import minkowski as ME
    C = 20
    sites = _sparse_case(sizes, C, batch_ids)
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(len(sites), C, generator=g) * 2 + 1
    dy = torch.randn(len(sites), C, generator=g)
    norm = ME.MinkowskiInstanceNorm(C).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(torch.rand(1, C, generator=g) + 0.5)
        norm.bias.copy_(torch.randn(1, C, generator=g))
    xf = feats.to(DEV).requires_grad_(True)
    cm = ME.SparseTensor(xf.detach(), torch.from_numpy(sites).int().to(DEV)).coordinate_manager
    assert cm.num_scenes == max(batch_ids) + 1
    x = ME.SparseTensor(xf, coordinate_manager=cm, tensor_stride=1)  # (the sites are sorted: row order = site order)
    dyd = dy.to(DEV)
    norm(x).F.backward(dyd)  # (first call: builds the segment table of this key set; libraries and allocator warm)
    torch.cuda.synchronize()
    norm.zero_grad()
    xf.grad = None
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            raises = False
        except RuntimeError:
            raises = True
        if raises:
            y = norm(x)
            y.F.backward(dyd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raises:
        y = norm(x)
        y.F.backward(dyd)
    full = [0] * (max(batch_ids) + 1)
    for b, n in zip(batch_ids, sizes):
        full[b] = n
    ref = R.inorm_eval(feats, full, norm.weight.detach().cpu().reshape(-1), norm.bias.detach().cpu().reshape(-1), dy)
    rests = [R.inorm_eval(feats, full, norm.weight.detach().cpu().reshape(-1), norm.bias.detach().cpu().reshape(-1), dy, dtype=R.F32,
                          order=o) for o in NC.ORDERS]
    got = {"y": y.F.detach().cpu(), "dx": xf.grad.cpu(), "dweight": norm.weight.grad.cpu().reshape(-1),
           "dbias": norm.bias.grad.cpu().reshape(-1)}
    NC.compare(got, ref, rests, NAMES)
    assert norm.weight.grad.shape == (1, C) and list(norm.state_dict()) == ["weight", "bias"]
    if 1 in sizes:
        a = sum(sizes[:sizes.index(1)])
        assert torch.equal(got["y"][a], norm.bias.detach().cpu().reshape(-1))
    with ME.geometry_only():
        assert norm(x) is x
    if not raises:
        pytest.skip("this runtime ignores torch.cuda.set_sync_debug_mode: the no-host-read check did not run (parity did, and passed)")
