"""Convolutions over cross and dilated regions, the residual blocks of vdetr_amd.modules and MinkResNet's InstanceNorm stem on
the GPU, against the oracle's sparse convolution on a dictionary-built map and the float64 restatements of
tests/sparse_modules_restatement.py."""
import numpy as np
import pytest
import torch

import sparse_modules_restatement as R
from oracle import sparse_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _sites(n=600, seed=21, extent=6):
    return R.cloud(n, seed, extent=extent)


@pytest.mark.parametrize("cross,dilation,cin,cout", [(True, 1, 16, 24), (False, 2, 16, 24), (True, 2, 8, 64), (False, 2, 64, 128)])
def test_convolution_over_cross_and_dilated_regions(cross, dilation, cin, cout):
    """K = 7 and K = 27 with dilation 2 through the default pair path: forward, input and weight gradients against
    oracle.sparse_oracle.sparse_conv on the oracle's map of the generator's offsets (the bound of test_sparse_conv_forward_backward)"""
    from vdetr_amd import minkowski as ME
    from vdetr_amd import sparse_ops as S
    assert S._MODE == "pairs" and not S._IM2COL
    sites = _sites()
    gen = ME.KernelGenerator(3, 1, dilation, region_type=ME.RegionType.HYPER_CROSS if cross else ME.RegionType.HYPER_CUBE, dimension=3)
    assert gen.kernel_volume == (7 if cross else 27)
    torch.manual_seed(cin + cout)
    conv = ME.MinkowskiConvolution(cin, cout, kernel_size=3, dilation=dilation, kernel_generator=gen, dimension=3).to(DEV)
    f = torch.randn(len(sites), cin)
    g = torch.randn(len(sites), cout)
    fd = f.to(DEV).requires_grad_(True)
    x = ME.SparseTensor(fd, torch.from_numpy(sites).int().to(DEV))
    out = conv(x)
    (out.F * g.to(DEV)).sum().backward()
    keys = torch.from_numpy(O.pack_keys_np(sites))
    nbr = O.kernel_map(keys, keys, torch.tensor(gen.scaled_offsets(), dtype=torch.int32))
    assert torch.equal(nbr.long(), R.neighbour_table(sites, sites, R.scale_reach(R.cross_offsets(3) if cross else R.cube_offsets(3), dilation)))
    _, _, plan = x.coordinate_manager.kernel_map(x.keys, x.keys, 1, 1, gen, False)
    assert isinstance(plan, S.PairPlan) and plan.K == gen.kernel_volume and plan.P == int((nbr >= 0).sum())
    fr, wr = f.double().requires_grad_(True), conv.kernel.detach().cpu().double().requires_grad_(True)
    ref = O.sparse_conv(fr, wr, nbr)
    (ref * g.double()).sum().backward()
    for name, a, b in (("out", out.F, ref), ("dfeats", fd.grad, fr.grad), ("dweight", conv.kernel.grad, wr.grad)):
        scale = float(b.detach().abs().max())
        assert float((a.detach().cpu().double() - b.detach()).abs().max()) <= 1e-4 * scale + 1e-6, name
    # the eval fused path (pair products finished by the BatchNorm's gather-sum) at this K: the same bits as the composition
    bn = ME.MinkowskiBatchNorm(cout).to(DEV).eval()
    with torch.no_grad():
        bn.bn.running_mean.normal_()
        bn.bn.running_var.uniform_(0.5, 1.5)
        conv.eval()
        fused = bn(conv(x), act="relu").F
        assert ME.LAST_PATHS[-1] == "fused"
        ME.INFER_FUSED = False
        try:
            plain = bn(conv(x), act="relu").F
        finally:
            ME.INFER_FUSED = True
    assert torch.equal(fused, plain)


BLOCKS = [("BasicBlock", "BN", False), ("BasicBlockIN", "IN", False), ("BasicBlockINBN", "INBN", False),
          ("Bottleneck", "BN", True), ("BottleneckIN", "IN", True), ("BottleneckINBN", "INBN", True)]


def _block_case(cls_name, bottleneck, conv_type_name, dilation, stride):
    from vdetr_amd import minkowski as ME
    from vdetr_amd.modules import common as C, resnet_block as RB
    torch.manual_seed(5)
    cls = getattr(RB, cls_name)
    width = 16 * cls.expansion
    down = torch.nn.Sequential(ME.MinkowskiConvolution(16, width, kernel_size=1, stride=stride, dimension=3), ME.MinkowskiBatchNorm(width))
    block = cls(16, 16, stride=stride, dilation=dilation, downsample=down, conv_type=getattr(C.ConvType, conv_type_name), D=3).to(DEV)
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():  # norms that are no identity
        for name, p in block.named_parameters():
            if "kernel" not in name:
                p.copy_((torch.rand(p.shape, generator=gen) + 0.5) if name.endswith("weight") else torch.randn(p.shape, generator=gen) * 0.3)
    sites = _sites(700, 33)
    outs = R.strided_sites(sites, stride) if stride > 1 else sites
    offs = R.scale_reach(R.cross_offsets(3) if "CROSS" in conv_type_name else R.cube_offsets(3), dilation)
    strided_map = R.neighbour_table(sites, outs, offs)
    same_in = R.neighbour_table(sites, sites, [(0, 0, 0)])
    same_out = R.neighbour_table(outs, outs, [(0, 0, 0)])
    after = R.neighbour_table(outs, outs, R.scale_reach(offs, stride))  # stride-1 layers on the output sites: reach x tensor stride
    if bottleneck:
        maps = {"conv1": same_in, "conv2": strided_map, "conv3": same_out}
    else:
        maps = {"conv1": strided_map, "conv2": after}
    maps["downsample"] = R.neighbour_table(sites, outs, [(0, 0, 0)])
    return block, sites, outs, maps


@pytest.mark.parametrize("cls_name,kind,bottleneck,conv_type,dilation,stride",
                         [b + ("HYPERCUBE", 1, 2) for b in BLOCKS] + [("BasicBlockINBN", "INBN", False, "HYPERCROSS", 2, 1)])
def test_blocks_match_the_restatement(cls_name, kind, bottleneck, conv_type, dilation, stride):
    from vdetr_amd import minkowski as ME
    block, sites, outs, maps = _block_case(cls_name, bottleneck, conv_type, dilation, stride)
    g = torch.Generator().manual_seed(1)
    f = torch.randn(len(sites), 16, generator=g)
    gout = torch.randn(len(outs), 16 * type(block).expansion, generator=g)
    fd = f.to(DEV).requires_grad_(True)
    block.train()
    out = block(ME.SparseTensor(fd, torch.from_numpy(sites).int().to(DEV)))
    assert np.array_equal(out.C.cpu().numpy(), outs) and out.tensor_stride == stride
    (out.F * gout.to(DEV)).sum().backward()
    P = {k: v.detach().cpu().double().requires_grad_(v.is_floating_point()) for k, v in block.state_dict().items()}
    fr = f.double().requires_grad_(True)
    ref = R.block_forward(P, kind, bottleneck, fr, maps, R.scene_sizes(sites, 2), R.scene_sizes(outs, 2))
    (ref * gout.double()).sum().backward()

    def close(name, a, b, scale=None):
        scale = float(b.detach().abs().max()) if scale is None else scale
        assert float((a.detach().cpu().double().reshape(b.shape) - b.detach()).abs().max()) <= 1e-3 * scale + 1e-7, name

    close("out", out.F, ref)
    close("dfeats", fd.grad, fr.grad)
    for name, p in block.named_parameters():
        assert p.grad is not None, name
        scale = None
        if kind == "INBN" and name.startswith("norm") and ".0." in name:
            # A BatchNorm removes any per-channel affine map in front of it: the gradients of the InstanceNorm's weight and bias
            # are zero up to eps, the residue of a cancelling sum.  Relative to that residue 1e-3 would ask for more digits than
            # float32 holds; the scale is the same sum without the cancellation, the gradient of the BatchNorm's own parameter.
            sibling = P[name.replace(".0.", ".1.bn.")].grad
            scale = max(float(P[name].grad.abs().max()), float(sibling.abs().max()))
        close(name, p.grad, P[name].grad, scale)
    if kind == "BN":  # eval, no_grad: the fused inference form gives the bits of the composition
        block.eval()
        with torch.no_grad():
            x = ME.SparseTensor(f.to(DEV), torch.from_numpy(sites).int().to(DEV))
            ME.clear_last_paths()
            fused = block(x).F
            assert "fused" in ME.LAST_PATHS
            ME.INFER_FUSED = False
            try:
                plain = block(x).F
            finally:
                ME.INFER_FUSED = True
        assert torch.equal(fused, plain)


def test_mink_resnet_with_the_instance_norm_stem():
    from vdetr_amd import minkowski as ME
    from vdetr_amd.mink_resnet import MinkResNet
    torch.manual_seed(2)
    model = MinkResNet(18, 3, inplanes=16, stem_bn=False).to(DEV).train()
    with torch.no_grad():
        model.norm1.weight.uniform_(0.5, 1.5)
        model.norm1.bias.normal_()
    sites = R.cloud(3000, 4, extent=12)
    f = torch.randn(len(sites), 3)
    fd = f.to(DEV).requires_grad_(True)
    stem = {}
    hook = model.norm1.register_forward_hook(lambda m, i, o: stem.update(out=o.F.detach().cpu()))
    feats = model(ME.SparseTensor(fd, torch.from_numpy(sites).int().to(DEV)))
    hook.remove()
    assert [t.tensor_stride for t in feats] == [4, 8, 16, 32]
    sum(t.F.square().mean() for t in feats).backward()
    assert bool(torch.isfinite(fd.grad).all()) and float(fd.grad.abs().sum()) > 0
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert float(model.norm1.weight.grad.abs().sum()) > 0 and float(model.norm1.bias.grad.abs().sum()) > 0
    outs = R.strided_sites(sites, 2)
    nbr = R.neighbour_table(sites, outs, R.cube_offsets(3))
    conv = R.conv(f.double(), model.conv1.kernel.detach().cpu().double(), nbr)
    ref = R.instance_norm(conv, R.scene_sizes(outs, 2), model.norm1.weight.detach().cpu().double(), model.norm1.bias.detach().cpu().double())
    assert float((stem["out"].double() - ref).abs().max()) <= 1e-3 * float(ref.abs().max())
