"""The generative FPN neck (woexpand_conv = False: MinkowskiGenerativeConvolutionTranspose up blocks whose skip add is a union add,
DESIGN 6.11) on the GPU: against the same modules on the CPU with the native entry points routed to the oracle and to
tests/sparse_union_restatement.py, through the whole model with and without a prepared geometry, in the fused eval form, and with
a MinkowskiPruning in the chain."""
import copy

import pytest
import torch

import sparse_union_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _clouds():
    torch.manual_seed(0)
    pts = torch.rand(3000, 3) * torch.tensor([2.0, 1.5, 0.8])
    return [(pts / 0.01, pts), (pts[:1200] / 0.01 + 5, pts[:1200] * 0.5)]


def _neck_modules(width=32):
    """MinkResNet18 at inplanes 16 with the three generative up blocks and the out block of ModelVDETR's neck"""
    from vdetr_amd import minkowski as ME
    from vdetr_amd.mink_resnet import MinkResNet
    from vdetr_amd.model_vdetr import ModelVDETR
    net = MinkResNet(18, 3, inplanes=16, num_stages=4, stem_bn=True)
    channels = [16, 32, 64, 128]
    ups = torch.nn.ModuleList([ModelVDETR._make_up_block(channels[i], channels[i - 1], False) for i in (3, 2, 1)])
    out_block = ModelVDETR._make_block(channels[0], width)
    return net, ME.fuse_activations(ups), ME.fuse_activations(torch.nn.ModuleList([out_block]))[0]


def _chain(ME, ups, out_block, stages):
    """backbone_forward's top-down loop: every level of the neck, then the out block's tensor"""
    x, levels = stages[-1], []
    for i, up in zip((2, 1, 0), ups):
        x = ME.sequential_add(up, x, stages[i])
        levels.append(x)
    return levels + [out_block(x)]


def test_generative_neck_equals_cpu_oracle(monkeypatch):
    from vdetr_amd import minkowski as ME
    data = _clouds()
    net, ups, out_block = _neck_modules()
    mods = torch.nn.ModuleList([net, ups, out_block]).train()
    mods_g = copy.deepcopy(mods).to(DEV)

    def run(mods, dev):
        net, ups, out_block = mods
        coords, feats = ME.batch_sparse_collate([(c.to(dev), f.to(dev)) for c, f in data])
        stages = net(ME.SparseTensor(feats, coordinates=coords))
        levels = _chain(ME, ups, out_block, stages)
        loss = sum(o.F.square().mean() for o in stages) + sum(o.F.square().mean() for o in levels)
        loss.backward()
        return stages, levels, loss.detach()

    stages_g, levels_g, loss_g = run(mods_g, DEV)
    with monkeypatch.context() as mp:
        R.route_to_cpu(mp)
        stages_c, levels_c, loss_c = run(mods, "cpu")
    for level, stage in zip(levels_c[:3], (stages_c[2], stages_c[1], stages_c[0])):  # every level took the union, not the skip's sites
        assert level.keys.shape[0] > stage.keys.shape[0] and level.tensor_stride == stage.tensor_stride
    assert levels_c[3].keys.shape[0] == levels_c[2].keys.shape[0]
    for og, oc in zip(stages_g + levels_g, stages_c + levels_c):
        assert torch.equal(og.keys.cpu(), oc.keys)
        scale = float(oc.F.detach().abs().max())
        assert float((og.F.detach().cpu() - oc.F.detach()).abs().max()) <= 1e-3 * scale
    assert abs(float(loss_g) - float(loss_c)) <= 1e-4 * abs(float(loss_c))
    gg, gc = mods_g[0].conv1.kernel.grad.cpu(), net.conv1.kernel.grad
    assert float((gg - gc).abs().max()) <= 2e-3 * float(gc.abs().max())


def _two_planes(sizes=(3000, 2000)):
    g = torch.Generator().manual_seed(1)
    clouds = []
    for n in sizes:  # points on two planes: a floor and a wall
        u = torch.rand((n, 2), generator=g)
        floor = torch.stack((u[:, 0] * 4, u[:, 1] * 3, torch.zeros(n)), 1)
        wall = torch.stack((u[:, 0] * 4, torch.zeros(n), u[:, 1] * 2.5), 1)
        clouds.append(torch.cat((floor[: n // 2], wall[n // 2:])).to(DEV) + 1.0)
    return {"point_clouds": clouds, "point_cloud_dims_min": torch.stack([c.min(0)[0] for c in clouds]),
            "point_cloud_dims_max": torch.stack([c.max(0)[0] for c in clouds])}


def test_full_model_with_the_generative_neck():
    """ModelVDETR with woexpand_conv = False: forward and backward run, gradients reach the stem, the first up block and the out
    block, and a geometry prepared ahead of time gives the same coordinates, features and gradients"""
    from vdetr_amd import minkowski as ME
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    from vdetr_amd.model_vdetr import build_vdetr, default_args
    torch.manual_seed(0)
    args = default_args(nqueries=32, dec_nlayers=2, preenc_npoints=256, woexpand_conv=False)
    model = build_vdetr(args, ScannetDatasetConfig(), "minkowski").to(DEV).train()
    assert isinstance(model.up_block_3[0], ME.MinkowskiGenerativeConvolutionTranspose)
    inputs = _two_planes()
    out = model(inputs)
    assert out["outputs"]["sem_cls_logits"].shape[:2] == (2, 32) and out["seed_xyz"].shape == (2, 256, 3)
    (out["outputs"]["sem_cls_logits"].sum() + out["outputs"]["center_normalized"].sum()).backward()
    params = dict(model.named_parameters())
    names = ("pre_encoder.conv1.kernel", "up_block_3.0.kernel", "out_block_0.0.kernel")
    for name in names:
        assert float(params[name].grad.abs().sum()) > 0, name
    runs = []
    for prepared in (False, True):
        extra = {"geometry": model.prepare_geometry(inputs)} if prepared else {}
        model.zero_grad(set_to_none=True)
        scenes = model.backbone_forward(dict(inputs, **extra))
        sum(f.square().sum() for _, f in scenes).backward()
        runs.append(([(c.clone(), f.detach().clone()) for c, f in scenes], [params[n].grad.clone() for n in names]))
        if prepared:  # the forward met the key tensors and maps of the geometry-only pass: three unions, on more sites than the skips'
            cm = extra["geometry"]
            assert len(cm._union_maps) == 3 and all(u.shape[0] > a.shape[0] for u, _, _, _, _, a, _ in cm._union_maps.values())
    (scenes_a, grads_a), (scenes_b, grads_b) = runs
    for (ca, fa), (cb, fb) in zip(scenes_a, scenes_b):
        assert torch.equal(ca, cb) and torch.equal(fa, fb)
    for ga, gb in zip(grads_a, grads_b):
        assert torch.equal(ga, gb)


def test_eval_mode_keeps_the_up_blocks_fused(monkeypatch):
    """eval + no_grad, INFER_FUSED True against False over the generative neck: every conv -> BatchNorm launch still fused (the last
    one of an up block without post_add: its add is the union add), |a - b| <= 8 * 2^-24 * M with the M of
    tests/test_gpu_sparse_infer.py at the last site of every level, the skip as its post_add"""
    from test_gpu_sparse_infer import U, _randomise, _reference
    from vdetr_amd import minkowski as ME
    from vdetr_amd import sparse_ops as S
    net, ups, out_block = _neck_modules()
    mods = torch.nn.ModuleList([net, ups, out_block])
    for i, m in enumerate(m for m in mods.modules() if isinstance(m, ME.MinkowskiBatchNorm)):
        _randomise(m, seed=i)
    mods.to(DEV).eval()
    coords, feats = ME.batch_sparse_collate([(c.to(DEV), f.to(DEV)) for c, f in _clouds()])
    with torch.no_grad():
        stages = net(ME.SparseTensor(feats, coordinates=coords))
        ME.clear_last_paths()
        fused = _chain(ME, ups, out_block, stages)
        assert ME.LAST_PATHS == ["fused"] * 7                   # two sites per up block, one in the out block
        monkeypatch.setattr(ME, "INFER_FUSED", False)
        ME.clear_last_paths()
        x, plain, sites = stages[-1], [], []
        for i, up in zip((2, 1, 0), ups):                      # `stages[i] + up(x)`, keeping the input of the block's last site
            h = up[2](up[1](up[0](x)))
            x = stages[i] + up[5](up[4](up[3](h)))
            sites.append((up[3], up[4], h, stages[i]))
            plain.append(x)
        sites.append((out_block[0], out_block[1], x, None))
        plain.append(out_block(x))
        assert ME.LAST_PATHS == ["composition"] * 7
        for a, b, (conv, bn, h, skip) in zip(fused, plain, sites):
            assert torch.equal(a.keys, b.keys) and a.F.shape == b.F.shape
            _, _, plan = h.coordinate_manager.kernel_map(h.keys, h.keys, h.tensor_stride, h.tensor_stride, conv._offsets, False)
            post = None
            if skip is not None:
                post = torch.zeros_like(b.F)
                post[torch.searchsorted(b.keys, skip.keys)] = skip.F
            _, M = _reference(S.pair_products(h.F, conv.kernel, plan), plan.slot, conv.out_channels, conv.bias, bn.bn.weight, bn.bn.bias,
                              bn.bn.running_mean, bn.bn.running_var, bn.bn.eps, None, post, 0)
            err = (a.F.double() - b.F.double()).abs()
            print(f"{a.keys.shape[0]} sites: bit-equal {torch.equal(a.F, b.F)}, max err / (2^-24 M) = {float((err / (U * M)).max()):.2f} (bound 8)")
            assert bool((err <= 8 * U * M).all())


def test_pruning_in_a_chain(monkeypatch):
    """generative up block -> MinkowskiPruning by the rows' norm against its median -> 3x3x3 convolution, train mode: the GPU against
    the patched CPU run.  The mask is data on either side, so a row whose norm sits on the median could be kept by one and dropped
    by the other.  Two fp32 evaluations of a row (sums of 8 x 128 products, a BatchNorm, an ELU) differ by a few 2^-24 sqrt(1024) of
    the largest value, about 4e-6; the case is checked to have no second row within 1e-5 of the largest norm around the median
    (the next one is 1e-4 away)"""
    from vdetr_amd import minkowski as ME
    from vdetr_amd.model_vdetr import ModelVDETR
    data = _clouds()
    torch.manual_seed(1)  # (the modules of this seed give such a case; those of seed 0 put a second row 3e-8 from the median)
    net, _, _ = _neck_modules()
    up = ME.fuse_activations(torch.nn.ModuleList([ModelVDETR._make_up_block(128, 64, False)]))[0]
    conv = ME.MinkowskiConvolution(64, 32, kernel_size=3, dimension=3)
    mods = torch.nn.ModuleList([net, up, conv]).train()
    mods_g = copy.deepcopy(mods).to(DEV)

    def run(mods, dev):
        net, up, conv = mods
        coords, feats = ME.batch_sparse_collate([(c.to(dev), f.to(dev)) for c, f in data])
        x = up(net(ME.SparseTensor(feats, coordinates=coords))[3])
        norm = x.F.detach().norm(dim=1)
        pruned = ME.MinkowskiPruning()(x, norm > norm.median())
        y = conv(pruned)
        y.F.square().mean().backward()
        return x, norm, pruned, y

    x_g, norm_g, pruned_g, y_g = run(mods_g, DEV)
    with monkeypatch.context() as mp:
        R.route_to_cpu(mp)
        x_c, norm_c, pruned_c, y_c = run(mods, "cpu")
    near = (norm_c - norm_c.median()).abs() <= 1e-5 * float(norm_c.max())
    assert int(near.sum()) == 1, "a row's norm next to the median: the two sides' masks may differ"
    assert 0 < pruned_c.keys.shape[0] < x_c.keys.shape[0] and torch.equal(pruned_c.keys, x_c.keys[norm_c > norm_c.median()])
    for og, oc in ((x_g, x_c), (pruned_g, pruned_c), (y_g, y_c)):
        assert torch.equal(og.keys.cpu(), oc.keys)
        assert float((og.F.detach().cpu() - oc.F.detach()).abs().max()) <= 1e-3 * float(oc.F.detach().abs().max())
    for m in (mods_g, mods):
        assert float(m[1][0].kernel.grad.abs().sum()) > 0 and float(m[0].conv1.kernel.grad.abs().sum()) > 0
