"""The eval-mode form of the sparse backbone: vdetr_sp_gather_sum_bn_act_f32 against its formula in float64, the
convolution -> BatchNorm hand-over of vdetr_amd.minkowski against the composition of launches it replaces, and its gate."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
U = 2.0 ** -24


# ---- the kernel against the formula in float64 -----------------------------------------------------------------------------------
def _abs_sum(y, slot):
    """sum over a row's valid slots of |y[slot]|, in float64: [N, stride]"""
    valid = slot >= 0
    rows = y.abs().double()[slot.long().clamp(min=0)]            # [K, N, stride]
    return (rows * valid[..., None]).sum(0)


def _reference(y, slot, C, bias, gamma, beta, mean, var, eps, res, post, act):
    """section 1's formula from the same fp32 operands, evaluated in float64; returns (out, M) with M the magnitude the bound scales by"""
    n = slot.shape[1]
    valid = slot >= 0
    if y is None:
        acc = torch.zeros((n, C), dtype=torch.float64, device=slot.device)
        mag = torch.zeros_like(acc)
    else:
        rows = y.double()[slot.long().clamp(min=0)][..., :C]     # [K, N, C]: the padded columns are never read
        acc = torch.where(valid[..., None], rows, torch.zeros_like(rows)).sum(0)
        mag = _abs_sum(y[:, :C], slot)
    zero = torch.zeros(C, dtype=torch.float64, device=slot.device)
    b = bias.double().reshape(-1) if bias is not None else zero
    scale = (gamma.double() if gamma is not None else zero + 1) * torch.rsqrt(var.double() + float(torch.tensor(eps, dtype=torch.float32)))
    shift = (beta.double() if beta is not None else zero) - mean.double() * scale
    r = res.double() if res is not None else torch.zeros_like(acc)
    p = post.double() if post is not None else torch.zeros_like(acc)
    v = (acc + b) * scale + shift + r
    out = {0: v, 1: v.clamp(min=0), 2: torch.where(v > 0, v, torch.expm1(v))}[act] + p
    M = (mag + b.abs()) * scale.abs() + shift.abs() + r.abs() + p.abs() + 1
    return out, M


def _launch(y, slot, C, stride, bias, gamma, beta, mean, var, eps, res, post, act):
    """the entry point itself, writing into the middle of a buffer whose two ends must stay as they were"""
    from vdetr_amd import _lib as L
    n, guard = slot.shape[1], 1024
    buf = torch.full((n * C + 2 * guard,), -777.0, dtype=torch.float32, device=DEV)
    d = L.SpGsumBnDesc()
    d.K, d.nrows, d.C, d.src_stride, d.act, d.eps = slot.shape[0], n, C, stride, act, eps
    d.src, d.slot, d.out = L.ptr(y).value, slot.data_ptr(), buf.data_ptr() + 4 * guard
    d.conv_bias, d.gamma, d.beta = L.ptr(bias).value, L.ptr(gamma).value, L.ptr(beta).value
    d.running_mean, d.running_var, d.residual, d.post_add = mean.data_ptr(), var.data_ptr(), L.ptr(res).value, L.ptr(post).value
    L.check(L.lib().vdetr_sp_gather_sum_bn_act_f32(ctypes.byref(d), L.stream_ptr()), "sp_gather_sum_bn_act")
    torch.cuda.synchronize()
    assert bool((buf[:guard] == -777.0).all()) and bool((buf[-guard:] == -777.0).all()), "wrote outside [nrows, C]"
    return buf[guard:guard + n * C].view(n, C)


def _operands(n, K, C, stride, seed, one_per_row=False, pairs=True, res=False, post=False, bias=False, no_gamma=False, no_beta=False,
              neg_gamma=False, small_var=False):
    g = torch.Generator().manual_seed(seed)
    if not pairs:
        valid = torch.zeros((K, n), dtype=torch.bool)
    elif one_per_row:  # a transposed k = 2 layer: every output site has exactly one parent
        valid = torch.zeros((K, n), dtype=torch.bool)
        valid[torch.randint(0, K, (n,), generator=g), torch.arange(n)] = True
    else:
        valid = torch.rand((K, n), generator=g) < 0.15
        valid[:, torch.rand(n, generator=g) < 0.05] = False     # rows without a single pair
    P = int(valid.sum())
    slot = torch.full((K, n), -1, dtype=torch.int32)
    slot[valid] = torch.randperm(P, generator=g).int()
    y = None
    if P:
        y = torch.randn((P, stride), generator=g)
        y[:, C:] = float("nan")                                  # the GEMM's padding columns: reading one poisons the row
    rnd = lambda *s: torch.randn(*s, generator=g)                # noqa: E731
    gamma = None if no_gamma else (-rnd(C).abs() - 0.1 if neg_gamma else rnd(C))
    var = torch.rand(C, generator=g) + 0.5
    if small_var:
        var[::3] = 1e-6
    t = dict(y=y, slot=slot, bias=rnd(1, C) if bias else None, gamma=gamma, beta=None if no_beta else rnd(C) * 0.5,
             mean=rnd(C) * 0.5, var=var, res=rnd(n, C) if res else None, post=rnd(n, C) if post else None)
    return {k: (v.to(DEV).contiguous() if v is not None else None) for k, v in t.items()}


_KERNEL_CASES = [
    # nrows, K, C, src_stride, act, options
    (1, 27, 4, 4, 0, {}),
    (1, 27, 4, 4, 2, dict(res=True, post=True, bias=True)),
    (37, 27, 16, 16, 1, dict(res=True)),
    (37, 27, 16, 16, 2, dict(post=True, no_gamma=True, no_beta=True)),
    (1000, 8, 64, 64, 1, dict(one_per_row=True, res=True, bias=True)),
    (1000, 8, 64, 64, 0, dict(one_per_row=True, post=True, neg_gamma=True)),
    (257, 1, 100, 112, 2, dict(res=True, post=True, bias=True, small_var=True)),
    (257, 1, 100, 112, 1, dict(no_gamma=True)),
    (300, 27, 512, 512, 1, dict(res=True)),
    (300, 27, 512, 512, 2, dict(post=True, bias=True, neg_gamma=True, small_var=True)),
    (64, 27, 1024, 1024, 0, dict(bias=True, no_beta=True)),
    (64, 27, 1024, 1024, 2, dict(res=True, post=True, small_var=True)),
]


@pytest.mark.parametrize("n,K,C,stride,act,opts", _KERNEL_CASES,
                         ids=[f"{n}x{K}x{C}s{s}-act{a}-{'+'.join(sorted(o)) or 'plain'}" for n, K, C, s, a, o in _KERNEL_CASES])
def test_kernel_against_float64(n, K, C, stride, act, opts):
    """|got - ref| <= 64 * 2^-24 * M elementwise, M = (sum_k |y_k| + |bias|) |scale| + |shift| + |residual| + |post_add| + 1:
    at most K + 4 roundings, the few-ulp rsqrtf and expm1f, ELU's (-1, 0] range.  Derived, not measured."""
    t = _operands(n, K, C, stride, seed=n + K + C + act, **opts)
    got = _launch(t["y"], t["slot"], C, stride, t["bias"], t["gamma"], t["beta"], t["mean"], t["var"], EPS, t["res"], t["post"], act)
    ref, M = _reference(t["y"], t["slot"], C, t["bias"], t["gamma"], t["beta"], t["mean"], t["var"], EPS, t["res"], t["post"], act)
    err = (got.double() - ref).abs()
    print(f"max err / (2^-24 M) = {float((err / (U * M)).max()):.2f} (bound 64)")
    assert bool(torch.isfinite(got).all())
    assert bool((err <= 64 * U * M).all())
    again = _launch(t["y"], t["slot"], C, stride, t["bias"], t["gamma"], t["beta"], t["mean"], t["var"], EPS, t["res"], t["post"], act)
    assert torch.equal(got, again)                               # no atomics: the same bits


@pytest.mark.parametrize("act,bias", [(1, False), (2, True)])
def test_layer_without_a_pair(act, bias):
    """P == 0 with src NULL: out = act(shift (+ bias * scale) + residual) + post_add"""
    n, K, C = 50, 27, 36
    t = _operands(n, K, C, 48, seed=3, pairs=False, res=True, post=True, bias=bias)
    assert t["y"] is None
    got = _launch(None, t["slot"], C, 48, t["bias"], t["gamma"], t["beta"], t["mean"], t["var"], EPS, t["res"], t["post"], act)
    ref, M = _reference(None, t["slot"], C, t["bias"], t["gamma"], t["beta"], t["mean"], t["var"], EPS, t["res"], t["post"], act)
    assert bool(((got.double() - ref).abs() <= 64 * U * M).all())


# ---- convolution -> BatchNorm sites: the hand-over against the composition -------------------------------------------------------------
def _randomise(bn_module, seed):
    gen = torch.Generator().manual_seed(seed)
    bn = bn_module.bn
    with torch.no_grad():  # BatchNorm that is no identity fold (as tools/sa_module_bench.py)
        if bn.weight is not None:
            bn.weight.copy_(torch.randn(bn.weight.shape, generator=gen))
            bn.bias.copy_(torch.randn(bn.bias.shape, generator=gen) * 0.5)
        if bn.running_mean is not None:
            bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=gen) * 0.5)
            bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=gen) + 0.5)
    return bn_module


def _input(npoints, cin, seed, stride2=False):
    """a sparse tensor of `cin` random channels on a random cloud (at tensor stride 2: the sites of a strided layer)"""
    from vdetr_amd import minkowski as ME
    g = torch.Generator().manual_seed(seed)
    coords = torch.cat((torch.randint(0, 2, (npoints, 1), generator=g), torch.randint(-9, 9, (npoints, 3), generator=g)), 1).int()
    x = ME.SparseTensor(torch.randn(npoints, cin, generator=g).to(DEV), coordinates=coords.to(DEV))
    if stride2:
        with torch.no_grad():
            x = ME.MinkowskiConvolution(cin, cin, kernel_size=3, stride=2, dimension=3).to(DEV)(x)
        x = x._like(torch.randn(x.keys.shape[0], cin, generator=g).to(DEV))
    return x


_SITES = {  # name -> (convolution class, kernel size, stride, act, residual, input at stride 2)
    "3x3x3 + residual": ("MinkowskiConvolution", 3, 1, "relu", True, False),
    "3x3x3 stride 2": ("MinkowskiConvolution", 3, 2, "relu", False, False),
    "1x1x1 stride 2 (downsample)": ("MinkowskiConvolution", 1, 2, None, False, False),
    "generative transposed k2": ("MinkowskiGenerativeConvolutionTranspose", 2, 2, "elu", False, True),
}


def _make_site(name, cin, cout, npoints, bias=False, **bn_args):
    from vdetr_amd import minkowski as ME
    cls, ks, stride, act, with_res, stride2 = _SITES[name]
    torch.manual_seed(len(name) + cin + npoints)
    conv = getattr(ME, cls)(cin, cout, kernel_size=ks, stride=stride, bias=bias, dimension=3).to(DEV)
    if bias:
        with torch.no_grad():
            conv.bias.normal_()
    bn = _randomise(ME.MinkowskiBatchNorm(cout, **bn_args), seed=cout).to(DEV)
    x = _input(npoints, cin, seed=npoints + cin, stride2=stride2)
    res = x._like(torch.randn(x.keys.shape[0], cout, device=DEV)) if with_res else None
    return conv, bn, x, act, res


def _run_site(conv, bn, x, act, res, fused, monkeypatch):
    from vdetr_amd import minkowski as ME
    monkeypatch.setattr(ME, "INFER_FUSED", fused)
    ME.clear_last_paths()
    out = bn(conv(x), act=act, residual=res)
    return out, list(ME.LAST_PATHS)


def _site_magnitude(conv, bn, x, out, res):
    """M of the kernel test for a module site: from the layer's own pair products and BatchNorm tensors"""
    from vdetr_amd import sparse_ops as S
    _, _, plan = x.coordinate_manager.kernel_map(x.keys, out.keys, x.tensor_stride, out.tensor_stride, conv.kernel_size, conv.transposed)
    w = conv.kernel if conv.kernel.dim() == 3 else conv.kernel[None]
    y = S.pair_products(x.F, w, plan)
    b = bn.bn
    _, M = _reference(y, plan.slot, conv.out_channels, conv.bias, b.weight, b.bias, b.running_mean, b.running_var, b.eps,
                      None if res is None else res.F, None, 0)
    return M


@pytest.mark.parametrize("npoints", [700, 5])
@pytest.mark.parametrize("cin,cout", [(16, 32), (20, 36)])
@pytest.mark.parametrize("name", list(_SITES))
def test_fused_site_equals_composition(name, cin, cout, npoints, monkeypatch):
    """eval + no_grad, INFER_FUSED True against False: |a - b| <= 8 * 2^-24 * M (the two forms differ at most by where the compiler
    contracts a multiply-add; the build contracts nowhere, so they are expected to be the same bits)"""
    conv, bn, x, act, res = _make_site(name, cin, cout, npoints)
    conv.eval(), bn.eval()
    with torch.no_grad():
        a, paths_a = _run_site(conv, bn, x, act, res, True, monkeypatch)
        b, paths_b = _run_site(conv, bn, x, act, res, False, monkeypatch)
        assert paths_a == ["fused"] and paths_b == ["composition"]
        assert torch.equal(a.keys, b.keys) and a.tensor_stride == b.tensor_stride and a.F.shape == b.F.shape == (a.keys.shape[0], cout)
        M = _site_magnitude(conv, bn, x, b, res)
    err = (a.F.double() - b.F.double()).abs()
    print(f"bit-equal {torch.equal(a.F, b.F)}, max err / (2^-24 M) = {float((err / (U * M)).max()) if err.numel() else 0:.2f} (bound 8)")
    assert bool((err <= 8 * U * M).all())
    assert a.applied_act == b.applied_act == act


# ---- the gate -------------------------------------------------------------------------------------------------------------------------
def _gate_case(kind):
    conv, bn, x, act, res = _make_site("3x3x3 + residual", 16, 32, 700, **({"track_running_stats": False} if kind == "no running statistics" else {}))
    if kind == "train mode":
        conv.train(), bn.train()
    else:
        conv.eval(), bn.eval()
    if kind == "SyncBatchNorm":
        bn = nn.SyncBatchNorm.convert_sync_batchnorm(bn).eval()
        assert type(bn.bn) is nn.SyncBatchNorm
    return conv, bn, x, act, res


@pytest.mark.parametrize("kind", ["train mode", "autograd on", "SyncBatchNorm", "no running statistics"])
def test_gate_keeps_the_composition(kind, monkeypatch):
    """outside the gate the switch changes nothing: the composition runs and gives the same bits as with INFER_FUSED = False"""
    outs = []
    for fused in (True, False):
        conv, bn, x, act, res = _gate_case(kind)                 # fresh modules: train mode moves the running statistics
        with torch.set_grad_enabled(kind in ("train mode", "autograd on")):
            out, paths = _run_site(conv, bn, x, act, res, fused, monkeypatch)
        assert paths == ["composition"], (kind, fused, paths)
        outs.append(out.F.detach())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("cout", [32, 36])
def test_bare_convolution_reads_as_before(bias, cout, monkeypatch):
    """a convolution that no BatchNorm follows: whatever reads .F of its output under inference gets the composition's values"""
    from vdetr_amd import minkowski as ME
    conv, _, x, _, _ = _make_site("3x3x3 stride 2", 20, cout, 700, bias=bias)
    conv.eval()
    with torch.no_grad():
        monkeypatch.setattr(ME, "INFER_FUSED", True)
        a = conv(x)
        assert a._pending is not None and a.device == x.device   # nothing summed yet
        s = a + a                                                # __add__ reads .F
        parts = a.decomposed()
        monkeypatch.setattr(ME, "INFER_FUSED", False)
        b = conv(x)
        assert b._pending is None
    assert torch.equal(a.F, b.F) and a.F.shape == (a.keys.shape[0], cout)
    assert torch.equal(s.F, b.F + b.F) and torch.equal(torch.cat([f for _, f in parts]), b.F)


# ---- backbone -------------------------------------------------------------------------------------------------------------------------
def _backbone():
    from vdetr_amd import minkowski as ME
    from vdetr_amd.mink_resnet import MinkResNet
    from vdetr_amd.model_vdetr import ModelVDETR
    torch.manual_seed(0)
    pts = torch.rand(3000, 3) * torch.tensor([2.0, 1.5, 0.8])
    data = [(pts / 0.01, pts), (pts[:1200] / 0.01 + 5, pts[:1200] * 0.5)]
    net = MinkResNet(18, 3, inplanes=16, num_stages=4, stem_bn=True)
    up = ME.fuse_activations(ModelVDETR._make_up_block(128, 64, True))   # lands on the sites of stage 3, as the default model's neck
    for i, m in enumerate(mod for part in (net, up) for mod in part.modules() if isinstance(mod, ME.MinkowskiBatchNorm)):
        _randomise(m, seed=i)
    return net.to(DEV).eval(), up.to(DEV).eval(), [(c.to(DEV), f.to(DEV)) for c, f in data]


def _run_backbone(net, up, data, fused, monkeypatch):
    from vdetr_amd import minkowski as ME
    monkeypatch.setattr(ME, "INFER_FUSED", fused)
    coords, feats = ME.batch_sparse_collate(data)
    with torch.no_grad():
        outs = net(ME.SparseTensor(feats, coordinates=coords))
        neck = ME.sequential_add(up, outs[3], outs[2]) if fused else outs[2] + up(outs[3])   # the latter: the composition's `stages[i] + x`
    return outs + [neck], list(ME.LAST_PATHS)


def test_backbone_fused_equals_composition(monkeypatch):
    from vdetr_amd import minkowski as ME
    net, up, data = _backbone()
    sites = sum(isinstance(m, ME.MinkowskiBatchNorm) for part in (net, up) for m in part.modules())
    state = {k: v.clone() for part in (net, up) for k, v in part.state_dict().items()}
    fused, paths = _run_backbone(net, up, data, True, monkeypatch)
    assert paths == ["fused"] * sites and sites == 21 + 2
    again, _ = _run_backbone(net, up, data, True, monkeypatch)
    plain, paths = _run_backbone(net, up, data, False, monkeypatch)
    assert paths == ["composition"] * sites
    worst = 0.0
    for a, a2, b in zip(fused, again, plain):
        assert torch.equal(a.keys, b.keys) and a.tensor_stride == b.tensor_stride
        assert torch.equal(a.F, a2.F)                            # two fused runs: the same bits
        scale = float(b.F.abs().max())
        err = float((a.F - b.F).abs().max())
        worst = max(worst, err / scale)
        assert err <= 1e-3 * scale
    print(f"backbone fused vs composition: max |diff| / max |composition| over the stage and neck outputs = {worst:.3e}")
    after = {k: v for part in (net, up) for k, v in part.state_dict().items()}
    assert all(torch.equal(state[k], after[k]) for k in state)   # running statistics, num_batches_tracked, parameters untouched


def test_fresh_parameters_are_read_at_every_call(monkeypatch):
    """there is no folded-parameter cache: after an optimizer step on the BatchNorm weights and after load_state_dict with other
    running statistics the next fused forward equals the composition on the new values"""
    conv, bn, x, act, res = _make_site("3x3x3 + residual", 16, 32, 700)
    conv.eval(), bn.eval()

    def check():
        with torch.no_grad():
            a, pa = _run_site(conv, bn, x, act, res, True, monkeypatch)
            b, pb = _run_site(conv, bn, x, act, res, False, monkeypatch)
            M = _site_magnitude(conv, bn, x, b, res)
        assert pa == ["fused"] and pb == ["composition"]
        assert bool(((a.F.double() - b.F.double()).abs() <= 8 * U * M).all())
        return b.F.clone()

    first = check()
    opt = torch.optim.SGD(bn.parameters(), lr=0.5)
    for p in bn.parameters():
        p.grad = torch.randn_like(p)
    opt.step()
    second = check()
    assert not torch.equal(first, second)
    other = copy.deepcopy(bn.state_dict())
    other["bn.running_mean"] = other["bn.running_mean"] + 1.0
    other["bn.running_var"] = other["bn.running_var"] * 3.0
    bn.load_state_dict(other)
    third = check()
    assert not torch.equal(second, third)


def test_whole_model_backbone(monkeypatch):
    """ModelVDETR.backbone_forward of the default minkowski model in eval under no_grad: every conv -> BatchNorm site fused, the
    prepared-geometry call the same bits, the result within the tensor contract of the INFER_FUSED = False run"""
    from vdetr_amd import minkowski as ME
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    from vdetr_amd.model_vdetr import build_vdetr, default_args
    torch.manual_seed(0)
    model = build_vdetr(default_args(nqueries=32, dec_nlayers=2, preenc_npoints=256), ScannetDatasetConfig(), "minkowski").to(DEV)
    sites = [m for m in model.modules() if isinstance(m, ME.MinkowskiBatchNorm)]
    assert len(sites) == 44                                      # 37 in MinkResNet34, 3 x 2 in the up blocks, 1 in the out block
    for i, m in enumerate(sites):
        _randomise(m, seed=100 + i)
    g = torch.Generator().manual_seed(1)
    clouds = []
    for b in range(2):  # points on two planes: a floor and a wall
        n = 6000 - 1500 * b
        u = torch.rand((n, 2), generator=g)
        floor = torch.stack((u[:, 0] * 4, u[:, 1] * 3, torch.zeros(n)), 1)
        wall = torch.stack((u[:, 0] * 4, torch.zeros(n), u[:, 1] * 2.5), 1)
        clouds.append(torch.cat((floor[: n // 2], wall[n // 2:])).to(DEV) + 1.0)
    inputs = {"point_clouds": clouds, "point_cloud_dims_min": torch.stack([c.min(0)[0] for c in clouds]),
              "point_cloud_dims_max": torch.stack([c.max(0)[0] for c in clouds])}
    geo = model.prepare_geometry(inputs)
    model.eval()
    with torch.no_grad():
        a = model.backbone_forward(inputs)
        assert ME.LAST_PATHS == ["fused"] * 44
        b = model.backbone_forward(dict(inputs, geometry=geo))
        assert ME.LAST_PATHS == ["fused"] * 44
        monkeypatch.setattr(ME, "INFER_FUSED", False)
        c = model.backbone_forward(inputs)
        assert ME.LAST_PATHS == ["composition"] * 44
    for (xa, fa), (xb, fb), (xc, fc) in zip(a, b, c):
        assert torch.equal(xa, xb) and torch.equal(fa, fb)
        assert torch.equal(xa, xc) and fa.shape == fc.shape
        assert float((fa - fc).abs().max()) <= 1e-3 * float(fc.abs().max())
