"""The channelwise (depthwise) sparse convolution on the GPU (csrc/sparse_cwconv.hip through sparse_ops.channelwise_conv and
MinkowskiChannelwiseConvolution) against the restatements of tests/channelwise_restatement.py.

Tolerances (derived there, nothing measured, no margin; u = 2^-24).  y and dx: ``torch.equal`` with the float32 restatement that
follows the kernel's order (one fmaf per present term in ascending k, the bias last), and |got - ref64| <= (K + 2) u (sum_k |W x|
+ |b|) / (K + 1) u sum_k |W dy|.  dW[k][c]: (n_k + 1) u sum_u |x dy| with n_k the pairs of offset k, which holds for any order
of summation; db[c]: nout u sum_u |dy|."""
import functools

import numpy as np
import pytest
import torch

import channelwise_restatement as CW
import sparse_modules_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [("two", 4), ("two", 20), ("two", 64), ("forty", 512), ("one", 4)]
FORWARD = [g for g in R.GEOMETRIES if not g.startswith("tr-")]


def _launch(x, w, b, nbr, dy, needs=(True, True, True), inv="table"):
    """-> (y, dx, dW, db) on the host; a gradient that ``needs`` does not ask for (or a missing bias) is None"""
    from vdetr_amd import sparse_ops as S
    nin = x.shape[0]
    nbr_d = nbr.int().to(DEV)
    inv_d = R.inverse_table(nbr, nin).int().to(DEV) if inv == "table" else inv
    xd = x.to(DEV).requires_grad_(needs[0])
    wd = w.to(DEV).requires_grad_(needs[1])
    bd = b.to(DEV).requires_grad_(needs[2]) if b is not None else None
    y = S.channelwise_conv(xd, wd, nbr_d, inv_d, bd)
    wanted = [t for t in (xd, wd, bd) if t is not None and t.requires_grad]
    grads = list(torch.autograd.grad(y, wanted, dy.to(DEV)))
    out = [grads.pop(0).cpu() if t is not None and t.requires_grad else None for t in (xd, wd, bd)]
    return (y.detach().cpu(), *out)


def _check(x, w, b, nbr, dy, got):
    y, dx, dw, db = got
    nin = x.shape[0]
    assert y.shape == (nbr.shape[1], x.shape[1]) and dx.shape == x.shape and dw.shape == w.shape
    assert torch.equal(y, CW.forward32(x, w, nbr, b))
    assert torch.equal(dx, CW.grad_input32(dy, w, nbr, nin))
    assert bool(((y.double() - CW.forward(x, w, nbr, b)).abs() <= CW.bound_forward(x, w, nbr, b)).all())
    assert bool(((dx.double() - CW.grad_input(dy, w, nbr, nin)).abs() <= CW.bound_input(dy, w, nbr, nin)).all())
    assert bool(((dw.double() - CW.grad_weight(x, dy, nbr)).abs() <= CW.bound_weight(x, dy, nbr)).all())
    if b is not None:
        assert db.shape == b.shape
        assert bool(((db.double() - CW.grad_bias(dy)).abs() <= CW.bound_bias(dy)).all())
    for t in got:
        assert t is None or bool(torch.isfinite(t).all())


def _same(a, b):
    return all((s is None and t is None) or torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("cloud,C", CASES)
@pytest.mark.parametrize("geometry", FORWARD)
def test_forward_and_gradients(geometry, cloud, C, bias):
    ins, outs, nbr = R.pool_geometry(cloud, geometry)
    x, dy = R.pool_inputs(cloud, geometry, C)
    w, b = CW.weights(nbr.shape[0], C, bias=bias)
    got = _launch(x, w, b, nbr, dy)
    _check(x, w, b, nbr, dy, got)
    assert _same(got, _launch(x, w, b, nbr, dy)), "two runs agree bit for bit"


@functools.lru_cache(maxsize=None)
def _cube_case(ks, C):
    sites = R.fine_sites("two")
    nbr = R.neighbour_table(sites, sites, R.cube_offsets(ks))
    g = torch.Generator().manual_seed(ks * 100 + C)
    return nbr, torch.randn(len(sites), C, generator=g), torch.randn(len(sites), C, generator=g)


@pytest.mark.parametrize("ks,C", [(5, 8), (1, 8)])
def test_largest_and_smallest_kernel(ks, C):
    nbr, x, dy = _cube_case(ks, C)
    assert nbr.shape[0] == ks ** 3
    w, b = CW.weights(ks ** 3, C)
    _check(x, w, b, nbr, dy, _launch(x, w, b, nbr, dy))


@pytest.mark.parametrize("C", [20, 68])
@pytest.mark.parametrize("edge", ["below", "exact", "ragged"])
def test_weight_gradient_chunk_edges(edge, C):
    """nout smaller than a chunk of the weight-gradient sweep, exactly one chunk, and more than two chunks with a ragged last one
    (C = 20: a slab narrower than its threads; C = 68: a second, nearly empty channel slab)"""
    from vdetr_amd import sparse_ops as S
    rows = S.cwconv_chunk_rows(1)
    assert rows > 0
    nout = {"below": rows // 2 + 1, "exact": rows, "ragged": 2 * rows + rows // 2 + 3}[edge]
    sites = R.cloud(6 * rows, 7, extent=8)[:nout]
    assert len(sites) == nout and S.cwconv_chunk_rows(nout) == rows
    if edge == "ragged":
        assert nout > 2 * rows and nout % rows != 0
    nbr = R.neighbour_table(sites, sites, R.cube_offsets(3))
    g = torch.Generator().manual_seed(nout + C)
    x, dy = torch.randn(nout, C, generator=g), torch.randn(nout, C, generator=g)
    w, b = CW.weights(27, C)
    got = _launch(x, w, b, nbr, dy)
    _check(x, w, b, nbr, dy, got)
    assert _same(got, _launch(x, w, b, nbr, dy))


def test_weight_gradient_chunks_longer_than_the_minimum():
    """above 512 chunks of the shortest length the chunks grow instead: rows per chunk above the minimum, several rows per lane"""
    from vdetr_amd import sparse_ops as S
    sites = R.cloud(44000, 13, extent=20)
    nout = len(sites)
    rows = S.cwconv_chunk_rows(nout)
    assert rows > S.cwconv_chunk_rows(1) and nout % rows != 0 and -(-nout // rows) <= 512
    nbr = R.neighbour_table(sites, sites, R.cross_offsets(3))
    g = torch.Generator().manual_seed(nout)
    x, dy = torch.randn(nout, 4, generator=g), torch.randn(nout, 4, generator=g)
    w, b = CW.weights(7, 4)
    _check(x, w, b, nbr, dy, _launch(x, w, b, nbr, dy))


def test_empty_neighbourhoods_give_exact_values():
    sites = R.fine_sites("two")
    nbr = R.neighbour_table(sites, sites, [(1, 0, 0), (0, 0, 40), (-1, -1, 0)])  # no centre; nothing lies 40 cells away
    assert int((nbr[1] >= 0).sum()) == 0 and int((nbr[0] >= 0).sum()) > 0
    empty = (nbr >= 0).sum(0) == 0
    assert int(empty.sum()) > 50
    unread = torch.ones(len(sites), dtype=torch.bool)
    unread[nbr[nbr >= 0]] = False
    assert int(unread.sum()) > 0
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(len(sites), 20, generator=g), torch.randn(len(sites), 20, generator=g)
    w, b = CW.weights(3, 20)
    y, dx, dw, db = _launch(x, w, b, nbr, dy)
    _check(x, w, b, nbr, dy, (y, dx, dw, db))
    assert torch.equal(y[empty], b[None].expand(int(empty.sum()), -1))
    assert bool((dx[unread] == 0).all()) and bool((dw[1] == 0).all()) and bool((dw[0] != 0).any())
    y0 = _launch(x, w, None, nbr, dy)[0]
    assert bool((y0[empty] == 0).all()) and not bool(torch.signbit(y0[empty]).any())


def test_backward_launches_only_what_is_asked_for():
    ins, outs, nbr = R.pool_geometry("two", "cube3-s2")
    x, dy = R.pool_inputs("two", "cube3-s2", 20)
    w, b = CW.weights(nbr.shape[0], 20)
    full = _launch(x, w, b, nbr, dy)
    for needs in ((True, False, False), (False, True, False), (False, False, True), (True, True, False)):
        got = _launch(x, w, b, nbr, dy, needs=needs)
        assert torch.equal(got[0], full[0])
        for have, ref, asked in zip(got[1:], full[1:], needs):
            assert (have is None) == (not asked)
            assert have is None or torch.equal(have, ref), needs
    # the inverse map is built inside when none is passed and feats wants a gradient
    assert _same(_launch(x, w, b, nbr, dy, inv=None), full)


def test_tables_without_rows():
    from vdetr_amd import sparse_ops as S
    K, C, n = 8, 12, 37
    w, b = CW.weights(K, C)
    g = torch.Generator().manual_seed(9)
    # no input row: every neighbourhood is empty
    nbr = torch.full((K, n), -1, dtype=torch.int64)
    dy = torch.randn(n, C, generator=g)
    y, dx, dw, db = _launch(torch.zeros(0, C), w, b, nbr, dy)
    assert torch.equal(y, b[None].expand(n, -1)) and dx.shape == (0, C) and bool((dw == 0).all()) and dw.shape == (K, C)
    assert bool(((db.double() - CW.grad_bias(dy)).abs() <= CW.bound_bias(dy)).all())
    # no output row
    x = torch.randn(n, C, generator=g)
    y, dx, dw, db = _launch(x, w, b, torch.zeros((K, 0), dtype=torch.int64), torch.zeros(0, C))
    assert y.shape == (0, C) and dx.shape == (n, C) and dw.shape == (K, C) and db.shape == (C,)
    assert bool((dx == 0).all()) and bool((dw == 0).all()) and bool((db == 0).all())
    torch.cuda.synchronize()
    assert S.cwconv_chunk_rows(0) > 0


def test_arguments_are_checked():
    from vdetr_amd import sparse_ops as S
    nbr = torch.zeros((8, 5), dtype=torch.int32, device=DEV)
    x = torch.zeros((5, 8), device=DEV)
    w = torch.zeros((8, 8), device=DEV)
    assert S.channelwise_conv(x, w, nbr).shape == (5, 8)
    with pytest.raises(RuntimeError, match="CPU"):
        S.channelwise_conv(x.cpu(), w, nbr)
    with pytest.raises(RuntimeError, match="weight"):
        S.channelwise_conv(x, w.cpu(), nbr)
    with pytest.raises(RuntimeError, match="feats"):
        S.channelwise_conv(x.double(), w, nbr)
    with pytest.raises(RuntimeError, match="weight"):
        S.channelwise_conv(x, w.double(), nbr)
    with pytest.raises(RuntimeError, match="feats"):
        S.channelwise_conv(torch.zeros((8, 5), device=DEV).t(), w, nbr)
    with pytest.raises(RuntimeError, match="C=6"):
        S.channelwise_conv(torch.zeros((5, 6), device=DEV), torch.zeros((8, 6), device=DEV), nbr)
    with pytest.raises(RuntimeError, match="nbr"):
        S.channelwise_conv(x, w, nbr.long())
    with pytest.raises(RuntimeError, match=r"weight is \(7, 8\)"):
        S.channelwise_conv(x, w[:7], nbr)
    with pytest.raises(RuntimeError, match=r"weight is \(8, 8, 8\)"):
        S.channelwise_conv(x, torch.zeros((8, 8, 8), device=DEV), nbr)
    with pytest.raises(RuntimeError, match=r"inv is \(8, 4\)"):
        S.channelwise_conv(x, w, nbr, torch.zeros((8, 4), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match=r"bias is \(4,\)"):
        S.channelwise_conv(x, w, nbr, None, torch.zeros(4, device=DEV))
    with pytest.raises(RuntimeError, match=r"bias is \(8, 1\)"):
        S.channelwise_conv(x, w, nbr, None, torch.zeros((8, 1), device=DEV))


# ---- the module --------------------------------------------------------------------------------------------------------------------
def _tensor(cloud, C, seed=0):
    from vdetr_amd import minkowski as ME
    sites = R.fine_sites(cloud)
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(len(sites), C, generator=g)
    return sites, feats, ME.SparseTensor(feats.to(DEV), torch.from_numpy(sites).int().to(DEV))


@pytest.mark.parametrize("ks,stride,dilation,cross,bias", [(3, 1, 1, False, True), (2, 2, 1, False, False), (3, 2, 1, False, True),
                                                           (3, 1, 2, True, True)])
def test_module_against_the_restatement_and_the_dense_convolution(ks, stride, dilation, cross, bias, monkeypatch):
    from vdetr_amd import minkowski as ME
    from vdetr_amd import sparse_ops as S
    C = 8
    sites, feats, x = _tensor("two", C)
    cm = x.coordinate_manager
    gen = ME.KernelGenerator(ks, stride, dilation, region_type=ME.RegionType.HYPER_CROSS if cross else ME.RegionType.HYPER_CUBE,
                             dimension=3)
    torch.manual_seed(ks + stride)
    cw = ME.MinkowskiChannelwiseConvolution(C, ks, stride=stride, dilation=dilation, bias=bias, kernel_generator=gen).to(DEV)
    K = gen.kernel_volume
    state = cw.state_dict()
    assert set(state) == ({"kernel", "bias"} if bias else {"kernel"}) and state["kernel"].shape == (K, C)
    assert float(cw.kernel.detach().abs().max()) <= float(np.float32(1.0 / np.sqrt(C * K)))  # uniform +-1 / sqrt(in_channels * volume)
    if bias:
        assert state["bias"].shape == (1, C) and bool((cw.bias == 0).all())
        with torch.no_grad():
            cw.bias.normal_()
    seen = {}
    for name in ("channelwise_conv", "sparse_conv"):
        def spy(*args, _inner=getattr(S, name), _name=name, **kw):
            seen[_name] = args[2].data_ptr()
            return _inner(*args, **kw)
        monkeypatch.setattr(S, name, spy)
    y = cw(x)
    nmaps = len(cm.maps)
    conv = ME.MinkowskiConvolution(C, C, ks, stride=stride, dilation=dilation, bias=bias, kernel_generator=gen, dimension=3).to(DEV)
    with torch.no_grad():
        conv.kernel.copy_(torch.diag_embed(cw.kernel))
        if bias:
            conv.bias.copy_(cw.bias)
    z = conv(x)
    assert len(cm.maps) == nmaps and seen["channelwise_conv"] == seen["sparse_conv"], "one cached map for both layers"
    assert y.tensor_stride == z.tensor_stride == stride and (y.keys is z.keys)
    if stride == 2:
        assert y.keys is cm.keys[2]
    outs = R.strided_sites(sites, stride) if stride > 1 else sites
    assert np.array_equal(y.C.cpu().numpy(), outs)
    nbr = R.neighbour_table(sites, outs, R.scale_reach(R.cross_offsets(ks) if cross else R.cube_offsets(ks), dilation))
    w = cw.kernel.detach().cpu()
    b = cw.bias.detach().cpu().reshape(-1) if bias else None
    assert torch.equal(y.F.detach().cpu(), CW.forward32(feats, w, nbr, b))
    # the dense path on the diagonal kernel (exact fp32 products at this width): the two results differ by at most the sum of the
    # two forward bounds
    bound = CW.bound_forward(feats, w, nbr, b) + CW.bound_forward_dense(feats, w, nbr, b)
    assert bool(((y.F.detach().cpu().double() - z.F.detach().cpu().double()).abs() <= bound).all())
    # gradients reach the parameters through the module
    dy = torch.randn(y.F.shape, generator=torch.Generator().manual_seed(1))
    fd = feats.to(DEV).requires_grad_(True)
    out = cw(x._like(fd))
    (out.F * dy.to(DEV)).sum().backward()
    got = (out.F.detach().cpu(), fd.grad.cpu(), cw.kernel.grad.cpu(), cw.bias.grad.cpu().reshape(-1) if bias else None)
    _check(feats, w, b, nbr, dy, got)


def test_module_geometry_pass_origin_tensors_and_strided_features():
    from vdetr_amd import minkowski as ME
    sites, feats, x = _tensor("two", 16, seed=2)
    cm = x.coordinate_manager
    cw = ME.MinkowskiChannelwiseConvolution(16, kernel_size=3, stride=2, bias=True, dimension=3).to(DEV)
    with ME.geometry_only():
        g = cw(x)
    nmaps, ninv = len(cm.maps), len(cm.__dict__.get("_pool_inverse", {}))
    y = cw(x)
    assert len(cm.maps) == nmaps and len(cm.__dict__.get("_pool_inverse", {})) == ninv, "the geometry pass built everything"
    assert g.F.shape == y.F.shape and g.keys is y.keys and g.tensor_stride == y.tensor_stride == 2
    # a feature table that is a strided view
    wide = torch.randn(len(sites), 32, generator=torch.Generator().manual_seed(4)).to(DEV)
    wide[:, ::2] = x.F
    view = wide[:, ::2]
    assert not view.is_contiguous()
    assert torch.equal(cw(x._like(view)).F, y.F)
    # one row per scene has no lattice
    with pytest.raises(ValueError, match="origin"):
        cw(ME.MinkowskiGlobalSumPooling()(x))
    with pytest.raises(ValueError):
        ME.MinkowskiChannelwiseConvolution(16, kernel_size=3, stride=2, dilation=2)
    with pytest.raises(NotImplementedError):
        ME.MinkowskiChannelwiseConvolution(16, kernel_size=3, stride=(2, 1, 2))
