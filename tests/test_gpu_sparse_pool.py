"""Sparse pooling on the GPU (csrc/sparse_pool.hip through sparse_ops.sparse_pool and the Minkowski*Pooling modules) against the
float64 restatements of tests/sparse_modules_restatement.py.

Tolerances.  max: ``torch.equal`` on y, arg and dx (a float maximum is exact; dx adds the same floats in the same ascending-k
order as the float32 restatement).  sum / avg: |got - ref64| <= (K + 1) 2^-24 sum_k |x_k| (1 / |N|) per element, forward and
(with dy) backward: the sequential-sum bound plus one rounding for the scale; nothing is measured, so there is no margin."""
import numpy as np
import pytest
import torch

import sparse_modules_restatement as R
from oracle import sparse_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [("two", 4), ("two", 20), ("two", 64), ("forty", 512), ("one", 4)]
FORWARD = [(g, m) for g in R.GEOMETRIES if not g.startswith("tr-") for m in ("sum", "avg", "max")]
TRANSPOSED = [(g, m) for g in R.GEOMETRIES if g.startswith("tr-") for m in ("sum", "avg")]


def _run(cloud, geometry, C, mode):
    from vdetr_amd import sparse_ops as S
    ins, outs, nbr = R.pool_geometry(cloud, geometry)
    x, dy = R.pool_inputs(cloud, geometry, C)
    nbr_d = nbr.int().to(DEV)
    inv_d = O.inverse_map(nbr.int(), len(ins)).to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    y, inv_count, arg = S.sparse_pool(xd, nbr_d, inv_d, mode, return_aux=True)
    (dx,) = torch.autograd.grad(y, xd, dy.to(DEV))
    return ins, nbr, x, dy, y.detach().cpu(), dx.cpu(), inv_count, arg


@pytest.mark.parametrize("cloud,C", CASES)
@pytest.mark.parametrize("geometry,mode", FORWARD + TRANSPOSED)
def test_pool_forward_backward(cloud, C, geometry, mode):
    ins, nbr, x, dy, y, dx, inv_count, arg = _run(cloud, geometry, C, mode)
    K, nin = nbr.shape[0], len(ins)
    empty = (nbr >= 0).sum(0) == 0
    if geometry == "tr-cube3-s2" and cloud == "two":
        assert len(set((nbr >= 0).sum(0).tolist())) >= 2  # the contributor counts differ
    if mode == "max":
        ry, _, rarg = R.pool_forward(x, nbr, "max", dtype=R.F32)
        assert torch.equal(y, ry)
        assert torch.equal(arg.cpu().long(), rarg)
        assert torch.equal(dx, R.pool_backward(dy, nbr, nin, "max", arg=rarg, dtype=R.F32))
    else:
        ry, ric, _ = R.pool_forward(x, nbr, mode)
        assert bool(((y.double() - ry).abs() <= R.pool_bound_forward(x, nbr, ric)).all())
        if mode == "avg":
            cnt = (nbr >= 0).sum(0)
            assert torch.equal(inv_count.cpu(), torch.where(cnt > 0, 1.0 / cnt.clamp(min=1).float(), torch.zeros(len(cnt))))
        rdx = R.pool_backward(dy, nbr, nin, mode, ric)
        assert bool(((dx.double() - rdx).abs() <= R.pool_bound_backward(dy, nbr, nin, ric)).all())
    assert bool((y[empty] == 0).all()) and bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    # two runs agree bit for bit
    _, _, _, _, y2, dx2, _, arg2 = _run(cloud, geometry, C, mode)
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    assert arg is None or torch.equal(arg, arg2)


@pytest.mark.parametrize("mode", ["sum", "avg", "max"])
def test_empty_neighbourhoods_give_exact_zeros(mode):
    ins, nbr, x, dy, y, dx, inv_count, arg = _run("two", "custom-s1", 20, mode)
    empty = (nbr >= 0).sum(0) == 0
    assert int(empty.sum()) > 50
    assert bool((y[empty] == 0).all()) and not bool(torch.signbit(y[empty]).any())
    unread = torch.ones(len(ins), dtype=torch.bool)
    unread[nbr[nbr >= 0]] = False
    assert int(unread.sum()) > 0 and bool((dx[unread] == 0).all())
    if mode == "max":
        assert bool((arg.cpu()[empty] == -1).all())
    if mode == "avg":
        assert bool((inv_count.cpu()[empty] == 0).all())


def test_arguments_are_checked():
    from vdetr_amd import sparse_ops as S
    nbr = torch.zeros((8, 5), dtype=torch.int32, device=DEV)
    x = torch.zeros((5, 8), device=DEV)
    with pytest.raises(RuntimeError):
        S.sparse_pool(x.cpu(), nbr, None, "sum")
    with pytest.raises(RuntimeError):
        S.sparse_pool(x.double(), nbr, None, "sum")
    with pytest.raises(RuntimeError):
        S.sparse_pool(x.t(), nbr[:, :5], None, "sum")
    with pytest.raises(RuntimeError, match="C=6"):
        S.sparse_pool(torch.zeros((5, 6), device=DEV), nbr, None, "sum")
    with pytest.raises(ValueError):
        S.sparse_pool(x, nbr, None, "median")


def _tensor(cloud, C, seed=0):
    from vdetr_amd import minkowski as ME
    sites = R.fine_sites(cloud)
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(len(sites), C, generator=g)
    return sites, feats, ME.SparseTensor(feats.to(DEV), torch.from_numpy(sites).int().to(DEV))


@pytest.mark.parametrize("cls,ks,stride,dilation,cross", [("MinkowskiSumPooling", 2, 2, 1, False), ("MinkowskiAvgPooling", 3, 1, 1, False),
                                                          ("MinkowskiMaxPooling", 3, 2, 1, False), ("MinkowskiAvgPooling", 3, 1, 2, True)])
def test_pooling_modules_share_sites_and_maps_with_a_convolution(cls, ks, stride, dilation, cross):
    from vdetr_amd import minkowski as ME
    sites, feats, x = _tensor("two", 8)
    gen = ME.KernelGenerator(ks, stride, dilation, region_type=ME.RegionType.HYPER_CROSS if cross else ME.RegionType.HYPER_CUBE,
                             dimension=3)
    pool = getattr(ME, cls)(ks, stride=stride, dilation=dilation, kernel_generator=gen)
    conv = ME.MinkowskiConvolution(8, 8, ks, stride=stride, dilation=dilation, kernel_generator=gen, dimension=3).to(DEV)
    y = pool(x)
    nmaps = len(x.coordinate_manager.maps)
    z = conv(x)
    assert len(x.coordinate_manager.maps) == nmaps, "a pooling and a convolution of equal geometry share one map"
    assert y.keys is z.keys or torch.equal(y.keys, z.keys)
    assert y.tensor_stride == z.tensor_stride == stride and y.F.shape == (z.F.shape[0], 8)
    outs = R.strided_sites(sites, stride) if stride > 1 else sites
    assert np.array_equal(y.C.cpu().numpy(), outs)
    offsets = R.cross_offsets(ks) if cross else R.cube_offsets(ks)
    nbr = R.neighbour_table(sites, outs, R.scale_reach(offsets, dilation))
    ref, ric, _ = R.pool_forward(feats, nbr, pool.mode, dtype=R.F32 if pool.mode == "max" else R.F64)
    if pool.mode == "max":
        assert torch.equal(y.F.cpu(), ref)
    else:
        assert bool(((y.F.cpu().double() - ref).abs() <= R.pool_bound_forward(feats, nbr, ric)).all())
    with ME.geometry_only():
        g = pool(x)
    assert g.F.shape == y.F.shape and g.keys is y.keys


@pytest.mark.parametrize("ks", [2, 3])
def test_unpooling_of_a_pooling(ks):
    """MinkowskiAvgUnpooling(MinkowskiAvgPooling(x)) lands on x's sites; values within twice the stage bound: each stage's error
    is at most (K + 1) 2^-24 max|x| (an average does not exceed the largest magnitude), and the second stage averages the first's"""
    from vdetr_amd import minkowski as ME
    sites, feats, x = _tensor("two", 20, seed=1)
    down, up = ME.MinkowskiAvgPooling(ks, stride=2), ME.MinkowskiAvgUnpooling(ks, stride=2)
    mid = down(x)
    back = up(mid)
    assert back.tensor_stride == 1 and back.keys is x.keys and back.F.shape == feats.shape
    coarse = R.strided_sites(sites, 2)
    n1 = R.neighbour_table(sites, coarse, R.cube_offsets(ks))
    n2 = R.neighbour_table(coarse, sites, R.scale_reach(R.cube_offsets(ks), -1))
    m64, _, _ = R.pool_forward(feats, n1, "avg")
    r64, _, _ = R.pool_forward(m64, n2, "avg")
    K = ks ** 3
    assert float((back.F.cpu().double() - r64).abs().max()) <= 2 * (K + 1) * 2.0 ** -24 * float(feats.abs().max())
    # MinkowskiPoolingTranspose: the same map, without the count
    s64, _, _ = R.pool_forward(m64, n2, "sum")
    plain = ME.MinkowskiPoolingTranspose(ks, stride=2)(mid)
    assert plain.keys is x.keys
    assert bool(((plain.F.cpu().double() - s64).abs() <= R.pool_bound_forward(m64, n2) + (K + 1) * 2.0 ** -24 * (n2 >= 0).sum(0)[:, None]
                 * float(feats.abs().max())).all())
    # gradients flow through both modules
    xf = feats.to(DEV).requires_grad_(True)
    xs = ME.SparseTensor(xf, coordinate_manager=x.coordinate_manager, tensor_stride=1)
    up(down(xs)).F.sum().backward()
    ref = feats.double().requires_grad_(True)
    mid_ref = (R._gathered(ref, n1).sum(0) * R.pool_forward(feats, n1, "avg")[1][:, None])
    (R._gathered(mid_ref, n2).sum(0) * R.pool_forward(m64, n2, "avg")[1][:, None]).sum().backward()
    # (every contribution to this gradient is positive: the sums of magnitudes in the two stage bounds are the values themselves)
    assert bool(((xf.grad.cpu().double() - ref.grad).abs() <= 2 * (K + 1) * 2.0 ** -24 * ref.grad.abs()).all())
