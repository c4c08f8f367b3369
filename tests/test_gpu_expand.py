"""Caller-chosen output sites on the GPU: the region-keys launch and ``sparse_ops.region_keys`` / ``target_keys``
against tests/expand_restatement.py (every key comparison bit-equal), and ``expand_coordinates=True`` / ``forward(x, coordinates)``
of the convolution, channelwise and pooling layers against the float64 oracle and the restatements.

Tolerances.  Convolutions: the bound of tests/test_gpu_sparse_modules.py for these kernels, 1e-4 max|ref| + 1e-6, against
oracle.sparse_oracle.sparse_conv in float64 on the oracle's dictionary-built map.  Poolings: the derived bounds of
sparse_modules_restatement (max: ``torch.equal``).  Channelwise forward, the hand-driven ``sparse_conv`` and the generative
transposed convolution: ``torch.equal``."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import channelwise_restatement as CW
import expand_restatement as E
import sparse_modules_restatement as R
from oracle import sparse_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = torch.int32


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _pick(n, seed, scenes=(0, 1), extent=10, ts=1):
    """exactly n sites of tensor stride ts, spread over ``scenes``, negative coordinates among them"""
    if n == 0:
        return np.zeros((0, 4), dtype=np.int64)
    rng = np.random.default_rng(seed)
    m = 4 * n + 8
    c = np.unique(np.concatenate((rng.choice(scenes, (m, 1)), rng.integers(-extent, extent, (m, 3)) * ts), 1), axis=0)
    assert len(c) >= n
    return R.sort_sites(c[rng.permutation(len(c))[:n]])


def _keys(sites):
    return torch.from_numpy(O.pack_keys_np(np.asarray(sites, dtype=np.int64).reshape(-1, 4)))


def _step(region, out_ts):
    """the int32 offsets the launch adds: scaled and signed by the host"""
    offsets, transposed, _ = E.REGIONS[region]
    ts, out_ts = E.strides(region, out_ts)
    return torch.tensor(offsets, dtype=I32).reshape(-1, 3) * (out_ts if transposed else -ts)


def _check_region_keys(sites, region, out_ts):
    from vdetr_amd import sparse_ops as S
    offsets, transposed, _ = E.REGIONS[region]
    ts, out_ts = E.strides(region, out_ts)
    got = S.region_keys(_keys(sites).to(DEV), _step(region, out_ts).to(DEV))
    ref = O.pack_keys_np(E.expanded_sites(sites, offsets, ts, out_ts, transposed))
    assert got.dtype == torch.int64 and got.dim() == 1 and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), ref)
    return got


def _tensor(sites, C, seed=0, grad=False):
    """(features on the host, the SparseTensor on ``sites`` (sorted, unique), its leaf feature table on the device)"""
    from vdetr_amd import minkowski as ME
    f = torch.randn(len(sites), C, generator=torch.Generator().manual_seed(seed))
    base = ME.SparseTensor(f.to(DEV), torch.from_numpy(sites).int().to(DEV))
    assert np.array_equal(base.C.cpu().numpy(), sites)
    leaf = f.to(DEV).requires_grad_(grad)
    return f, base._like(leaf), leaf


def _oracle(f, w, bias, nbr, g):
    """float64: (out, dfeats, dkernel) of out = sparse_conv(f, w, nbr) (+ bias) under the cotangent g"""
    fr, wr = f.double().requires_grad_(True), w.detach().cpu().double().requires_grad_(True)
    ref = O.sparse_conv(fr, wr if wr.dim() == 3 else wr[None], nbr)
    if bias is not None:
        ref = ref + bias.detach().cpu().double().reshape(1, -1)
    (ref * g.double()).sum().backward()
    return ref.detach(), fr.grad, wr.grad


def _inside(got, ref, name):
    """the bound of tests/test_gpu_sparse_modules.py"""
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got.detach().cpu().double() - ref).abs().max()) if ref.numel() else 0.0
    print(f"{name}: max error {err:.3e}, bound {1e-4 * scale + 1e-6:.3e}")
    assert got.shape == ref.shape and err <= 1e-4 * scale + 1e-6, name


# ---- keys --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["0", "1", "T-1", "T", "T+1", "2T+1"])
@pytest.mark.parametrize("region", list(E.REGIONS))
def test_region_keys_at_the_tile_edges(region, size):
    from vdetr_amd import sparse_ops as S
    T = S.voxel_tile()
    n = {"0": 0, "1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}[size]
    ts, _ = E.strides(region, 1)
    sites = _pick(n, 7 + n, ts=ts)
    assert len(sites) == n and (n < 8 or int(sites[:, 1:].min()) < 0)
    got = _check_region_keys(sites, region, 1)
    assert got.shape[0] >= n and (n > 0 or got.shape[0] == 0)


@pytest.mark.parametrize("out_ts,scenes", [(2, (0, 2)), (4, (0, 1, 2))])
@pytest.mark.parametrize("region", list(E.REGIONS))
def test_region_keys_at_tensor_strides_and_scenes(region, out_ts, scenes):
    """tensor strides 2 and 4; three scenes, and three of which the middle one is empty"""
    ts, _ = E.strides(region, out_ts)
    sites = _pick(300, out_ts, scenes=scenes, extent=5, ts=ts)
    assert set(sites[:, 0]) == set(scenes) and int(sites[:, 1:].min()) < 0
    got = _check_region_keys(sites, region, out_ts)
    assert set((got >> 48).cpu().tolist()) == set(scenes)


def test_runs_of_equal_candidates_cross_the_tiles_of_the_sites_pass():
    from vdetr_amd import sparse_ops as S
    T = S.voxel_tile()
    # a line of sites along x under (-1, 0, +1): every interior site is reached three times, run j lies at 3 j - 1 .. 3 j + 1
    n = T // 2 + 40
    line = np.stack((np.zeros(n), np.arange(n) - 5, np.full(n, 3), np.full(n, -2)), 1).astype(np.int64)
    offsets = [(-1, 0, 0), (0, 0, 0), (1, 0, 0)]
    cand = np.sort(O.pack_keys_np(E.candidates(line, offsets, 1, 1, False)))
    assert cand[T - 1] == cand[T] and len(cand) > T, "a run crosses the first tile boundary"
    got = S.region_keys(_keys(line).to(DEV), -torch.tensor(offsets, dtype=I32).to(DEV))
    assert np.array_equal(got.cpu().numpy(), np.unique(cand)) and got.shape[0] == n + 2
    # a run longer than a tile: T + 5 equal offsets of a custom region over three sites
    few = np.array([[0, 1, 2, 3], [0, 4, -4, 0], [1, 0, 0, 0]], dtype=np.int64)
    same = torch.tensor([(2, 0, -1)] * (T + 5), dtype=I32)
    got = S.region_keys(_keys(few).to(DEV), same.to(DEV))
    assert np.array_equal(got.cpu().numpy(), O.pack_keys_np(few + np.array([0, 2, 0, -1])))


def _raw_candidates(keys, step):
    from vdetr_amd import _lib as L
    N, K = keys.shape[0], step.shape[0]
    cand = torch.full((K * N,), -7, dtype=torch.int64, device=DEV)
    d = L.SpRegionKeysDesc()
    d.N, d.K, d.keys, d.offsets, d.cand = N, K, keys.data_ptr(), step.data_ptr(), cand.data_ptr()
    L.check(L.lib().vdetr_sp_region_keys_i64(ctypes.byref(d), L.stream_ptr()), "sp_region_keys")
    return cand.cpu().numpy().reshape(K, N)


def test_keys_at_the_range_edge():
    from vdetr_amd import sparse_ops as S
    legal = R.sort_sites(np.array([[0, 32766, 0, 0], [0, -32766, 5, 5], [2, 3, 32766, -32766], [2, 0, 0, 0], [2, -32766, -32766, 32766]]))
    got = _check_region_keys(legal, "cube3", 1)  # a reach of 1 from +-32766 stays inside
    assert set((got >> 48).cpu().tolist()) == {0, 2}
    step = _step("cube3", 1).to(DEV)
    for bad in ([0, 32767, 0, 0], [2, 0, -32768, 0], [0, 0, 0, 32767], [2, -32768, 1, 1]):
        sites = R.sort_sites(np.concatenate((legal, [bad])))
        with pytest.raises(ValueError, match=S.RANGE_MESSAGE):
            S.region_keys(_keys(sites).to(DEV), step)
        # the launch itself: a candidate whose field leaves the range is -1, every other one has only its own fields moved
        c = E.candidates(sites, E.REGIONS["cube3"][0], 1, 1, False).reshape(len(sites), 27, 4)
        inside = ((c[:, :, 1:] >= -32768) & (c[:, :, 1:] <= 32767)).all(2)
        want = np.where(inside, O.pack_keys_np(c.reshape(-1, 4)).reshape(len(sites), 27), -1).T  # [K, N]
        raw = _raw_candidates(_keys(sites).to(DEV), step)
        assert 0 < int((~inside).sum()) < inside.size and np.array_equal(raw, want)
        kept = raw[raw >= 0]
        assert set((kept >> 48).tolist()) == {0, 2} and np.array_equal(kept >> 48, np.broadcast_to(sites[:, 0], raw.shape)[raw >= 0])
    # a site AT the edge whose only child moves inwards is legal: (1, 0, 0) not transposed reaches x - 1
    edge = R.sort_sites(np.array([[0, 32767, -32768, 32767], [1, 32767, 0, 0]]))
    _check_region_keys(edge, "custom-x", 1)
    with pytest.raises(ValueError, match=S.RANGE_MESSAGE):
        S.region_keys(_keys(edge).to(DEV), -_step("custom-x", 1).to(DEV))
    with pytest.raises(RuntimeError, match="CPU"):
        S.region_keys(_keys(edge), _step("custom-x", 1))
    with pytest.raises(RuntimeError, match="CPU"):
        S.target_keys(torch.zeros((3, 4), dtype=I32))


def test_target_keys():
    from vdetr_amd import sparse_ops as S
    rng = np.random.default_rng(4)
    coords = np.concatenate((rng.integers(0, 3, (700, 1)), rng.integers(-6, 6, (700, 3))), 1)
    coords = np.concatenate((coords, coords[:90]))[rng.permutation(790)]
    sites, inverse = E.target_sites(coords)
    for dtype in (I32, torch.int64):
        keys, inv = S.target_keys(torch.from_numpy(coords).to(dtype).to(DEV))
        assert inv.dtype == I32 and np.array_equal(keys.cpu().numpy(), O.pack_keys_np(sites)) and np.array_equal(inv.cpu().numpy(), inverse)
    with pytest.raises(ValueError, match=S.RANGE_MESSAGE):
        S.target_keys(torch.tensor([[0, 1, 2, 3], [0, 40000, 0, 0]], dtype=I32, device=DEV))


# ---- layers on expanded sites --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cloud():
    return R.cloud(600, 21, extent=6)


@pytest.mark.parametrize("cin,cout", [(16, 24), (64, 128)])
@pytest.mark.parametrize("ks", [3, 2])
def test_convolution_on_expanded_sites(ks, cin, cout):
    from vdetr_amd import minkowski as ME
    from vdetr_amd import sparse_ops as S
    assert S._MODE == "pairs" and not S._IM2COL
    sites, offsets = _cloud(), R.cube_offsets(ks)
    torch.manual_seed(cin + ks)
    conv = ME.MinkowskiConvolution(cin, cout, kernel_size=ks, expand_coordinates=True, dimension=3).to(DEV)
    f, x, leaf = _tensor(sites, cin, grad=True)
    cm = x.coordinate_manager
    out = conv(x)
    ref_sites = E.expanded_sites(sites, offsets, 1, 1, False)
    ref_keys = _keys(ref_sites)
    assert torch.equal(out.keys.cpu(), ref_keys) and out.tensor_stride == 1 and out.inverse_mapping is None
    assert cm.keys[1] is x.keys and out.keys is not x.keys and list(cm.keys) == [1], "a new, non-canonical key set"
    assert out.F.shape == (len(ref_sites), cout) and len(ref_sites) > len(sites)
    g = torch.randn(len(ref_sites), cout, generator=torch.Generator().manual_seed(2))
    (out.F * g.to(DEV)).sum().backward()
    nbr = O.kernel_map(_keys(sites), ref_keys, torch.tensor(offsets, dtype=I32))
    assert bool((nbr >= 0).any(0).all()), "no row of the map is empty: the definition"
    ry, rdf, rdw = _oracle(f, conv.kernel, None, nbr, g)
    _inside(out.F, ry, "out")
    _inside(leaf.grad, rdf, "dfeats")
    _inside(conv.kernel.grad, rdw, "dkernel")
    # by hand on a map built from the restatement's keys: the same bits
    nbr_d = S.kernel_map(x.keys, ref_keys.to(DEV), torch.tensor(offsets, dtype=I32).to(DEV))
    assert torch.equal(nbr_d.cpu(), nbr)
    hand = S.sparse_conv(leaf.detach(), conv.kernel.detach(), nbr_d, None, S.PairPlan(nbr_d, len(sites)))
    assert torch.equal(hand, out.F.detach())


@functools.lru_cache(maxsize=None)
def _coarse(C=16):
    """a tensor of stride 2 under a strided convolution of the cloud: (coarse sites, its features on the host, the tensor)"""
    from vdetr_amd import minkowski as ME
    sites = _cloud()
    _, x, _ = _tensor(sites, 8, seed=3)
    torch.manual_seed(1)
    with torch.no_grad():
        y = ME.MinkowskiConvolution(8, C, kernel_size=2, stride=2, dimension=3).to(DEV)(x)
    coarse = R.strided_sites(sites, 2)
    assert np.array_equal(y.C.cpu().numpy(), coarse) and y.tensor_stride == 2
    return coarse, y.F.detach().cpu(), y, x


@pytest.mark.parametrize("ks", [2, 3])
def test_transposed_expansion_is_the_generative_convolution(ks):
    from vdetr_amd import minkowski as ME
    coarse, yf, y, _ = _coarse()
    torch.manual_seed(ks)
    a = ME.MinkowskiConvolutionTranspose(16, 24, kernel_size=ks, stride=2, bias=True, expand_coordinates=True, dimension=3).to(DEV)
    b = ME.MinkowskiGenerativeConvolutionTranspose(16, 24, kernel_size=ks, stride=2, bias=True, dimension=3).to(DEV)
    with torch.no_grad():
        a.bias.normal_()
        b.kernel.copy_(a.kernel)
        b.bias.copy_(a.bias)
    fa, fb = (yf.to(DEV).requires_grad_(True) for _ in range(2))
    oa, ob = a(y._like(fa)), b(y._like(fb))
    ref = _keys(E.expanded_sites(coarse, R.cube_offsets(ks), 2, 1, True))
    assert torch.equal(oa.keys, ob.keys) and oa.keys is not ob.keys and torch.equal(oa.keys.cpu(), ref)
    assert oa.tensor_stride == ob.tensor_stride == 1 and torch.equal(oa.F, ob.F)
    g = torch.randn(oa.F.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    (oa.F * g).sum().backward()
    (ob.F * g).sum().backward()
    assert torch.equal(fa.grad, fb.grad) and torch.equal(a.kernel.grad, b.kernel.grad) and torch.equal(a.bias.grad, b.bias.grad)


@pytest.mark.parametrize("cls,ks", [("MinkowskiPoolingTranspose", 2), ("MinkowskiPoolingTranspose", 3), ("MinkowskiAvgUnpooling", 3)])
def test_transposed_pooling_on_expanded_sites(cls, ks):
    from vdetr_amd import minkowski as ME
    coarse, yf, y, _ = _coarse()
    pool = getattr(ME, cls)(ks, stride=2, expand_coordinates=True)
    out = pool(y)
    offsets = R.cube_offsets(ks)
    ref_sites = E.expanded_sites(coarse, offsets, 2, 1, True)
    assert torch.equal(out.keys.cpu(), _keys(ref_sites)) and out.tensor_stride == 1
    assert out.keys is y.coordinate_manager.expanded(y.keys, 2, 1, ME.KernelGenerator(ks, dimension=3), True)
    nbr = R.neighbour_table(coarse, ref_sites, E.reach(offsets, 2, 1, True))
    assert bool((nbr >= 0).any(0).all())
    ry, ric, _ = R.pool_forward(yf, nbr, pool.mode)
    assert bool(((out.F.cpu().double() - ry).abs() <= R.pool_bound_forward(yf, nbr, ric)).all())


@functools.lru_cache(maxsize=None)
def _tied_inputs(nin, nout, C):
    g = torch.Generator().manual_seed(nin + nout + C)
    values = torch.tensor([-1.5, -1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 2.0])
    return values[torch.randint(0, 8, (nin, C), generator=g)], torch.randn(nout, C, generator=g)


@pytest.mark.parametrize("mode", ["sum", "avg", "max"])
@pytest.mark.parametrize("region", ["cube3", "cube2", "cross3", "cube3-d2"])
def test_pooling_on_expanded_sites(region, mode):
    from vdetr_amd import minkowski as ME
    sites, (offsets, _, _) = _cloud(), E.REGIONS[region]
    gen = ME.KernelGenerator(region_type=ME.RegionType.CUSTOM, region_offsets=offsets, dimension=3)
    pool = {"sum": ME.MinkowskiSumPooling, "avg": ME.MinkowskiAvgPooling, "max": ME.MinkowskiMaxPooling}[mode](
        3, kernel_generator=gen, expand_coordinates=True)
    ref_sites = E.expanded_sites(sites, offsets, 1, 1, False)
    xf, dy = _tied_inputs(len(sites), len(ref_sites), 20)
    _, x, _ = _tensor(sites, 20)
    leaf = xf.to(DEV).requires_grad_(True)
    out = pool(x._like(leaf))
    assert torch.equal(out.keys.cpu(), _keys(ref_sites))
    (dx,) = torch.autograd.grad(out.F, leaf, dy.to(DEV))
    nbr = R.neighbour_table(sites, ref_sites, E.reach(offsets, 1, 1, False))
    y = out.F.detach().cpu()
    if mode == "max":
        ry, _, rarg = R.pool_forward(xf, nbr, "max", dtype=R.F32)
        assert torch.equal(y, ry) and torch.equal(dx.cpu(), R.pool_backward(dy, nbr, len(sites), "max", arg=rarg, dtype=R.F32))
    else:
        ry, ric, _ = R.pool_forward(xf, nbr, mode)
        assert bool(((y.double() - ry).abs() <= R.pool_bound_forward(xf, nbr, ric)).all())
        rdx = R.pool_backward(dy, nbr, len(sites), mode, ric)
        assert bool(((dx.cpu().double() - rdx).abs() <= R.pool_bound_backward(dy, nbr, len(sites), ric)).all())


@pytest.mark.parametrize("region", ["cube2", "cross3", "custom-x"])
def test_channelwise_convolution_on_expanded_sites(region):
    from vdetr_amd import minkowski as ME
    sites, (offsets, _, _) = _cloud(), E.REGIONS[region]
    gen = ME.KernelGenerator(region_type=ME.RegionType.CUSTOM, region_offsets=offsets, dimension=3)
    torch.manual_seed(3)
    cw = ME.MinkowskiChannelwiseConvolution(20, kernel_generator=gen, bias=True, expand_coordinates=True).to(DEV)
    with torch.no_grad():
        cw.bias.normal_()
    f, x, _ = _tensor(sites, 20, seed=6)
    out = cw(x)
    ref_sites = E.expanded_sites(sites, offsets, 1, 1, False)
    assert torch.equal(out.keys.cpu(), _keys(ref_sites))
    nbr = R.neighbour_table(sites, ref_sites, E.reach(offsets, 1, 1, False))
    assert torch.equal(out.F.detach().cpu(), CW.forward32(f, cw.kernel.detach().cpu(), nbr, cw.bias.detach().cpu().reshape(-1)))


# ---- forward(x, coordinates) ---------------------------------------------------------------------------------------------------------
def _conv_case(conv, x, f, leaf, coordinates, in_sites, want_sites, offsets_step, want_inverse=None):
    """run ``conv(x, coordinates)`` and hold keys, inverse map, rows and gradients to the float64 oracle on the oracle's map"""
    out = conv(x, coordinates)
    want_keys = _keys(want_sites)
    assert torch.equal(out.keys.cpu(), want_keys)
    if want_inverse is None:
        assert out.inverse_mapping is None
    else:
        assert out.inverse_mapping.dtype == I32 and np.array_equal(out.inverse_mapping.cpu().numpy(), want_inverse)
    g = torch.randn(len(want_sites), conv.out_channels, generator=torch.Generator().manual_seed(8))
    conv.zero_grad()
    leaf.grad = None
    (out.F * g.to(DEV)).sum().backward()
    nbr = O.kernel_map(_keys(in_sites), want_keys, torch.tensor(offsets_step, dtype=I32).reshape(-1, 3))
    ry, rdf, rdw = _oracle(f, conv.kernel, conv.bias, nbr, g)
    _inside(out.F, ry, "out")
    _inside(leaf.grad, rdf, "dfeats")
    _inside(conv.kernel.grad, rdw, "dkernel")
    return out, nbr, ry


def test_coordinates_the_inputs_own_sites_reuse_the_cached_map():
    from vdetr_amd import minkowski as ME
    sites = _cloud()
    f, x, _ = _tensor(sites, 16)
    cm = x.coordinate_manager
    torch.manual_seed(0)
    conv = ME.MinkowskiConvolution(16, 24, kernel_size=3, bias=True, dimension=3).to(DEV)
    pool = ME.MinkowskiAvgPooling(3)
    plain, pooled = conv(x), pool(x)
    nmaps, nbr = len(cm.maps), cm.kernel_map(x.keys, x.keys, 1, 1, 3, False)[0]
    for given in (x, x.keys, plain):
        out = conv(x, given)
        assert torch.equal(out.F, plain.F) and out.keys is x.keys and out.inverse_mapping is None
        assert torch.equal(pool(x, given).F, pooled.F)
    assert len(cm.maps) == nmaps and cm.kernel_map(x.keys, x.keys, 1, 1, 3, False)[0] is nbr, "the cached map, the same nbr object"


def test_coordinates_another_tensor_of_the_manager():
    from vdetr_amd import minkowski as ME
    sites = _cloud()
    f, x, leaf = _tensor(sites, 16, grad=True)
    mask = torch.from_numpy(np.random.default_rng(1).random(len(sites)) < 0.4)
    other = ME.MinkowskiPruning()(x, mask.to(DEV))
    torch.manual_seed(1)
    conv = ME.MinkowskiConvolution(16, 24, kernel_size=3, bias=True, dimension=3).to(DEV)
    with torch.no_grad():
        conv.bias.normal_()
    out, _, _ = _conv_case(conv, x, f, leaf, other, sites, sites[mask.numpy()], R.cube_offsets(3))
    assert out.keys is other.keys and out.tensor_stride == 1
    nmaps = len(x.coordinate_manager.maps)
    assert ME.MinkowskiSumPooling(3)(x, other).keys is other.keys and len(x.coordinate_manager.maps) == nmaps, "one map for both"


@functools.lru_cache(maxsize=None)
def _target_list(lattice=1):
    """a shuffled coordinate list [M, 4] on the cloud: input sites, duplicates, and targets far from every input site"""
    sites = _cloud()
    rng = np.random.default_rng(12)
    near = sites[rng.permutation(len(sites))[:160]].copy()
    near[:, 1:] = np.floor_divide(near[:, 1:], lattice) * lattice
    far = near[:90] + np.array([0, 40, -40, 40]) * lattice
    coords = np.concatenate((near, far, near[:50], far[:20]))
    return sites, coords[rng.permutation(len(coords))]


def test_coordinates_a_shuffled_list_with_duplicates_and_unreached_targets():
    from vdetr_amd import minkowski as ME
    sites, coords = _target_list()
    want_sites, want_inverse = E.target_sites(coords)
    assert len(want_sites) < len(coords)
    f, x, leaf = _tensor(sites, 16, grad=True)
    torch.manual_seed(2)
    conv = ME.MinkowskiConvolution(16, 24, kernel_size=3, bias=True, dimension=3).to(DEV)
    with torch.no_grad():
        conv.bias.normal_()
    given = torch.from_numpy(coords).to(I32).to(DEV)
    out, nbr, ry = _conv_case(conv, x, f, leaf, given, sites, want_sites, R.cube_offsets(3), want_inverse)
    empty = ~(nbr >= 0).any(0)
    assert 4 * int(empty[torch.from_numpy(want_inverse)].sum()) >= len(coords), "a quarter of the targets have no neighbour"
    assert torch.equal(out.F.detach()[empty.to(DEV)], conv.bias.detach().expand(int(empty.sum()), -1)), "a zero row plus bias"
    # the rows in the caller's order against the oracle on the caller's own list (duplicates and all)
    listed = O.kernel_map(_keys(sites), _keys(coords), torch.tensor(R.cube_offsets(3), dtype=I32))
    ref = O.sparse_conv(f.double(), conv.kernel.detach().cpu().double(), listed) + conv.bias.detach().cpu().double()
    _inside(out.F[out.inverse_mapping.long()], ref, "rows in the caller's order")
    assert out.keys is conv(x, given).keys, "cached per coordinate tensor"
    # int64 coordinates give the same sites; the poolings write their empty-row value
    assert torch.equal(conv(x, given.long()).F, out.F.detach())
    for cls in (ME.MinkowskiSumPooling, ME.MinkowskiAvgPooling, ME.MinkowskiMaxPooling):
        p = cls(3)(x, given)
        assert torch.equal(p.keys, out.keys) and np.array_equal(p.inverse_mapping.cpu().numpy(), want_inverse)
        assert bool((p.F[empty.to(DEV)] == 0).all()) and bool((p.F[~empty.to(DEV)] != 0).any())
        table = R.neighbour_table(sites, want_sites, R.cube_offsets(3))
        rp, ric, _ = R.pool_forward(f, table, cls.mode, dtype=R.F32 if cls.mode == "max" else R.F64)
        if cls.mode == "max":
            assert torch.equal(p.F.cpu(), rp)
        else:
            assert bool(((p.F.cpu().double() - rp).abs() <= R.pool_bound_forward(f, table, ric)).all())
    cw = ME.MinkowskiChannelwiseConvolution(16, kernel_size=3, bias=True).to(DEV)
    with torch.no_grad():
        cw.bias.normal_()
    c = cw(x, given)
    table = R.neighbour_table(sites, want_sites, R.cube_offsets(3))
    assert torch.equal(c.F.detach().cpu(), CW.forward32(f, cw.kernel.detach().cpu(), table, cw.bias.detach().cpu().reshape(-1)))
    assert np.array_equal(c.inverse_mapping.cpu().numpy(), want_inverse)


@pytest.mark.parametrize("ks", [2, 3])
def test_coordinates_a_strided_convolution_onto_given_sites(ks):
    from vdetr_amd import minkowski as ME
    sites, coords = _target_list(lattice=2)
    want_sites, want_inverse = E.target_sites(coords)
    f, x, leaf = _tensor(sites, 16, grad=True)
    torch.manual_seed(ks)
    conv = ME.MinkowskiConvolution(16, 24, kernel_size=ks, stride=2, dimension=3).to(DEV)
    out, nbr, _ = _conv_case(conv, x, f, leaf, torch.from_numpy(coords).to(I32).to(DEV), sites, want_sites, R.cube_offsets(ks), want_inverse)
    assert out.tensor_stride == 2 and 2 not in x.coordinate_manager.keys, "given sites are never the canonical ones"
    assert 0 < int((nbr >= 0).any(0).sum()) < nbr.shape[1]


def test_coordinates_a_transposed_convolution_onto_a_pruned_tensors_sites():
    from vdetr_amd import minkowski as ME
    coarse, yf, y, x = _coarse()
    sites = _cloud()
    mask = torch.from_numpy(np.random.default_rng(2).random(len(sites)) < 0.5)
    pruned = ME.MinkowskiPruning()(x, mask.to(DEV))
    torch.manual_seed(4)
    up = ME.MinkowskiConvolutionTranspose(16, 8, kernel_size=2, stride=2, bias=True, dimension=3).to(DEV)
    leaf = yf.to(DEV).requires_grad_(True)
    step = [tuple(-v for v in o) for o in R.cube_offsets(2)]  # the transposed map reads v - offset * out_ts
    out, nbr, _ = _conv_case(up, y._like(leaf), yf, leaf, pruned, coarse, sites[mask.numpy()], step)
    assert out.keys is pruned.keys and out.tensor_stride == 1
    assert bool((nbr >= 0).any(0).all()), "every fine site has its parent"


# ---- errors, inference, geometry -------------------------------------------------------------------------------------------------------
def test_errors():
    from vdetr_amd import minkowski as ME
    sites = _cloud()
    _, x, _ = _tensor(sites, 8)
    _, other, _ = _tensor(sites, 8)
    conv = ME.MinkowskiConvolution(8, 8, kernel_size=3, dimension=3).to(DEV)
    layers = [conv, ME.MinkowskiChannelwiseConvolution(8, kernel_size=3).to(DEV), ME.MinkowskiAvgPooling(3)]
    coords = torch.from_numpy(sites[:50]).to(I32).to(DEV)
    for layer in layers:
        with pytest.raises(ValueError, match="different coordinate manager"):
            layer(x, other)
        with pytest.raises(ValueError, match="tensor stride 2.*output stride is 1"):
            layer(x, ME.SparseTensor(x.F, tensor_stride=2, coordinate_manager=x.coordinate_manager, keys=x.keys))
        with pytest.raises(ValueError, match="float32"):
            layer(x, coords.float())
        with pytest.raises(ValueError, match="cpu"):
            layer(x, coords.cpu())
        with pytest.raises(ValueError, match=r"\(50, 3\)"):
            layer(x, coords[:, :3].contiguous())
        with pytest.raises(ValueError, match="list"):
            layer(x, sites[:50].tolist())
    strided = ME.MinkowskiConvolution(8, 8, kernel_size=2, stride=2, dimension=3).to(DEV)
    with pytest.raises(ValueError, match="tensor stride 1.*output stride is 2"):
        strided(x, x)
    for cls, args in ((ME.MinkowskiConvolution, (8, 8, 3)), (ME.MinkowskiChannelwiseConvolution, (8, 3)), (ME.MinkowskiMaxPooling, (3,))):
        expanding = cls(*args, expand_coordinates=True).to(DEV)
        with pytest.raises(ValueError, match="expand_coordinates=True"):
            expanding(x, coords)
        with pytest.raises(ValueError, match="expand_coordinates=True"):
            expanding(x, x)
    for cls, args in ((ME.MinkowskiConvolution, (8, 8, 3)), (ME.MinkowskiChannelwiseConvolution, (8, 3)), (ME.MinkowskiSumPooling, (3,)),
                      (ME.MinkowskiAvgPooling, (3,)), (ME.MinkowskiMaxPooling, (3,))):
        with pytest.raises(NotImplementedError, match="stride 2"):
            cls(*args, stride=2, expand_coordinates=True)
    with pytest.raises(ValueError, match="origin"):
        ME.MinkowskiConvolution(8, 8, kernel_size=3, expand_coordinates=True, dimension=3).to(DEV)(ME.MinkowskiGlobalSumPooling()(x))


def test_eval_mode_fuses_an_expanding_convolution_with_its_batch_norm():
    from vdetr_amd import minkowski as ME
    sites = _cloud()
    _, x, _ = _tensor(sites, 16)
    torch.manual_seed(6)
    conv = ME.MinkowskiConvolution(16, 24, kernel_size=3, bias=True, expand_coordinates=True, dimension=3).to(DEV).eval()
    bn = ME.MinkowskiBatchNorm(24).to(DEV).eval()
    coords = torch.from_numpy(_target_list()[1]).to(I32).to(DEV)
    plain_conv = ME.MinkowskiConvolution(16, 24, kernel_size=3, dimension=3).to(DEV).eval()
    with torch.no_grad():
        conv.bias.normal_()
        bn.bn.running_mean.normal_()
        bn.bn.running_var.uniform_(0.5, 1.5)
        for layer, given in ((conv, None), (plain_conv, coords)):
            fused = bn(layer(x, given), act="relu")
            assert ME.LAST_PATHS[-1] == "fused"
            ME.INFER_FUSED = False
            try:
                plain = bn(layer(x, given), act="relu")
                assert ME.LAST_PATHS[-1] == "composition"
            finally:
                ME.INFER_FUSED = True
            assert torch.equal(fused.F, plain.F) and fused.keys is plain.keys and fused.F.shape[0] == fused.keys.shape[0]


def test_a_geometry_pass_builds_the_expanded_sites_and_their_maps():
    from vdetr_amd import minkowski as ME
    sites = _cloud()
    _, x, _ = _tensor(sites, 8)
    cm = x.coordinate_manager
    torch.manual_seed(7)
    net = torch.nn.Sequential(ME.MinkowskiConvolution(8, 16, kernel_size=3, expand_coordinates=True, dimension=3), ME.MinkowskiBatchNorm(16),
                              ME.MinkowskiReLU(), ME.MinkowskiConvolution(16, 16, kernel_size=3, dimension=3),
                              ME.MinkowskiAvgPooling(2, expand_coordinates=True)).to(DEV)
    with ME.geometry_only():
        g = net(x)
    nmaps, nexp = len(cm.maps), len(cm._expanded)
    assert nmaps == 3 and nexp == 2
    a, b = net(x), net(x)
    assert len(cm.maps) == nmaps and len(cm._expanded) == nexp, "the geometry pass built everything"
    assert a.keys is b.keys and a.keys is g.keys and a.F.shape == g.F.shape and torch.equal(a.F, b.F)
    first = E.expanded_sites(sites, R.cube_offsets(3), 1, 1, False)
    assert torch.equal(a.keys.cpu(), _keys(E.expanded_sites(first, R.cube_offsets(2), 1, 1, False)))
    assert list(cm.keys) == [1] and cm.keys[1] is x.keys, "expanded key sets never become canonical"
