"""csrc/sparse_voxel.hip on the GPU against tests/voxelize_restatement.py: the maps word for word (np.unique), the key arithmetic
against torch's own device expression, the range flag, the quantisation modes and their gradients bit for bit (sequential float32
folds), the MinkowskiEngine-named API on top, and the model's entry from raw clouds."""
import itertools

import numpy as np
import pytest
import torch

import voxelize_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _np(t):
    return t.detach().cpu().numpy()


def _check_maps(vm, keys):
    """a VoxelMap against the restatement on the same int64 keys: ==, dtypes included"""
    want = R.voxel_maps(keys)
    assert len(vm) == 5
    for name, got, w in zip(("sites", "inverse", "first", "seg", "order"), vm, want):
        got = _np(got)
        assert got.dtype == w.dtype and got.shape == w.shape and np.array_equal(got, w), name
    return want


def _sizes():
    from vdetr_amd import sparse_ops as S
    T = S.voxel_tile()
    return T, (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7)


def _coords_of_ids(ids, batch=0):
    """site ids -> [N, 4] coordinates whose KEY order is the id order (z carries the id; negative values included)"""
    ids = np.asarray(ids, dtype=np.int64)
    return np.stack((np.full_like(ids, batch), np.full_like(ids, -3), np.full_like(ids, 2), ids - 2000), 1)


def test_maps_at_every_size_all_distinct_and_all_in_one_voxel():
    from vdetr_amd import sparse_ops as S
    T, sizes = _sizes()
    rng = np.random.default_rng(0)
    for n in sizes:
        for ids in (rng.permutation(n), np.zeros(n, np.int64)):  # all distinct (shuffled); one run of n (longer than a tile at 3T + 7)
            coords = _coords_of_ids(ids)
            vm = S.voxel_map_coords(torch.from_numpy(coords).to(DEV))
            _check_maps(vm, R.pack_keys(coords))
            assert vm.num_scenes == (1 if n else 0)
            assert vm.sites.shape[0] == (len(set(ids.tolist())))
    for dtype in (torch.int32, torch.int64):  # random duplicates, either integer width
        coords = np.concatenate((rng.integers(0, 3, (2 * T + 5, 1)), rng.integers(-6, 6, (2 * T + 5, 3))), 1)
        _check_maps(S.voxel_map_coords(torch.from_numpy(coords).to(DEV).to(dtype)), R.pack_keys(coords))


@pytest.mark.parametrize("run", [2, 3, 4, 5])
def test_maps_with_runs_across_every_tile_boundary(run):
    from vdetr_amd import sparse_ops as S
    T, _ = _sizes()
    n = 3 * T + 7
    ids = np.arange(n)
    for b in (T, 2 * T, 3 * T):
        start = b - (run + 1) // 2
        ids[start:start + run] = ids[start]
    perm = np.random.default_rng(run).permutation(n)
    coords = _coords_of_ids(ids[perm])
    keys = R.pack_keys(coords)
    _, _, _, seg, _ = _check_maps(S.voxel_map_coords(torch.from_numpy(coords).to(DEV)), keys)
    for b in (T, 2 * T, 3 * T):  # a run of `run` keys lies across every multiple of the tile, in sorted order
        r = np.searchsorted(seg, b, side="right") - 1
        assert seg[r] < b < seg[r + 1] and seg[r + 1] - seg[r] == run


@pytest.mark.parametrize("offsets", [(0, 700, 700, 1500), (0, 1500)], ids=["B3-empty-middle", "B1"])
def test_maps_from_raw_clouds(offsets):
    """points with negative coordinates and extra columns, a row stride wider than the three coordinates, host or device offsets"""
    from vdetr_amd import sparse_ops as S
    g = torch.Generator().manual_seed(len(offsets))
    pts = torch.cat(((torch.rand(1500, 3, generator=g) - 0.5) * 0.16, torch.randn(1500, 4, generator=g)), 1)
    keys = R.pack_keys(R.cloud_coords(pts.numpy(), offsets, 0.02))
    assert len(np.unique(keys)) < 1200  # (duplicates)
    for off in (list(offsets), torch.tensor(offsets, dtype=torch.int32, device=DEV)):
        vm = S.voxel_map(pts.to(DEV), off, 0.02)
        _check_maps(vm, keys)
        assert vm.num_scenes == len(offsets) - 1
    wide = torch.zeros(1500, 16, device=DEV)
    wide[:, 5:12] = pts.to(DEV)
    _check_maps(S.voxel_map(wide[:, 5:9], list(offsets), 0.02), keys)
    empty = S.voxel_map(pts[:0].to(DEV), [0, 0], 0.02)
    assert [t.shape[0] for t in empty] == [0, 0, 0, 1, 0] and empty.seg.tolist() == [0] and empty.num_scenes == 1


@pytest.mark.parametrize("voxel", [0.01, 0.02, 0.05, 0.03, 0.013])  # (at 0.03 float32(1 / 0.03) and 1 / float32(0.03) differ)
def test_key_arithmetic_is_the_device_expression(voxel):
    """coordinates at k * voxel and one ulp either side, k negative, zero and positive up to the edge of the key range, and -0.0:
    the voxel indices equal torch.floor(p / voxel).to(torch.int32) evaluated on the device here"""
    from vdetr_amd import sparse_ops as S
    rng = np.random.default_rng(int(voxel * 100))
    ks = np.concatenate((np.arange(-64, 65), rng.integers(-32000, 32000, 1500)))
    base = (ks * voxel).astype(np.float32)
    xs = np.concatenate((base, np.nextafter(base, np.float32(np.inf)), np.nextafter(base, np.float32(-np.inf)), np.float32([-0.0, 0.0])))
    xs = xs[(np.abs(xs) < 32700 * voxel)]
    pts = torch.zeros(len(xs), 3)
    pts[:, 0] = torch.from_numpy(xs)
    pts[:, 1] = torch.from_numpy(xs[::-1].copy())
    p = pts.to(DEV)
    want = torch.floor(p / voxel).to(torch.int32)
    vm = S.voxel_map(p, [0, len(xs)], voxel)
    got = S.unpack_keys(vm.sites)[vm.inverse.long()]
    assert torch.equal(got[:, 1:], want) and int(got[:, 0].abs().max()) == 0
    assert np.array_equal(_np(want).astype(np.float32), R.voxel_indices(pts.numpy(), voxel))  # (and the restatement's arithmetic)


def test_range_flag():
    from vdetr_amd import sparse_ops as S
    voxel = 0.05

    def cloud(value, column=0):
        p = torch.rand(300, 3) * 2
        p[123, column] = value
        return p.to(DEV)

    def index(value):
        return int(torch.floor(torch.tensor([value], device=DEV) / voxel).to(torch.int32))

    hi, lo, top, bottom = 32768.5 * voxel, -32768.5 * voxel, 32767.5 * voxel, -32767.5 * voxel
    assert (index(hi), index(lo), index(top), index(bottom)) == (32768, -32769, 32767, -32768)
    for column, bad in itertools.product((0, 2), (hi, lo, float("nan"), float("inf"), float("-inf"), 3.0e38)):
        with pytest.raises(ValueError, match="voxel coordinates outside the 16-bit key range"):
            S.voxel_map(cloud(bad, column), [0, 300], voxel)
    for legal in (top, bottom):
        vm = S.voxel_map(cloud(legal, 1), [0, 100, 300], voxel)
        c = S.unpack_keys(vm.sites)[vm.inverse.long()[123]]
        assert c.tolist() == [1, int(c[1]), index(legal), int(c[3])]
    coords = torch.zeros(50, 4, dtype=torch.int32)
    for row in ([0, 32768, 0, 0], [0, 0, 0, -32769], [32768, 0, 0, 0], [-1, 0, 0, 0]):
        c = coords.clone()
        c[7] = torch.tensor(row, dtype=torch.int32)
        for dtype in (torch.int32, torch.int64):
            with pytest.raises(ValueError, match="voxel coordinates outside the 16-bit key range"):
                S.voxel_map_coords(c.to(DEV).to(dtype))
    c = coords.clone()
    c[7], c[8] = torch.tensor([32767, 32767, -32768, 0], dtype=torch.int32), torch.tensor([0, -32768, 32767, 5], dtype=torch.int32)
    vm = S.voxel_map_coords(c.to(DEV))
    _check_maps(vm, R.pack_keys(c.numpy()))
    assert vm.num_scenes == 32768
    with pytest.raises(ValueError, match="16-bit key range"):
        S.voxel_map(cloud(0.5), [0] + [300] * 32769, voxel)  # B = 32769 scenes


_CASE = {}


def _feature_case(C):
    """3T + 7 points in runs of 1 .. ~12 over two scenes (shared by the mode and gradient tests), a NaN and tied rows included"""
    if C not in _CASE:
        from vdetr_amd import sparse_ops as S
        T, _ = _sizes()
        n = 3 * T + 7
        rng = np.random.default_rng(C)
        coords = np.concatenate((rng.integers(0, 2, (n, 1)), rng.integers(-4, 4, (n, 3))), 1)
        coords[-5:] = [[1, 9, 9, 9], [1, 9, 9, 8], [1, 9, 9, 9], [1, 9, 9, 7], [1, 9, 9, 9]]  # (a run of 3, two runs of 1)
        feats = rng.standard_normal((n, C)).astype(np.float32)
        feats[n - 3] = feats[n - 5]               # two tied rows in one voxel: the lower row wins every channel it wins at all
        feats[11, 0] = np.nan                     # a NaN wins its site's maximum and poisons its sum
        feats[n - 1, C - 1] = np.nan
        keys = R.pack_keys(coords)
        maps = R.voxel_maps(keys)
        vm = S.voxel_map_coords(torch.from_numpy(coords).to(DEV))
        _CASE[C] = (feats, maps, vm)
    return _CASE[C]


@pytest.mark.parametrize("C", [1, 3, 6, 7, 64])
def test_modes_equal_the_sequential_fold(C):
    from vdetr_amd import sparse_ops as S
    feats, (sites, inverse, first, seg, order), vm = _feature_case(C)
    m = len(sites)
    x = torch.from_numpy(feats).to(DEV)
    assert np.array_equal(_np(S.voxel_reduce(x, vm, "first")).view(np.uint32), feats[first].view(np.uint32))  # (copies: a NaN's bits too)
    for mode in ("sum", "average", "max"):
        want, winners = R.reduce_features(feats, inverse, m, mode)
        got, arg = S.voxel_reduce(x, vm, mode, return_arg=True)
        again, arg2 = S.voxel_reduce(x, vm, mode, return_arg=True)
        assert got.dtype == torch.float32 and tuple(got.shape) == (m, C)
        g, w = _np(got), want
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.isnan(w).any(), mode
        assert np.array_equal(g[~np.isnan(w)].view(np.uint32), w[~np.isnan(w)].view(np.uint32)), mode  # == bit for bit
        assert np.array_equal(_np(again).view(np.uint32), g.view(np.uint32)), mode  # a second run is bit-identical
        if mode == "max":
            assert arg.dtype == torch.int32 and np.array_equal(_np(arg), winners) and torch.equal(arg, arg2)
            tie = inverse[len(feats) - 5]
            assert (winners[tie] != len(feats) - 3).all()  # the tied higher row never wins
        else:
            assert arg is None


@pytest.mark.parametrize("C", [1, 3, 6, 7, 64])
def test_gradients_equal_the_restatement(C):
    from vdetr_amd import sparse_ops as S
    feats, (sites, inverse, first, seg, order), vm = _feature_case(C)
    m, n = len(sites), len(feats)
    d_sites = np.random.default_rng(100 + C).standard_normal((m, C)).astype(np.float32)
    for mode in ("sum", "average", "max", "first"):
        x = torch.from_numpy(feats).to(DEV).requires_grad_(True)
        y, arg = S.voxel_reduce(x, vm, mode, return_arg=True)
        y.backward(torch.from_numpy(d_sites).to(DEV))
        want = R.reduce_grad(d_sites, inverse, m, mode, None if arg is None else _np(arg))
        got = _np(x.grad)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), mode
        if mode == "max":  # rows that win nothing get exact zeros
            lost = np.ones((n, C), bool)
            winners = _np(arg)
            for ch in range(C):
                lost[winners[:, ch], ch] = False
            assert lost.any() and (got[lost].view(np.uint32) == 0).all()
    # slice: forward a gather through inverse, backward the sum fold of the point gradients
    s = torch.from_numpy(d_sites).to(DEV).requires_grad_(True)
    p = S.voxel_slice(s, vm)
    assert torch.equal(p.detach().cpu(), torch.from_numpy(d_sites[inverse]))
    p.backward(torch.from_numpy(feats).nan_to_num(0.5).to(DEV))
    want = R.slice_grad(np.nan_to_num(feats, nan=0.5), inverse, m)
    assert np.array_equal(_np(s.grad).view(np.uint32), want.view(np.uint32))


def test_host_entry_points_refuse_bad_tables():
    from vdetr_amd import sparse_ops as S
    feats, _, vm = _feature_case(3)
    x = torch.from_numpy(feats).to(DEV)
    with pytest.raises(RuntimeError, match="features must be a float tensor"):
        S.voxel_reduce(x.double(), vm, "sum")
    with pytest.raises(RuntimeError, match="features must be a contiguous tensor"):
        S.voxel_reduce(torch.cat((x, x), 1)[:, :3], vm, "sum")
    with pytest.raises(RuntimeError, match="inverse is"):
        S.voxel_reduce(x[:-1].contiguous(), vm, "sum")
    with pytest.raises(ValueError, match="mode 'median'"):
        S.voxel_reduce(x, vm, "median")
    with pytest.raises(RuntimeError, match="vmap must be"):
        S.voxel_reduce(x, (vm.sites, vm.inverse), "sum")
    with pytest.raises(RuntimeError, match="site_features has"):
        S.voxel_slice(x, vm)


def test_sparse_quantize_every_return_combination():
    from vdetr_amd import minkowski as ME
    rng = np.random.default_rng(5)
    n = 700
    pts = ((rng.random((n, 3)) - 0.5) * 0.4).astype(np.float32)
    feats = rng.standard_normal((n, 5)).astype(np.float32)
    labels = rng.integers(0, 3, n)
    coords = np.concatenate((np.zeros((n, 1), np.int64), R.voxel_indices(pts, 0.05).astype(np.int64)), 1)
    sites, inverse, first, seg, order = R.voxel_maps(R.pack_keys(coords))
    site_labels = R.site_labels(labels, inverse, len(sites), -100)
    assert (site_labels == -100).any() and (site_labels != -100).any()
    P, F, Lb = torch.from_numpy(pts).to(DEV), torch.from_numpy(feats).to(DEV), torch.from_numpy(labels).to(DEV)
    want = {"coords": coords[first][:, 1:], "feats": feats[first], "labels": site_labels, "index": first, "inverse": inverse}
    for use_f, use_l, ret_i, ret_v in itertools.product((False, True), repeat=4):
        out = ME.sparse_quantize(P, features=F if use_f else None, labels=Lb if use_l else None, return_index=ret_i,
                                 return_inverse=ret_v, quantization_size=0.05)
        names = ["coords"] + ["feats"] * use_f + ["labels"] * use_l + ["index"] * ret_i + ["inverse"] * ret_v
        out = (out,) if len(names) == 1 else out
        assert len(out) == len(names)
        for name, t in zip(names, out):
            assert t.is_cuda and np.array_equal(_np(t), want[name]), (name, use_f, use_l, ret_i, ret_v)
    only = ME.sparse_quantize(P, return_maps_only=True, quantization_size=0.05)
    both = ME.sparse_quantize(P, return_maps_only=True, return_inverse=True, quantization_size=0.05)
    assert np.array_equal(_np(only), first) and np.array_equal(_np(both[0]), first) and np.array_equal(_np(both[1]), inverse)
    # ready integer coordinates, with a batch column, and a size per axis; another ignore_label
    C4 = torch.from_numpy(coords).to(DEV)
    c, lab = ME.sparse_quantize(C4, labels=Lb.int(), ignore_label=255)
    assert np.array_equal(_np(c), coords[first]) and c.dtype == torch.int32
    assert np.array_equal(_np(lab), R.site_labels(labels, inverse, len(sites), 255)) and lab.dtype == torch.int32
    per_axis = ME.sparse_quantize(P, quantization_size=(0.05, 0.05, 0.05))
    assert np.array_equal(_np(per_axis), _np(torch.floor(P / torch.tensor([0.05] * 3, device=DEV)).int())[first])


def test_tensor_field_and_sparse_tensor_modes():
    from vdetr_amd import minkowski as ME
    modes = ME.SparseTensorQuantizationMode
    feats, (sites, inverse, first, seg, order), vm = _feature_case(6)
    clean = np.nan_to_num(feats, nan=0.25)
    coords = S_unpack(sites)[inverse]
    C4, F = torch.from_numpy(coords).int().to(DEV), torch.from_numpy(clean).to(DEV)
    for mode, name in ((modes.RANDOM_SUBSAMPLE, "first"), (modes.UNWEIGHTED_AVERAGE, "average"), (modes.UNWEIGHTED_SUM, "sum"),
                       (modes.MAX_POOL, "max")):
        x = ME.SparseTensor(F, coordinates=C4, quantization_mode=mode)
        want = R.reduce_features(clean, inverse, len(sites), name)[0]
        assert x.quantization_mode is mode and np.array_equal(_np(x.F).view(np.uint32), want.view(np.uint32)), name
        assert np.array_equal(_np(x.keys), sites) and np.array_equal(_np(x.unique_index), first)
        assert np.array_equal(_np(x.inverse_mapping), inverse) and x.coordinate_manager.num_scenes == 2
    assert ME.SparseTensor(F, coordinates=C4).quantization_mode is modes.RANDOM_SUBSAMPLE  # the default is unchanged
    field = ME.TensorField(F, C4)
    assert field.quantization_mode is modes.UNWEIGHTED_AVERAGE
    with pytest.raises(RuntimeError, match="call sparse"):
        field.inverse_mapping
    sp = field.sparse()
    assert np.array_equal(_np(sp.F).view(np.uint32), R.reduce_features(clean, inverse, len(sites), "average")[0].view(np.uint32))
    back = sp.slice(field)
    assert isinstance(back, ME.TensorField) and torch.equal(back.F, sp.F[field.inverse_mapping.long()]) and back.C is field.C
    assert np.array_equal(_np(field.inverse_mapping), inverse)
    # through a layer that keeps the sites, with gradients: d sp.F = the sum of the point gradients of each site
    f = F.clone().requires_grad_(True)
    fld = ME.TensorField(f, C4.float() + 0.25, quantization_mode=modes.UNWEIGHTED_SUM)  # (float coordinates are floored)
    y = ME.MinkowskiReLU()(fld.sparse()).slice(fld)
    d = torch.randn(y.F.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    y.F.backward(d)
    summed = R.reduce_features(clean, inverse, len(sites), "sum")[0]
    d_site = np.where(summed > 0, R.slice_grad(_np(d), inverse, len(sites)), np.float32(0))  # (the ReLU passes or selects +0)
    assert np.array_equal(_np(f.grad).view(np.uint32), R.reduce_grad(d_site.astype(np.float32), inverse, len(sites), "sum").view(np.uint32))
    other = ME.TensorField(F, C4)
    with pytest.raises(ValueError, match="whose sparse"):
        sp.slice(other)


def S_unpack(keys):
    return np.stack((keys >> 48, ((keys >> 32) & 0xFFFF) - 32768, ((keys >> 16) & 0xFFFF) - 32768, (keys & 0xFFFF) - 32768), 1)


# ---- the model's entry from raw clouds ---------------------------------------------------------------------------------------------
def _model_case():
    """two clouds [n, 6] (xyz + colour) on a floor and a wall, 2 cm voxels: most voxels hold several points"""
    g = torch.Generator().manual_seed(1)
    clouds = []
    for b in range(2):
        n = 5000 - 1200 * b
        u = torch.rand((n, 2), generator=g)
        floor = torch.stack((u[:, 0] * 2, u[:, 1] * 1.5, torch.zeros(n)), 1)
        wall = torch.stack((u[:, 0] * 2, torch.zeros(n), u[:, 1] * 1.2), 1)
        xyz = torch.cat((floor[: n // 2], wall[n // 2:])) + 1.0
        clouds.append(torch.cat((xyz, torch.rand((n, 3), generator=g)), 1))
    return clouds


def _inputs(clouds):
    clouds = [c.to(DEV) for c in clouds]
    return {"point_clouds": clouds, "point_cloud_dims_min": torch.stack([c[:, :3].min(0)[0] for c in clouds]),
            "point_cloud_dims_max": torch.stack([c[:, :3].max(0)[0] for c in clouds])}


def _build(**overrides):
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    from vdetr_amd.model_vdetr import build_vdetr, default_args
    torch.manual_seed(0)
    args = default_args(nqueries=32, dec_nlayers=2, preenc_npoints=256, voxel_size=0.02, use_color=True, **overrides)
    return build_vdetr(args, ScannetDatasetConfig(), "minkowski").to(DEV).eval()


def test_model_default_mode_keeps_its_keys_and_rows():
    """(a) the manager's stride-1 keys and unique_index equal the composition the entry replaced, computed here"""
    from vdetr_amd import minkowski as ME
    from vdetr_amd import sparse_ops as S
    model = _build()
    assert model.quantization_mode is ME.SparseTensorQuantizationMode.RANDOM_SUBSAMPLE
    inputs = _inputs(_model_case())
    cm = model.prepare_geometry(inputs)
    coordinates, features = ME.batch_sparse_collate([(p[:, :3] / model.voxel_size, p[:, 3:]) for p in inputs["point_clouds"]])
    keys_in = S.pack_keys(coordinates)
    keys, inverse = torch.unique(keys_in, return_inverse=True)
    first = torch.full((keys.shape[0],), keys_in.shape[0], dtype=torch.int64, device=DEV)
    first.scatter_reduce_(0, inverse, torch.arange(keys_in.shape[0], device=DEV), reduce="amin")
    assert keys.shape[0] < 0.9 * keys_in.shape[0]  # (duplicate voxels)
    assert torch.equal(cm.keys[1], keys) and torch.equal(cm.unique_index, first) and cm.num_scenes == 2
    assert torch.equal(cm.inverse_mapping.long(), inverse)
    with torch.no_grad():
        scenes = model.backbone_forward(inputs)
        x = ME.SparseTensor(features.contiguous(), coordinates=coordinates)  # the tensor the entry used to build
        assert torch.equal(x.keys, keys) and torch.equal(x.F, features[first])
        again = model.backbone_forward(dict(inputs, geometry=cm))
    for (xa, fa), (xb, fb) in zip(scenes, again):
        assert torch.equal(xa, xb) and torch.equal(fa, fb)


def test_model_average_mode_equals_the_deduplicated_cloud():
    """(b) quantization_mode="unweighted_average" with use_color: the output equals, with ==, the output for the cloud with one
    point per voxel whose colours are the restatement's averages, and differs from the default mode's; (c) prepare_geometry
    followed by forward gives (b) again"""
    clouds = _model_case()
    model = _build(quantization_mode="unweighted_average")
    plain = _build()
    plain.load_state_dict(model.state_dict())
    dedup = []
    for c in clouds:
        c = c.numpy()
        coords = R.cloud_coords(c, [0, len(c)], 0.02)
        sites, inverse, first, _, _ = R.voxel_maps(R.pack_keys(coords))
        avg = R.reduce_features(c[:, 3:], inverse, len(sites), "average")[0]
        dedup.append(torch.from_numpy(np.concatenate((c[first, :3], avg), 1)))
    inputs, inputs_dedup = _inputs(clouds), _inputs(dedup)
    for key in ("point_cloud_dims_min", "point_cloud_dims_max"):
        inputs_dedup[key] = inputs[key]
    with torch.no_grad():
        got = model(inputs)
        want = model(inputs_dedup)
        default = plain(inputs)
        prepared = model(dict(inputs, geometry=model.prepare_geometry(inputs)))
        scenes, scenes_want = model.backbone_forward(inputs), model.backbone_forward(inputs_dedup)
    for (xa, fa), (xb, fb) in zip(scenes, scenes_want):
        assert torch.equal(xa, xb) and torch.equal(fa, fb)
    for name in ("sem_cls_logits", "center_normalized", "size_normalized", "box_corners"):
        assert torch.equal(got["outputs"][name], want["outputs"][name]), name
        assert torch.equal(got["outputs"][name], prepared["outputs"][name]), name
    assert torch.equal(got["seed_xyz"], default["seed_xyz"])  # the same sites ...
    assert not torch.equal(got["outputs"]["sem_cls_logits"], default["outputs"]["sem_cls_logits"])  # ... other features
