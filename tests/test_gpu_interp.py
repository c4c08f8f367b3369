"""csrc/sparse_interp.hip on the GPU against tests/interp_restatement.py: the map word for word (nbr) and within 8 * 2^-24 (w), the
edges of the key fields, exact-value cases, forward and backward within the rounding bounds of their float32 sums, the backward's
extremes, bit reproducibility, no host read, and the MinkowskiEngine-named API on top."""
import numpy as np
import pytest
import torch

import interp_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24
RATIOS = {}  # the largest observed error / bound per check (printed: DESIGN 6.16 quotes them)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tile():
    from vdetr_amd import sparse_ops as S
    return S.interp_tile()


def _check_map(imap, keys, s, tfield):
    """an InterpMap against the restatement: nbr ==, w within 8 * 2^-24, an exact 0 where a corner is absent"""
    nbr, w = R.interp_map(keys, s, tfield)
    got_nbr, got_w = _np(imap.nbr), _np(imap.w)
    assert got_nbr.dtype == np.int32 and got_w.dtype == np.float32 and got_nbr.shape == got_w.shape == (len(tfield), 8)
    assert (imap.M, imap.N) == (len(keys), len(tfield))
    assert np.array_equal(got_nbr, nbr), np.nonzero((got_nbr != nbr).any(1))[0][:8]
    err = np.abs(got_w.astype(np.float64) - w).max() if w.size else 0.0
    print(f"interp map: N={len(tfield)} M={len(keys)} s={s} max |w - w64| = {err / EPS:.2f} x 2^-24")
    assert err <= 8 * EPS, err
    assert not got_w[nbr < 0].any()
    return nbr, w


def _map(keys, s, tfield):
    from vdetr_amd import sparse_ops as S
    return S.interp_map(_dev(keys), s, _dev(tfield))


def _sites(rng, M, scenes, s, box):
    """M distinct lattice sites of stride s in a box^3 block around zero, spread over `scenes` -> (keys sorted, coords)"""
    lo = -(box // 2)
    grid = np.stack(np.meshgrid(*(np.arange(box),) * 3, indexing="ij"), -1).reshape(-1, 3)
    every = np.concatenate([np.concatenate((np.full((len(grid), 1), b), (grid + lo) * s), 1) for b in scenes])
    coords = every[rng.choice(len(every), M, replace=False)] if M else np.zeros((0, 4), np.int64)
    keys = R.pack_keys(coords)
    order = np.argsort(keys)
    return keys[order], coords[order]


def _points(rng, N, batches, s, box):
    lo = -(box // 2)
    p = (rng.random((N, 3)) * (box + 1) + lo - 1) * s  # a cell beyond the block on either side
    return np.concatenate((rng.choice(np.asarray(batches, dtype=np.float64), (N, 1)), p), 1).astype(np.float32)


@pytest.mark.parametrize("M", [0, 1, 2, 3000])
def test_map_at_every_size(M):
    T = _tile()
    rng = np.random.default_rng(M)
    box = 16 if M > 2 else 2
    for scenes in ((0,), (0, 2)):  # one scene; three with the middle one empty
        keys, _ = _sites(rng, M, scenes, 1, box)
        batches = range(max(scenes) + 1)
        for N in (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7):
            tfield = _points(rng, N, batches, 1, box)
            nbr, _ = _check_map(_map(keys, 1, tfield), keys, 1, tfield)
            if len(scenes) > 1:
                assert not (nbr[tfield[:, 0] == 1] >= 0).any()
            if M == 3000 and N >= T:
                assert 0.1 < (nbr >= 0).mean() < 0.9  # (neither empty nor full: both answers of every search are met)


@pytest.mark.parametrize("s", [1, 2, 3, 4, 8])
def test_map_at_every_stride(s):
    T = _tile()
    rng = np.random.default_rng(10 + s)
    keys, coords = _sites(rng, 900, (0, 1), s, 10)
    assert coords[:, 1:].min() < 0 < coords[:, 1:].max() and (coords[:, 1:] % s == 0).all()
    tfield = _points(rng, T + 1, (0, 1), s, 10)
    tfield[:40, 1:] = coords[:40, 1:]  # points exactly on sites
    tfield[:40, 0] = coords[:40, 0]
    nbr, w = _check_map(_map(keys, s, tfield), keys, s, tfield)
    assert np.array_equal(nbr[:40, 0], np.arange(40)) and (tfield[:, 1:] < 0).any() and (tfield[:, 1:] > 0).any()
    # a key set off the lattice of s (sites of stride 1 read at stride s): still the rows of the corners' keys
    keys1, _ = _sites(rng, 2000, (0, 1), 1, 14)
    tfield = _points(rng, T + 1, (0, 1), 1, 14)
    _check_map(_map(keys1, s, tfield), keys1, s, tfield)


def test_map_at_the_edges_of_the_fields():
    coords = np.array([[0, 5, 5, 32767], [0, 5, 6, -32768], [0, 32767, 0, 0], [1, -32768, 0, 0], [0, 32767, 32767, 32767],
                       [0, -32768, -32768, -32768], [3, 0, 0, 0], [3, 0, 0, 1]], np.int64)
    keys = R.pack_keys(coords)
    order = np.argsort(keys)
    keys, coords = keys[order], coords[order]
    at = {tuple(c): r for r, c in enumerate(coords.tolist())}
    nan, inf = np.nan, np.inf
    tfield = np.array([[0, 5, 5, 32767.5],            # upper z corners outside; the decoy (5, 6, -32768) is where a carry would land
                       [0, 32767.5, 0, 0], [0, 32767.25, 32767.5, 32767.75], [1, -32768, 0, 0], [0, -32768, -32768, -32768],
                       [1, -32768.5, 0, 0], [0, -40000, 0, 0], [0, 40000, 0, 0], [0, 5, 5, 32768],
                       [0, nan, 0, 0], [0, 0, inf, 0], [0, 0, 0, -inf], [nan, 5, 5, 5], [inf, 5, 5, 5],
                       [0.5, 5, 5, 32767], [-1, 5, 5, 32767], [32768, 5, 5, 32767], [2, 0, 0, 0],   # batch 2 has no site
                       [3, 0, 0, 0.25], [3, 0, 0, 1], [3, -1e-9, 0, 0.5], [0, 5, 5.999, 32767.999]], np.float32)
    nbr, w = _check_map(_map(keys, 1, tfield), keys, 1, tfield)
    got = _np(_map(keys, 1, tfield).nbr)
    assert got[0].tolist() == [at[(0, 5, 5, 32767)]] + [-1] * 7
    assert got[1].tolist() == [at[(0, 32767, 0, 0)]] + [-1] * 7 and got[2].tolist() == [at[(0, 32767, 32767, 32767)]] + [-1] * 7
    assert got[3][0] == at[(1, -32768, 0, 0)] and got[4][0] == at[(0, -32768, -32768, -32768)]
    assert not (got[5:18] >= 0).any()
    assert got[18].tolist() == [at[(3, 0, 0, 0)], at[(3, 0, 0, 1)]] + [-1] * 6 and got[19][0] == at[(3, 0, 0, 1)]
    # the strides whose lower site falls below the field: (-32768 // 3) * 3 = -32769 is absent, the upper one is read
    keys3 = R.pack_keys([[0, -32766, 0, 0], [0, 32766, 0, 0]])
    tf3 = np.array([[0, -32768, 0, 0], [0, -32767.5, 0, 0], [0, 32767, 0, 0]], np.float32)
    nbr3, _ = _check_map(_map(keys3, 3, tf3), keys3, 3, tf3)
    assert nbr3[0].tolist() == [-1, -1, -1, -1, 0, -1, -1, -1] and nbr3[2].tolist() == [1] + [-1] * 7


def _filled_box(s, half=3, scenes=(0, 1)):
    grid = np.stack(np.meshgrid(*(np.arange(-half, half + 1),) * 3, indexing="ij"), -1).reshape(-1, 3) * s
    coords = np.concatenate([np.concatenate((np.full((len(grid), 1), b), grid), 1) for b in scenes])
    keys = R.pack_keys(coords)
    order = np.argsort(keys)
    return keys[order], coords[order]


@pytest.mark.parametrize("s,C", [(1, 4), (2, 3), (4, 64)])
def test_exact_values_on_sites_and_at_cell_midpoints(s, C):
    from vdetr_amd import sparse_ops as S
    rng = np.random.default_rng(s)
    keys, coords = _filled_box(s)
    # integer coordinates interpolate at themselves: weight 1 times the row plus exact zeros
    F = rng.standard_normal((len(keys), C)).astype(np.float32)
    rows = rng.integers(0, len(keys), 2 * _tile() + 5)
    imap = S.interp_map(_dev(keys), s, _dev(coords[rows].astype(np.float32)))
    assert np.array_equal(_np(imap.nbr)[:, 0], rows)
    assert np.array_equal(_np(S.interpolate(_dev(F), imap)), F[rows])
    # cell midpoints, all eight corners there, small-integer features: eight weights of 0.125 and exact sums
    inner = coords[(coords[:, 1:] < coords[:, 1:].max()).all(1)]
    tfield = (inner[rng.integers(0, len(inner), 300)] + np.array([0, s / 2, s / 2, s / 2])).astype(np.float32)
    Fi = rng.integers(-8, 9, (len(keys), C)).astype(np.float32)
    imap = S.interp_map(_dev(keys), s, _dev(tfield))
    nbr, w = R.interp_map(keys, s, tfield)
    assert (nbr >= 0).all() and (w == 0.125).all() and np.array_equal(_np(imap.w).astype(np.float64), w)
    assert np.array_equal(_np(S.interpolate(_dev(Fi), imap)).astype(np.float64), R.forward(Fi, nbr, w))


def _note(name, err, bound):
    ok = bound > 0
    ratio = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print(f"interp {name}: max error / bound = {ratio:.4f} (largest so far {RATIOS[name]:.4f})")
    assert (err <= bound).all(), (name, ratio)


def _check_forward_backward(keys, s, tfield, C, seed):
    """forward within 32 * 2^-24 * sum |F[nbr]|, backward within (n_m + 16) * 2^-24 * sum |dy| over the site's pairs"""
    from vdetr_amd import sparse_ops as S
    rng = np.random.default_rng(seed)
    M, N = len(keys), len(tfield)
    F = rng.standard_normal((M, C)).astype(np.float32)
    dy = rng.standard_normal((N, C)).astype(np.float32)
    imap = S.interp_map(_dev(keys), s, _dev(tfield))
    nbr, w64 = R.interp_map(keys, s, tfield)
    assert np.array_equal(_np(imap.nbr), nbr)
    x = _dev(F).requires_grad_(True)
    y = S.interpolate(x, imap)
    y.backward(_dev(dy))
    assert y.shape == (N, C) and x.grad.shape == (M, C)
    _note("forward", np.abs(_np(y).astype(np.float64) - R.forward(F, nbr, w64)), 32 * EPS * R.forward_bound(F, nbr))
    mass, count = R.backward_bound(dy, nbr, M)
    _note("backward", np.abs(_np(x.grad).astype(np.float64) - R.backward(dy, nbr, w64, M)), (count[:, None] + 16) * EPS * mass)
    lonely = count == 0
    assert not _np(x.grad)[lonely].any() and not np.signbit(_np(x.grad)[lonely]).any()  # an exact +0
    return imap, nbr, w64, F, dy, y.detach(), x.grad


@pytest.mark.parametrize("C", [1, 3, 4, 20, 64, 68])
def test_random_case_forward_and_backward(C):
    T = _tile()
    s, scenes = {1: (1, (0, 1)), 3: (2, (0, 2)), 4: (1, (0, 1)), 20: (3, (0,)), 64: (4, (0, 1)), 68: (8, (0, 2))}[C]
    keys, coords, tfield = R.random_case(C, T, scenes=scenes, s=s)
    assert len(tfield) == len(scenes) * (2 * T + 5)
    nbr, _ = R.interp_map(keys, s, tfield)
    present = (nbr >= 0).mean()
    assert present >= 0.25 and 1 - present >= 0.1, present
    _check_forward_backward(keys, s, tfield, C, C)


@pytest.mark.parametrize("C", [3, 64])
def test_backward_extremes_and_adjoint_identity(C):
    T = _tile()
    rng = np.random.default_rng(C)
    s = 2
    keys, coords = _filled_box(s, half=2, scenes=(0,))
    N = 3 * T + 7
    # every point in ONE cell: its eight sites have N pairs each (more than a tile), every other site has none
    tfield = np.concatenate((np.zeros((N, 1)), rng.random((N, 3)) * (s - 0.01) - s), 1).astype(np.float32)
    imap, nbr, w64, F, dy, y, dF = _check_forward_backward(keys, s, tfield, C, C)
    assert (nbr >= 0).all() and len(np.unique(nbr)) == 8
    count = np.bincount(nbr.reshape(-1), minlength=len(keys))
    assert sorted(count[count > 0].tolist()) == [N] * 8 and (count == 0).sum() == len(keys) - 8
    assert not _np(dF)[count == 0].any()
    # <interp(F), G> == <F, interp^T(G)> in float64, within what the two bounds allow
    lhs = (_np(y).astype(np.float64) * dy).sum()
    rhs = (F.astype(np.float64) * _np(dF).astype(np.float64)).sum()
    mass, cnt = R.backward_bound(dy, nbr, len(keys))
    allowed = (np.abs(dy) * 32 * EPS * R.forward_bound(F, nbr)).sum() + (np.abs(F) * (cnt[:, None] + 16) * EPS * mass).sum()
    print(f"interp adjoint: |lhs - rhs| / allowed = {abs(lhs - rhs) / allowed:.4f}")
    assert abs(lhs - rhs) <= allowed, (lhs, rhs, allowed)
    # the same identity on a scattered cloud
    keys, coords, tfield = R.random_case(C + 1, T, scenes=(0, 1), s=s)
    imap, nbr, w64, F, dy, y, dF = _check_forward_backward(keys, s, tfield, C, C + 1)
    lhs, rhs = (_np(y).astype(np.float64) * dy).sum(), (F.astype(np.float64) * _np(dF).astype(np.float64)).sum()
    mass, cnt = R.backward_bound(dy, nbr, len(keys))
    allowed = (np.abs(dy) * 32 * EPS * R.forward_bound(F, nbr)).sum() + (np.abs(F) * (cnt[:, None] + 16) * EPS * mass).sum()
    assert abs(lhs - rhs) <= allowed, (lhs, rhs, allowed)


@pytest.mark.parametrize("C", [5, 64])
def test_two_runs_give_the_same_bits_and_a_permutation_permutes_the_rows(C):
    from vdetr_amd import sparse_ops as S
    T = _tile()
    keys, coords, tfield = R.random_case(21, T, scenes=(0, 1, 2), s=2)
    g = torch.Generator().manual_seed(C)
    F, dy = torch.randn(len(keys), C, generator=g).to(DEV), torch.randn(len(tfield), C, generator=g).to(DEV)
    runs = []
    for _ in range(2):
        imap = S.interp_map(_dev(keys), 2, _dev(tfield))
        x = F.clone().requires_grad_(True)
        y = S.interpolate(x, imap)
        y.backward(dy)
        again = S.interpolate(x, imap)  # the same map, used twice
        x.grad = None
        again.backward(dy)
        runs.append((imap.nbr, imap.w, imap.order, imap.seg, y.detach(), again.detach(), x.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][4], runs[0][5])
    perm = torch.randperm(len(tfield), generator=g)
    moved = S.interpolate(F, S.interp_map(_dev(keys), 2, _dev(tfield[perm.numpy()])))
    assert torch.equal(moved, runs[0][4][perm.to(DEV)])
    # the segments: every site's pairs in ascending (n, k)
    order, seg, nbr = _np(runs[0][2]).astype(np.int64), _np(runs[0][3]), _np(runs[0][0]).reshape(-1)
    assert seg.shape == (len(keys) + 1,) and seg[-1] == 8 * len(tfield) and seg[0] == (nbr < 0).sum()
    want = np.argsort(nbr, kind="stable")
    assert np.array_equal(order, want) and np.array_equal(seg, np.searchsorted(nbr[want], np.arange(len(keys) + 1)))


def test_empty_tables_and_empty_fields():
    from vdetr_amd import sparse_ops as S
    keys, coords, tfield = R.random_case(3, 16, scenes=(0,), s=1)
    none = np.zeros(0, np.int64)
    for k, tf in ((none, tfield), (keys, tfield[:0]), (none, tfield[:0])):
        for C in (3, 8):
            x = torch.randn(len(k), C).to(DEV).requires_grad_(True)
            imap = S.interp_map(_dev(k), 2, _dev(tf))
            y = S.interpolate(x, imap)
            assert y.shape == (len(tf), C) and not y.any()  # M == 0: zeros are WRITTEN
            y.backward(torch.ones_like(y))
            assert x.grad.shape == (len(k), C) and not x.grad.any()
            assert imap.seg.shape == (len(k) + 1,) and imap.order.shape == (8 * len(tf),)
            assert _np(imap.seg).tolist() == [8 * len(tf)] * (len(k) + 1)  # (no site: every pair is absent; no point: no pair)


def test_map_forward_and_backward_read_nothing_back():
    from vdetr_amd import sparse_ops as S
    T = _tile()
    keys, coords, tfield = R.random_case(5, T, scenes=(0, 1), s=2)
    kd, td = _dev(keys), _dev(tfield)
    g = torch.Generator().manual_seed(0)
    F, dy = torch.randn(len(keys), 20, generator=g).to(DEV), torch.randn(len(tfield), 20, generator=g).to(DEV)

    def run():
        x = F.clone().requires_grad_(True)
        y = S.interpolate(x, S.interp_map(kd, 2, td))
        y.backward(dy)
        return y.detach(), x.grad

    want = run()  # (first call: libraries and allocator warm)
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            raises = False
        except RuntimeError:
            raises = True
        if raises:
            got = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raises:
        got = run()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if not raises:
        pytest.skip("this runtime ignores torch.cuda.set_sync_debug_mode: the no-host-read check did not run (parity did, and passed)")


# ---- the MinkowskiEngine-named API -------------------------------------------------------------------------------------------------
def _tensor(keys, s, F):
    """a SparseTensor at stride s on given sorted keys (rows in key order)"""
    from vdetr_amd import minkowski as ME
    cm = ME.CoordinateManager(torch.device(DEV))
    cm.keys[s] = _dev(keys)
    return ME.SparseTensor(F, tensor_stride=s, coordinate_manager=cm)


@pytest.mark.parametrize("kernel_map,weights", [(False, False), (True, False), (False, True), (True, True)])
def test_minkowski_interpolation_module(kernel_map, weights):
    from vdetr_amd import minkowski as ME
    keys, coords, tfield = R.random_case(9, 64, scenes=(0, 1), s=2)
    F = np.random.default_rng(1).standard_normal((len(keys), 12)).astype(np.float32)
    x = _tensor(keys, 2, _dev(F).requires_grad_(True))
    got = ME.MinkowskiInterpolation(return_kernel_map=kernel_map, return_weights=weights)(x, _dev(tfield))
    nbr, w64 = R.interp_map(keys, 2, tfield)
    in_map, out_map, wt = R.pairs(nbr, w64)
    if not (kernel_map or weights):
        assert torch.is_tensor(got)
        got = [got]
    assert isinstance(got, list) and len(got) == 1 + kernel_map + weights
    out = got[0]
    bound = 32 * EPS * R.forward_bound(F, nbr)
    assert out.shape == (len(tfield), 12) and (np.abs(_np(out).astype(np.float64) - R.forward(F, nbr, w64)) <= bound).all()
    if kernel_map:
        gi, go = got[1]
        assert gi.dtype == go.dtype == torch.int32 and np.array_equal(_np(gi), in_map) and np.array_equal(_np(go), out_map)
    if weights:
        gw = _np(got[-1])
        assert gw.dtype == np.float32 and gw.shape == wt.shape and np.abs(gw.astype(np.float64) - wt).max() <= 8 * EPS
        # out is the scatter of weights * F[in_map] over out_map
        scat = np.zeros((len(tfield), 12))
        np.add.at(scat, out_map, gw.astype(np.float64)[:, None] * F[in_map])
        assert (np.abs(_np(out).astype(np.float64) - scat) <= bound).all()
    out.sum().backward()
    assert np.abs(_np(x.F.grad).astype(np.float64) - R.backward(np.ones((len(tfield), 12)), nbr, w64, len(keys))).max() < 1e-3
    # the map is geometry: cached in the manager, and a geometry-only pass builds it without computing features
    td = _dev(tfield)
    y1 = x.features_at_coordinates(td)
    cache = x.coordinate_manager._interp_maps
    n_maps = len(cache)
    y2 = ME.MinkowskiInterpolation()(x, td)
    assert len(cache) == n_maps and torch.equal(y1, y2) and torch.equal(y1, out)
    fresh = _tensor(keys, 2, _dev(F))
    with ME.geometry_only():
        blank = ME.MinkowskiInterpolation()(fresh, td)
    assert blank.shape == out.shape and len(fresh.coordinate_manager._interp_maps) == 1
    (imap, _, _), = fresh.coordinate_manager._interp_maps.values()
    assert torch.equal(ME.MinkowskiInterpolation()(fresh, td), out) and len(fresh.coordinate_manager._interp_maps) == 1
    assert np.array_equal(_np(imap.nbr), nbr)


def test_interpolate_a_strided_tensor_on_its_field_cat_slice_and_slice():
    from vdetr_amd import minkowski as ME
    rng = np.random.default_rng(4)
    n = 700
    pts = np.concatenate((rng.integers(0, 2, (n, 1)).astype(np.float64), rng.random((n, 3)) * 22 - 9), 1).astype(np.float32)
    feats = rng.standard_normal((n, 4)).astype(np.float32)
    f = _dev(feats).requires_grad_(True)
    field = ME.TensorField(f, _dev(pts))
    # .C and slice of a float-coordinate field are what they were
    assert field.C.dtype == torch.int32 and np.array_equal(_np(field.C), np.floor(pts).astype(np.int32))
    assert field.float_coordinates.dtype == torch.float32 and np.array_equal(_np(field.float_coordinates), pts)
    sp = field.sparse()
    back = sp.slice(field)
    assert isinstance(back, ME.TensorField) and torch.equal(back.F, sp.F[field.inverse_mapping.long()]) and back.C is field.C
    # cat_slice: the site features first, then the field's own
    cat = sp.cat_slice(field)
    assert isinstance(cat, ME.TensorField) and cat.C is field.C and cat.F.shape == (n, 8)
    assert torch.equal(cat.F[:, :4], back.F) and torch.equal(cat.F[:, 4:], field.F)
    torch.manual_seed(0)
    conv1 = ME.MinkowskiConvolution(4, 8, kernel_size=2, stride=2, dimension=3).to(DEV)
    conv2 = ME.MinkowskiConvolution(8, 6, kernel_size=2, stride=2, dimension=3).to(DEV)
    deep = conv2(conv1(sp))
    assert deep.tensor_stride == 4
    for bad, text in ((ME.TensorField(_dev(feats), _dev(pts)), "whose sparse"), (field.F, "a TensorField is expected")):
        for call in (sp.slice, sp.cat_slice):
            with pytest.raises(ValueError, match=text):
                call(bad)
    for call in (deep.slice, deep.cat_slice):
        with pytest.raises(ValueError, match="tensor stride 1"):
            call(field)
    # the stride-4 tensor read at the raw points, against the restatement on its keys and features
    out = deep.interpolate(field)
    assert isinstance(out, ME.TensorField) and out.C is field.C and out.F.shape == (n, 6)
    keys, F4 = _np(deep.keys), _np(deep.F)
    nbr, w64 = R.interp_map(keys, 4, pts)
    assert (nbr >= 0).mean() > 0.25
    assert (np.abs(_np(out.F).astype(np.float64) - R.forward(F4, nbr, w64)) <= 32 * EPS * R.forward_bound(F4, nbr)).all()
    assert torch.equal(out.F, deep.features_at_coordinates(field.float_coordinates))
    out.F.square().sum().backward()
    for p in (conv1.kernel, conv2.kernel, f):
        assert torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0
    # another manager's field, and integer coordinates, which interpolate at themselves
    other = ME.TensorField(_dev(feats[:50]), _dev(pts[:50]))
    assert torch.equal(deep.interpolate(other).F, out.F[:50])
    sites = ME.TensorField(sp.F.detach(), sp.C)
    assert sites.float_coordinates.dtype == torch.float32 and torch.equal(sp.interpolate(sites).F, sp.F.detach())
