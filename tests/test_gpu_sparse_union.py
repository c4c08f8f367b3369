"""csrc/sparse_union.hip on the GPU against tests/sparse_union_restatement.py: the union map and the prune map word for word
(np.union1d / np.searchsorted / np.nonzero), the union add and the row gather bit for bit (one fp32 add of two given floats; copies),
their gradients, and what the entry points refuse."""
import numpy as np
import pytest
import torch

import sparse_union_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (0, 1, 63, 64, 65, 257, 5000)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w), (g.shape, w.shape)


@pytest.mark.parametrize("relation", R.RELATIONS)
def test_union_map_equals_numpy(relation):
    from vdetr_amd import sparse_ops as S
    tile = S.union_tile()
    pairs = [(na, nb) for na in SIZES for nb in SIZES] + [(tile, tile), (tile, tile + 1), (tile + 1, tile), (2 * tile, 65)]
    for na, nb in pairs:
        a, b = R.key_sets(relation, na, nb)
        got = S.union_map(a.to(DEV), b.to(DEV))
        _same(got, R.union_map(a, b))


def test_union_map_with_a_shared_run_across_a_tile_boundary():
    """a run of keys that both sets hold lies across a multiple of the kernel's tile in each of them: the match counts of two
    tiles per side take part in every row behind it"""
    from vdetr_amd import sparse_ops as S
    tile = S.union_tile()
    for run in (2, 9):
        a, b = R.run_across_boundary(tile, run)
        first_a, first_b = int(torch.searchsorted(a, b[2 * tile - run // 2])), 2 * tile - run // 2
        assert first_a < tile < first_a + run and first_b < 2 * tile < first_b + run and torch.equal(a[first_a:first_a + run], b[first_b:first_b + run])
        for x, y in ((a, b), (b, a)):
            _same(S.union_map(x.to(DEV), y.to(DEV)), R.union_map(x, y))


def _operands(C, na=257, nb=5000, relation="interleaved"):
    a, b = R.key_sets(relation, na, nb, seed=C)
    g = torch.Generator().manual_seed(C)
    return a, b, torch.randn(a.shape[0], C, generator=g), torch.randn(b.shape[0], C, generator=g)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("C", [4, 20, 64, 256])
def test_union_add_forward_and_backward(C, sign):
    from vdetr_amd import sparse_ops as S
    a, b, fa, fb = _operands(C)
    with torch.no_grad():  # an infinity on a row the other side lacks, on either side
        ref_map = R.union_map(a, b)
        only_a = int(torch.nonzero(ref_map[4][ref_map[1].long()] < 0)[0])
        only_b = int(torch.nonzero(ref_map[3][ref_map[2].long()] < 0)[0])
        fa[only_a, 1], fb[only_b, 2] = float("inf"), float("inf")
    maps = S.union_map(a.to(DEV), b.to(DEV))
    _same(maps, ref_map)
    dy = torch.randn(ref_map[0].shape[0], C, generator=torch.Generator().manual_seed(1))
    for grad_a, grad_b in ((True, False), (False, True), (True, True)):
        xa, xb = fa.clone().requires_grad_(grad_a), fb.clone().requires_grad_(grad_b)
        want = R.union_add(xa, xb, *ref_map[1:], sign=sign)
        want.backward(dy)
        ga, gb = fa.to(DEV).requires_grad_(grad_a), fb.to(DEV).requires_grad_(grad_b)
        got = S.union_add(ga, gb, *maps[1:], sign=sign)
        again = S.union_add(ga, gb, *maps[1:], sign=sign)
        got.backward(dy.to(DEV))
        assert torch.equal(got.detach().cpu(), want.detach()) and torch.equal(got, again)
        assert not bool(torch.isnan(got).any())
        out = got.detach()
        assert float(out[int(ref_map[1][only_a]), 1]) == float("inf") and float(out[int(ref_map[2][only_b]), 2]) == sign * float("inf")
        for g, w, needed in ((ga.grad, xa.grad, grad_a), (gb.grad, xb.grad, grad_b)):
            assert (g is None and w is None) if not needed else torch.equal(g.cpu(), w)
    assert torch.equal(ga.grad.cpu(), dy[ref_map[1].long()]) and torch.equal(gb.grad.cpu(), sign * dy[ref_map[2].long()])


def test_union_add_with_an_empty_side():
    from vdetr_amd import sparse_ops as S
    a, b, fa, fb = _operands(8, na=0, nb=65)
    for x, y, fx, fy in ((a, b, fa, fb), (b, a, fb, fa)):
        for sign in (1, -1):
            maps, ref_map = S.union_map(x.to(DEV), y.to(DEV)), R.union_map(x, y)
            got = S.union_add(fx.to(DEV), fy.to(DEV), *maps[1:], sign=sign)
            assert torch.equal(got.cpu(), R.union_add(fx, fy, *ref_map[1:], sign=sign))


def _pruned(n, kind, C=8):
    from vdetr_amd import minkowski as ME
    counts = R.scene_split(n)
    keys = R.scene_keys(counts, seed=n)
    mask = R.mask_of(kind, counts)
    cm = ME.CoordinateManager(torch.device(DEV))
    cm.keys[1] = keys.to(DEV)
    cm.num_scenes = len(counts)
    f = torch.randn(n, C, generator=torch.Generator().manual_seed(n))
    x = ME.SparseTensor(f.to(DEV).requires_grad_(True), tensor_stride=1, coordinate_manager=cm)
    return x, f, keys, mask, counts


@pytest.mark.parametrize("kind", R.MASKS)
@pytest.mark.parametrize("n", [1, 64, 65, 1025, 5000])
def test_prune_map_and_pruning(n, kind):
    from vdetr_amd import minkowski as ME
    from vdetr_amd import sparse_ops as S
    if n < 3 and kind.endswith("_scene"):
        kind = "all" if kind == "no_middle_scene" else "none"  # (one row is one scene: keeping it or not is all there is)
    x, f, keys, mask, counts = _pruned(n, kind)
    _same(S.prune_map(mask.to(DEV), x.keys), R.prune_map(mask, keys))
    y = ME.MinkowskiPruning()(x, mask.to(DEV))
    assert y.tensor_stride == 1 and y.coordinate_manager is x.coordinate_manager
    assert torch.equal(y.keys.cpu(), keys[mask]) and torch.equal(y.F.detach().cpu(), f[mask])
    parts = y.decomposed()
    kept_per_scene = [int(m.sum()) for m in torch.split(mask, counts)]
    assert [p[1].shape[0] for p in parts] == kept_per_scene and [p[0].shape for p in parts] == [(k, 3) for k in kept_per_scene]
    if kind.endswith("_scene"):
        assert len(parts) == 3 and kept_per_scene[1 if kind == "no_middle_scene" else 2] == 0
    dy = torch.randn(int(mask.sum()), f.shape[1], generator=torch.Generator().manual_seed(2))
    y.F.backward(dy.to(DEV))
    grad = x.F.grad.cpu()
    want = torch.zeros_like(f)
    want[mask] = dy
    assert torch.equal(grad, want)
    assert bool((grad[~mask] == 0).all()) and not bool(torch.signbit(grad[~mask]).any())  # exact zeros, no sign bit


def test_take_rows_negates_and_zeroes():
    from vdetr_amd import sparse_ops as S
    x = torch.randn(300, 20, generator=torch.Generator().manual_seed(3))
    idx = torch.full((700,), -1, dtype=torch.int32)
    perm = torch.randperm(700, generator=torch.Generator().manual_seed(4))[:300]
    idx[perm] = torch.arange(300, dtype=torch.int32)
    for sign in (1, -1):
        got = S.take_rows(x.to(DEV), idx.to(DEV), sign=sign)
        assert torch.equal(got.cpu(), R.take_rows(x, idx, sign=sign))
        assert not bool(torch.signbit(got[idx.to(DEV) < 0]).any())


def _tensor(keys, C, stride=1, cm=None):
    from vdetr_amd import minkowski as ME
    if cm is None:
        cm = ME.CoordinateManager(torch.device(DEV))
        cm.num_scenes = 1
    return ME.SparseTensor(torch.randn(keys.shape[0], C, device=DEV), tensor_stride=stride, coordinate_manager=cm, keys=keys.to(DEV))


def test_refusals():
    from vdetr_amd import minkowski as ME
    from vdetr_amd import sparse_ops as S
    a, b, fa, fb = _operands(8, na=64, nb=65)
    maps = S.union_map(a.to(DEV), b.to(DEV))
    da, db = fa.to(DEV), fb.to(DEV)
    ref_map = R.union_map(a, b)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        S.union_map(a, b)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        S.union_add(fa, fb, *ref_map[1:])
    with pytest.raises(RuntimeError, match="CPU not supported"):
        S.prune_map(torch.ones(64, dtype=torch.bool), a)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        S.take_rows(fa, ref_map[1])
    with pytest.raises(RuntimeError, match="int64"):
        S.union_map(a.to(DEV).int(), b.to(DEV))
    with pytest.raises(RuntimeError, match="float tensor"):
        S.union_add(da.double(), db.double(), *maps[1:])
    with pytest.raises(RuntimeError, match="float tensor"):
        S.take_rows(da.double(), maps[1])
    with pytest.raises(RuntimeError, match="contiguous"):
        S.union_add(torch.randn(8, 64, device=DEV).t(), db, *maps[1:])
    with pytest.raises(RuntimeError, match="contiguous"):
        S.take_rows(torch.randn(8, 64, device=DEV).t(), maps[1])
    with pytest.raises(RuntimeError, match="C=6"):
        S.union_add(torch.randn(64, 6, device=DEV), torch.randn(65, 6, device=DEV), *maps[1:])
    with pytest.raises(RuntimeError, match="C=6"):
        S.take_rows(torch.randn(64, 6, device=DEV), maps[1])
    with pytest.raises(ValueError, match="8 and 12 channels"):
        S.union_add(da, torch.randn(65, 12, device=DEV), *maps[1:])
    with pytest.raises(RuntimeError, match="row_a"):
        S.union_add(da[:60].contiguous(), db, *maps[1:])
    with pytest.raises(RuntimeError, match="`back`"):
        S.take_rows(da.clone().requires_grad_(True), maps[1])
    with pytest.raises(RuntimeError, match="bool"):
        S.prune_map(torch.ones(64, dtype=torch.uint8, device=DEV), a.to(DEV))
    with pytest.raises(RuntimeError, match="one entry per row"):
        S.prune_map(torch.ones(63, dtype=torch.bool, device=DEV), a.to(DEV))
    x = _tensor(a, 8)
    for bad, text in ((torch.ones(63, dtype=torch.bool, device=DEV), "mask of shape"), (torch.ones(64, dtype=torch.uint8, device=DEV), "bool"),
                      (torch.ones(64, dtype=torch.bool), "the mask is on")):
        with pytest.raises(ValueError, match=text):
            ME.MinkowskiPruning()(x, bad)
    with pytest.raises(ValueError, match="tensor strides: 1 and 2"):
        x + _tensor(b, 8, stride=2, cm=x.coordinate_manager)
    with pytest.raises(ValueError, match="channel counts: 8 and 12"):
        x - _tensor(b, 12, cm=x.coordinate_manager)
    with pytest.raises(ValueError, match="coordinate managers"):
        x + _tensor(b, 8)
    y = x + _tensor(b, 8, cm=x.coordinate_manager)  # what fits is taken
    assert torch.equal(y.keys.cpu(), ref_map[0])
