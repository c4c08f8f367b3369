"""tests/voxelize_restatement.py against a dictionary loop on small random inputs: the maps, the four quantisation modes with
their winners and gradients, the label rule and the key arithmetic.  No GPU needed."""
import numpy as np
import pytest

import voxelize_restatement as R


def _case(seed, n, span=3, scenes=2, c=3):
    rng = np.random.default_rng(seed)
    coords = np.concatenate((rng.integers(0, scenes, (n, 1)), rng.integers(-span, span, (n, 3))), 1)
    feats = rng.standard_normal((n, c)).astype(np.float32)
    return coords, feats


def _loop_maps(keys):
    rows = {}
    for i, k in enumerate(keys.tolist()):
        rows.setdefault(k, []).append(i)
    sites = sorted(rows)
    row_of = {k: r for r, k in enumerate(sites)}
    inverse = [row_of[k] for k in keys.tolist()]
    first = [rows[k][0] for k in sites]
    seg, order = [0], []
    for k in sites:
        order += rows[k]
        seg.append(len(order))
    return sites, inverse, first, seg, order, [rows[k] for k in sites]


@pytest.mark.parametrize("seed,n", [(0, 0), (1, 1), (2, 40), (3, 300)])
def test_maps_equal_a_dictionary_loop(seed, n):
    coords, _ = _case(seed, n)
    keys = R.pack_keys(coords)
    sites, inverse, first, seg, order = R.voxel_maps(keys)
    want = _loop_maps(keys)
    assert sites.tolist() == want[0] and inverse.tolist() == want[1] and first.tolist() == want[2]
    assert seg.tolist() == want[3] and order.tolist() == want[4]
    assert sites.dtype == np.int64 and inverse.dtype == np.int32 and first.dtype == np.int64 and seg.dtype == np.int32


@pytest.mark.parametrize("mode", ["first", "sum", "average", "max"])
def test_modes_and_gradients_equal_a_sequential_loop(mode):
    coords, feats = _case(7, 200, c=5)
    feats[17, 2] = np.nan
    feats[40] = feats[41]  # (rows 40 and 41 tie wherever they share a voxel)
    coords[41] = coords[40]
    keys = R.pack_keys(coords)
    _, inverse, _, _, _ = R.voxel_maps(keys)
    rows = _loop_maps(keys)[5]
    m = len(rows)
    got, winners = R.reduce_features(feats, inverse, m, mode)
    want = np.zeros((m, 5), np.float32)
    win = np.zeros((m, 5), np.int32)
    for r, members in enumerate(rows):
        for ch in range(5):
            if mode == "first":
                want[r, ch] = feats[members[0], ch]
            elif mode == "max":
                best, who = feats[members[0], ch], members[0]
                for i in members[1:]:
                    v = feats[i, ch]
                    if v > best or (np.isnan(v) and not np.isnan(best)):
                        best, who = v, i
                want[r, ch], win[r, ch] = best, who
            else:
                acc = np.float32(0)
                for i in members:
                    acc = np.float32(acc + feats[i, ch])
                want[r, ch] = acc / np.float32(len(members)) if mode == "average" else acc
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
    if mode == "max":
        assert np.array_equal(winners, win)
    d = np.random.default_rng(8).standard_normal((m, 5)).astype(np.float32)
    grad = R.reduce_grad(d, inverse, m, mode, winners)
    want_g = np.zeros((200, 5), np.float32)
    for r, members in enumerate(rows):
        for i in members:
            for ch in range(5):
                if mode == "sum":
                    want_g[i, ch] = d[r, ch]
                elif mode == "average":
                    want_g[i, ch] = d[r, ch] / np.float32(len(members))
                elif mode == "max":
                    want_g[i, ch] = d[r, ch] if win[r, ch] == i else 0
                else:
                    want_g[i, ch] = d[r, ch] if members[0] == i else 0
    assert grad.dtype == np.float32 and np.array_equal(grad, want_g)


def test_slice_gradient_and_labels():
    coords, feats = _case(9, 150)
    keys = R.pack_keys(coords)
    _, inverse, _, _, _ = R.voxel_maps(keys)
    rows = _loop_maps(keys)[5]
    got = R.slice_grad(feats, inverse, len(rows))
    for r, members in enumerate(rows):
        acc = np.zeros(3, np.float32)
        for i in members:
            acc = (acc + feats[i]).astype(np.float32)
        assert np.array_equal(got[r], acc)
    labels = np.random.default_rng(10).integers(0, 2, 150)
    lab = R.site_labels(labels, inverse, len(rows), ignore_label=-7)
    want = [labels[m[0]] if len({int(labels[i]) for i in m}) == 1 else -7 for m in rows]
    assert lab.tolist() == want and -7 in want and any(len(m) > 1 and w != -7 for m, w in zip(rows, want))


def test_key_arithmetic_is_a_float32_reciprocal_product():
    pts = np.array([[0.03, -0.0, 0.07], [-0.01, 0.29, 1.0]], np.float32)
    inv = np.float32(1.0 / 0.03)
    assert inv != np.float32(1.0) / np.float32(0.03)  # (the reciprocal is taken in double: at 0.03 the two differ)
    assert np.array_equal(R.voxel_indices(pts, 0.03), np.floor(pts * inv))
    assert R.voxel_indices(pts, 0.01).dtype == np.float32
    coords = R.cloud_coords(pts, [0, 1, 1, 2], 0.01)
    assert coords[:, 0].tolist() == [0, 2]  # (the middle scene is empty)
    with pytest.raises(ValueError, match="16-bit key range"):
        R.cloud_coords(np.array([[np.nan, 0, 0]], np.float32), [0, 1], 0.01)
    for bad in ([0, 32768, 0, 0], [0, 0, -32769, 0], [-1, 0, 0, 0], [32768, 0, 0, 0]):
        with pytest.raises(ValueError, match="16-bit key range"):
            R.pack_keys(np.array([bad]))
    assert R.pack_keys(np.array([[32767, 32767, -32768, 0]])).tolist() == [(32767 << 48) | (65535 << 32) | 32768]
