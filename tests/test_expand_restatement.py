"""tests/expand_restatement.py pinned to the definition it restates: on small clouds the expanded set equals the brute
force over every lattice site of the grown bounding box whose row of the neighbour table is not empty; the transposed case equals
``CoordinateManager.generated`` on CPU key tensors; the order of a coordinate list is that of its keys.  No GPU needed."""
import itertools

import numpy as np
import pytest
import torch

import expand_restatement as E
import sparse_modules_restatement as R
from oracle import sparse_oracle as O


def _cloud(ts, seed=3):
    sites = R.cloud(200, seed, batch=2, extent=4, ts=ts)
    assert 100 < len(sites) <= 200 and set(sites[:, 0]) == {0, 1} and int(sites[:, 1:].min()) < 0
    return sites


def _brute_force(in_sites, offsets, ts, out_ts, transposed):
    reach = E.reach(offsets, ts, out_ts, transposed)
    grow = max(abs(v) for r in reach for v in r)
    lo, hi = in_sites[:, 1:].min(0) - grow, in_sites[:, 1:].max(0) + grow
    axes = [range(int(np.floor_divide(a, out_ts)) * out_ts, int(b) + 1, out_ts) for a, b in zip(lo, hi)]
    box = np.array([(b,) + p for b in sorted(set(in_sites[:, 0])) for p in itertools.product(*axes)], dtype=np.int64)
    nbr = R.neighbour_table(in_sites, box, reach).numpy()
    return R.sort_sites(box[(nbr >= 0).any(0)])


@pytest.mark.parametrize("out_ts", [1, 2])
@pytest.mark.parametrize("region", list(E.REGIONS))
def test_expanded_sites_are_the_sites_with_a_neighbour(region, out_ts):
    offsets, transposed, _ = E.REGIONS[region]
    ts, out_ts = E.strides(region, out_ts)
    sites = _cloud(ts)
    got = E.expanded_sites(sites, offsets, ts, out_ts, transposed)
    ref = _brute_force(sites, offsets, ts, out_ts, transposed)
    assert np.array_equal(got, ref)
    assert len(got) > len(sites) or region == "custom-x"
    if region == "custom-x":  # the single offset (1, 0, 0): the output site that READS v through it lies at v - ts
        assert np.array_equal(got, R.sort_sites(sites - np.array([0, ts, 0, 0])))
    if region == "cube2":
        wrong = np.unique(E.candidates(sites, [tuple(-v for v in o) for o in offsets], ts, out_ts, transposed), axis=0)
        assert not np.array_equal(wrong, ref), "the cloud tells the two signs apart"


@pytest.mark.parametrize("out_ts", [1, 2])
@pytest.mark.parametrize("region", [r for r in E.REGIONS if E.REGIONS[r][1]])
def test_transposed_sites_are_the_generated_ones(region, out_ts):
    from vdetr_amd import minkowski as ME
    offsets, transposed, _ = E.REGIONS[region]
    ts, out_ts = E.strides(region, out_ts)
    sites = _cloud(ts, seed=5)
    keys = torch.from_numpy(O.pack_keys_np(sites))
    gen = ME.CoordinateManager("cpu").generated(keys, out_ts, tuple(offsets))
    got = E.expanded_sites(sites, offsets, ts, out_ts, transposed)
    assert np.array_equal(O.pack_keys_np(got), gen.numpy())


def test_target_sites_are_in_key_order_with_their_inverse():
    rng = np.random.default_rng(0)
    coords = np.concatenate((rng.integers(0, 3, (300, 1)), rng.integers(-5, 5, (300, 3))), 1)
    coords = np.concatenate((coords, coords[:40]))  # duplicates
    sites, inverse = E.target_sites(coords)
    keys = O.pack_keys_np(sites)
    assert bool((np.diff(keys) > 0).all()) and len(sites) < len(coords)
    assert np.array_equal(sites[inverse], coords) and inverse.shape == (340,)
    assert set(map(tuple, sites)) == set(map(tuple, coords))
    empty, inv = E.target_sites(np.zeros((0, 4)))
    assert empty.shape == (0, 4) and inv.shape == (0,)


def test_the_keyword_and_what_is_not_built():
    from vdetr_amd import minkowski as ME
    for cls, args in ((ME.MinkowskiConvolution, (4, 4, 3)), (ME.MinkowskiChannelwiseConvolution, (4, 3)), (ME.MinkowskiSumPooling, (3,)),
                      (ME.MinkowskiAvgPooling, (3,)), (ME.MinkowskiMaxPooling, (3,))):
        assert cls(*args, expand_coordinates=True).expand_coordinates is True
        assert cls(*args).expand_coordinates is False and cls(*args, stride=2).expand_coordinates is False
        with pytest.raises(NotImplementedError, match="expand_coordinates=True with stride 2"):
            cls(*args, stride=2, expand_coordinates=True)
    for cls, args in ((ME.MinkowskiConvolutionTranspose, (4, 4, 2)), (ME.MinkowskiPoolingTranspose, (2,)), (ME.MinkowskiAvgUnpooling, (2,))):
        layer = cls(*args, stride=2, expand_coordinates=True)
        assert layer.expand_coordinates is True and layer.kernel_generator.expand_coordinates is True
