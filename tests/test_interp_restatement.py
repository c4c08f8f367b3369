"""tests/interp_restatement.py against brute-force dictionary look-ups on tiny inputs: the corners and weights of the definition in
DESIGN 6.16, floor_div below zero, the edge of the 16-bit field, and the occupancy of the random case the GPU test uses."""
import math
from fractions import Fraction

import numpy as np
import pytest

import interp_restatement as R


def _brute(sites, s, tfield, F=None):
    """a dictionary of sites and Python's own integer / rational arithmetic: per point the list of (k, site row, weight)"""
    table = {tuple(int(v) for v in c): r for r, c in enumerate(sites)}
    out = []
    for b, *xyz in np.asarray(tfield, dtype=np.float32).tolist():
        found = []
        ok = all(math.isfinite(v) for v in (b, *xyz)) and b == int(b) and 0 <= b <= 32767 and all(-32768 <= math.floor(v) <= 32767 for v in xyz)
        if ok:
            lo = [(math.floor(v) // s) * s for v in xyz]  # (Python's // rounds towards minus infinity)
            t = [(Fraction(v) - l) / s for v, l in zip(xyz, lo)]
            for k in range(8):
                bits = ((k >> 2) & 1, (k >> 1) & 1, k & 1)
                c = tuple(l + bit * s for l, bit in zip(lo, bits))
                if (int(b),) + c in table and all(-32768 <= v <= 32767 for v in c):
                    wt = Fraction(1)
                    for bit, tt in zip(bits, t):
                        wt *= tt if bit else 1 - tt
                    found.append((k, table[(int(b),) + c], wt))
        out.append(found)
    return out


def _sorted_sites(coords):
    coords = np.asarray(coords, dtype=np.int64)
    keys = R.pack_keys(coords)
    order = np.argsort(keys)
    return keys[order], coords[order]


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_map_and_weights_against_the_dictionary(s):
    rng = np.random.default_rng(s)
    grid = np.stack(np.meshgrid(*(np.arange(-3, 3),) * 3, indexing="ij"), -1).reshape(-1, 3) * s
    coords = np.concatenate([np.concatenate((np.full((len(g), 1), b), g), 1) for b in (0, 2)
                             for g in (grid[rng.random(len(grid)) < 0.6],)])
    keys, coords = _sorted_sites(coords)
    pts = (rng.random((60, 3)) * 7 - 3.5) * s
    tfield = np.concatenate((rng.choice([0.0, 1.0, 2.0], (60, 1)), pts), 1).astype(np.float32)  # (scene 1 has no site)
    tfield[:6, 1:] = np.round(tfield[:6, 1:] / s) * s  # points exactly on lattice positions
    nbr, w = R.interp_map(keys, s, tfield)
    assert nbr.dtype == np.int32 and nbr.shape == (60, 8) and w.shape == (60, 8)
    want = _brute(coords, s, tfield)
    for n, found in enumerate(want):
        exp_nbr, exp_w = np.full(8, -1), np.zeros(8)
        for k, r, wt in found:
            exp_nbr[k], exp_w[k] = r, float(wt)
        assert np.array_equal(nbr[n], exp_nbr), (n, tfield[n])
        assert np.allclose(w[n], exp_w, rtol=1e-14, atol=0), (n, tfield[n])
    assert not (nbr[tfield[:, 0] == 1.0] >= 0).any()
    # forward / backward and the compacted pair lists against the same dictionary
    F = rng.standard_normal((len(keys), 3))
    dy = rng.standard_normal((60, 3))
    out, dF = np.zeros((60, 3)), np.zeros((len(keys), 3))
    flat = []
    for n, found in enumerate(want):
        for k, r, wt in found:
            out[n] += float(wt) * F[r]
            dF[r] += float(wt) * dy[n]
            flat.append((r, n))
    assert np.allclose(R.forward(F, nbr, w), out, rtol=1e-12, atol=1e-14)
    assert np.allclose(R.backward(dy, nbr, w, len(keys)), dF, rtol=1e-12, atol=1e-14)
    in_map, out_map, wt = R.pairs(nbr, w)
    assert in_map.dtype == out_map.dtype == np.int32 and [(int(a), int(b)) for a, b in zip(in_map, out_map)] == flat
    assert np.array_equal(wt, w[nbr >= 0])


def test_interior_weights_sum_to_one_and_lattice_points_read_their_site():
    s = 2
    grid = np.stack(np.meshgrid(*(np.arange(-2, 3),) * 3, indexing="ij"), -1).reshape(-1, 3) * s
    keys, coords = _sorted_sites(np.concatenate((np.zeros((len(grid), 1), np.int64), grid), 1))
    rng = np.random.default_rng(0)
    tfield = np.concatenate((np.zeros((40, 1)), rng.random((40, 3)) * 7.9 - 3.95), 1).astype(np.float32)
    nbr, w = R.interp_map(keys, s, tfield)
    assert (nbr >= 0).all() and np.allclose(w.sum(1), 1.0, rtol=0, atol=1e-15) and (w >= 0).all()
    on = np.concatenate((np.zeros((len(coords), 1)), coords[:, 1:]), 1).astype(np.float32)
    nbr, w = R.interp_map(keys, s, on)
    assert np.array_equal(nbr[:, 0], np.arange(len(keys))) and np.array_equal(w[:, 0], np.ones(len(keys))) and not w[:, 1:].any()
    F = rng.standard_normal((len(keys), 2))
    assert np.array_equal(R.forward(F, nbr, w), F)


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_floor_div_below_zero(s):
    i = np.arange(-40, 41)
    assert R.floor_div(i, s).tolist() == [v // s for v in i.tolist()] == [math.floor(v / s) for v in i.tolist()]
    assert R.floor_div(np.array([-32768, -1, 0, 32767]), s).tolist() == [(-32768) // s, -1, 0, 32767 // s]
    # a point just below zero reads the cell that ENDS at zero: lower site -s, weight of the upper site close to 1
    keys, _ = _sorted_sites([[0, -s, 0, 0], [0, 0, 0, 0]])
    nbr, w = R.interp_map(keys, s, np.array([[0, -0.25, 0, 0]], np.float32))
    assert nbr[0].tolist() == [0, -1, -1, -1, 1, -1, -1, -1]
    assert w[0, 0] == pytest.approx(0.25 / s, rel=1e-14) and w[0, 4] == pytest.approx(1 - 0.25 / s, rel=1e-14)


def test_field_edge_and_rows_without_corners():
    # a site at 32767 and a decoy on the key that a carry out of the z field would land on: (x, y + 1, z = -32768)
    coords = [[0, 5, 5, 32767], [0, 5, 6, -32768], [0, 32767, 0, 0], [1, -32768, 0, 0]]
    keys, coords = _sorted_sites(coords)
    at = {tuple(c): r for r, c in enumerate(coords.tolist())}
    tfield = np.array([[0, 5, 5, 32767.5], [0, 32767.5, 0, 0], [1, -32768.5, 0, 0], [0, np.nan, 0, 0], [0, 0, np.inf, 0],
                       [0, 0, 0, -np.inf], [0.5, 5, 5, 5], [-1, 5, 5, 5], [32768, 5, 5, 5], [np.nan, 5, 5, 5], [0, 40000, 0, 0]], np.float32)
    nbr, w = R.interp_map(keys, 1, tfield)
    assert nbr[0].tolist() == [at[(0, 5, 5, 32767)]] + [-1] * 7 and w[0, 0] == 0.5 and not w[0, 1:].any()
    assert nbr[1].tolist() == [at[(0, 32767, 0, 0)]] + [-1] * 7
    assert not (nbr[2:] >= 0).any() and not w[2:].any()
    # stride 3: the lower site of -32768 would be -32769: absent, the upper one (-32766) is read
    keys3, _ = _sorted_sites([[0, -32766, 0, 0]])
    nbr, w = R.interp_map(keys3, 3, np.array([[0, -32768, 0, 0]], np.float32))
    assert nbr[0].tolist() == [-1, -1, -1, -1, 0, -1, -1, -1] and w[0, 4] == pytest.approx(1 / 3, rel=1e-15)
    # no sites at all
    nbr, w = R.interp_map(np.zeros(0, np.int64), 2, tfield)
    assert not (nbr >= 0).any() and not w.any() and not R.forward(np.zeros((0, 3)), nbr, w).any()


@pytest.mark.parametrize("s,scenes", [(1, (0, 1)), (2, (0, 2)), (4, (0,))])
def test_the_random_case_is_neither_full_nor_empty(s, scenes):
    keys, coords, tfield = R.random_case(7, 16, scenes=scenes, s=s)
    assert np.array_equal(keys, np.unique(keys)) and np.array_equal(R.pack_keys(coords), keys)
    assert (coords[:, 1:] % s == 0).all() and coords[:, 1:].min() < 0 < coords[:, 1:].max()
    assert tfield.dtype == np.float32 and tfield.shape == (len(scenes) * 37, 4)
    nbr, _ = R.interp_map(keys, s, tfield)
    present = (nbr >= 0).mean()
    assert present >= 0.25 and 1 - present >= 0.1, present
