"""A numpy restatement of the trilinear interpolation (csrc/sparse_interp.hip): the map in integers, the weights, the
forward and the backward in float64, all from the same float32 inputs; pair lists compacted.  It shares no code with the package;
tests/test_interp_restatement.py checks it against dictionary look-ups."""
import numpy as np

KEY_BIAS = 32768


def pack_keys(coords):
    """[M, 4] integer (batch, x, y, z) inside the 16-bit fields -> int64 keys"""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    assert not c.size or (c[:, 1:].min() >= -KEY_BIAS and c[:, 1:].max() < KEY_BIAS and c[:, 0].min() >= 0 and c[:, 0].max() < 32768)
    return (c[:, 0] << 48) | ((c[:, 1] + KEY_BIAS) << 32) | ((c[:, 2] + KEY_BIAS) << 16) | (c[:, 3] + KEY_BIAS)


def floor_div(i, s):
    """towards minus infinity, in integers (written out: no reliance on the language's // for negative operands)"""
    i = np.asarray(i, dtype=np.int64)
    q = np.abs(i) // s
    return np.where(i >= 0, q, -q - (np.abs(i) % s != 0))


def interp_map(keys, s, tfield):
    """keys [M] int64 ascending unique, s >= 1, tfield [N, 4] float32 -> (nbr [N, 8] int32, w [N, 8] float64).  Corner
    k = 4 bx + 2 by + bz, bit 1 = the upper site lo + s; w = fx fy fz, 0 where nbr = -1."""
    keys = np.asarray(keys, dtype=np.int64)
    tf = np.asarray(tfield, dtype=np.float32).reshape(-1, 4)
    n = tf.shape[0]
    nbr = np.full((n, 8), -1, np.int32)
    w = np.zeros((n, 8), np.float64)
    with np.errstate(invalid="ignore"):
        fl = np.floor(tf)
        row = np.isfinite(tf).all(1) & (fl[:, 1:] >= -32768).all(1) & (fl[:, 1:] <= 32767).all(1)
        row &= (tf[:, 0] == fl[:, 0]) & (tf[:, 0] >= 0) & (tf[:, 0] <= 32767)
    for i in np.nonzero(row)[0]:
        b = int(tf[i, 0])
        lo = floor_div(fl[i, 1:].astype(np.int64), s) * s                     # [3] integers
        t = (tf[i, 1:].astype(np.float64) - lo.astype(np.float64)) / float(s)  # exact subtraction, one float64 division
        for k in range(8):
            bits = np.array([(k >> 2) & 1, (k >> 1) & 1, k & 1])
            c = lo + bits * s
            if c.min() < -KEY_BIAS or c.max() >= KEY_BIAS:
                continue  # outside the 16-bit field: absent, never another field's key
            key = (b << 48) | (int(c[0] + KEY_BIAS) << 32) | (int(c[1] + KEY_BIAS) << 16) | int(c[2] + KEY_BIAS)
            at = int(np.searchsorted(keys, key))
            if at < keys.shape[0] and keys[at] == key:
                nbr[i, k] = at
                f = np.where(bits == 1, t, 1.0 - t)
                w[i, k] = f[0] * f[1] * f[2]
    return nbr, w


def pairs(nbr, w):
    """the pairs that exist in ascending (n, k): (in_map = site rows [P] int32, out_map = point rows [P] int32, weights [P])"""
    at = np.nonzero(nbr.reshape(-1) >= 0)[0]
    return nbr.reshape(-1)[at].astype(np.int32), (at >> 3).astype(np.int32), w.reshape(-1)[at]


def forward(F, nbr, w):
    """[N, C] float64 = sum over the pairs of w * F[site]"""
    F = np.asarray(F, dtype=np.float64)
    out = np.zeros((nbr.shape[0], F.shape[1]), np.float64)
    sites, points, wt = pairs(nbr, w)
    np.add.at(out, points, wt[:, None] * F[sites])
    return out


def backward(dy, nbr, w, m):
    """[M, C] float64 = sum over the pairs of a site of w * dy[point]; a site without a pair gets zero"""
    dy = np.asarray(dy, dtype=np.float64)
    dF = np.zeros((m, dy.shape[1]), np.float64)
    sites, points, wt = pairs(nbr, w)
    np.add.at(dF, sites, wt[:, None] * dy[points])
    return dF


def forward_bound(F, nbr):
    """[N, C] = sum over the pairs of |F[site]| (the issue's forward bound is 32 * 2^-24 times this)"""
    return forward(np.abs(np.asarray(F, dtype=np.float64)), nbr, (nbr >= 0).astype(np.float64))


def backward_bound(dy, nbr, m):
    """([M, C] = sum over a site's pairs of |dy|, [M] = its number of pairs)"""
    present = (nbr >= 0).astype(np.float64)
    return backward(np.abs(np.asarray(dy, dtype=np.float64)), nbr, present, m), np.bincount(nbr[nbr >= 0], minlength=m)


def random_case(seed, tile, scenes=(0, 1), box=12, s=1, lo=-5):
    """The random case of the tests: per scene a Bernoulli(0.5) subset of a box^3 block of sites at stride s (lower corner lo * s)
    and 2 * tile + 5 points uniform in the box.  -> (keys [M] sorted, coords [M, 4], tfield [N, 4] float32)"""
    rng = np.random.default_rng(seed)
    grid = np.stack(np.meshgrid(*(np.arange(box),) * 3, indexing="ij"), -1).reshape(-1, 3)
    coords, pts = [], []
    for b in scenes:
        keep = grid[rng.random(grid.shape[0]) < 0.5]
        coords.append(np.concatenate((np.full((keep.shape[0], 1), b), (keep + lo) * s), 1))
        p = (rng.random((2 * tile + 5, 3)) * (box - 1) + lo) * s
        pts.append(np.concatenate((np.full((p.shape[0], 1), float(b)), p), 1))
    coords = np.concatenate(coords).astype(np.int64)
    keys = pack_keys(coords)
    order = np.argsort(keys)
    return keys[order], coords[order], np.concatenate(pts).astype(np.float32)
