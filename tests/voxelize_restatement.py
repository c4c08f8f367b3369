"""A numpy restatement of the voxeliser (csrc/sparse_voxel.hip): the maps are np.unique on the packed keys, the
quantisation modes are sequential float32 folds in ascending input-row order (np.add.at / np.maximum.at), the label rule is an
integer run test.  It shares no code with the package; tests/test_voxelize_restatement.py checks it against a dictionary loop."""
import numpy as np

KEY_BIAS = 32768


def pack_keys(coords):
    """[N, 4] integer (batch, x, y, z) -> int64 keys; ValueError outside the 16-bit fields"""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    if c.size and (c[:, 1:].min() < -KEY_BIAS or c[:, 1:].max() >= KEY_BIAS or c[:, 0].min() < 0 or c[:, 0].max() >= 32768):
        raise ValueError("voxel coordinates outside the 16-bit key range")
    return (c[:, 0] << 48) | ((c[:, 1] + KEY_BIAS) << 32) | ((c[:, 2] + KEY_BIAS) << 16) | (c[:, 3] + KEY_BIAS)


def voxel_indices(points, voxel_size):
    """the float32 arithmetic of the keys launch: ONE reciprocal, taken in double and rounded to float32, then a float32 product
    per coordinate"""
    inv = np.float32(1.0 / float(voxel_size))
    return np.floor(np.asarray(points, dtype=np.float32)[:, :3] * inv)


def cloud_coords(points, offsets, voxel_size):
    """packed points + offsets -> [N, 4] int64 (batch, x, y, z); ValueError on a non-finite coordinate"""
    f = voxel_indices(points, voxel_size)
    if not np.isfinite(f).all():
        raise ValueError("voxel coordinates outside the 16-bit key range")
    batch = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(np.asarray(offsets, dtype=np.int64)))
    return np.concatenate((batch[:, None], f.astype(np.int64)), 1)


def voxel_maps(keys):
    """keys [N] int64 -> (sites [M] ascending unique, inverse [N] int32, first [M] int64 = the lowest row of each site,
    seg [M + 1] int32 = the run starts in sorted order, order [N] int32 = the stable sort's permutation)"""
    keys = np.asarray(keys, dtype=np.int64)
    sites, first, inverse, counts = np.unique(keys, return_index=True, return_inverse=True, return_counts=True)
    seg = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    order = np.argsort(keys, kind="stable").astype(np.int32)
    return sites, inverse.reshape(-1).astype(np.int32), first.astype(np.int64), seg, order


def reduce_features(features, inverse, m, mode):
    """features [N, C] float32, inverse [N] -> ([M, C] float32, winners [M, C] int32 or None); rows folded in ascending order"""
    x = np.asarray(features, dtype=np.float32)
    n, c = x.shape
    inverse = np.asarray(inverse, dtype=np.int64)
    if mode == "first":
        first = np.full(m, n, np.int64)
        np.minimum.at(first, inverse, np.arange(n))
        return x[first], None
    if mode in ("sum", "average"):
        y = np.zeros((m, c), np.float32)
        np.add.at(y, inverse, x)
        if mode == "average":
            y = y / np.bincount(inverse, minlength=m).astype(np.float32)[:, None]
        return y.astype(np.float32), None
    assert mode == "max", mode
    y = np.full((m, c), -np.inf, np.float32)
    np.maximum.at(y, inverse, x)
    # the winner: the lowest row that holds the site's value (any NaN row where the value is a NaN: the first)
    hit = (x == y[inverse]) | (np.isnan(x) & np.isnan(y[inverse]))
    rows = np.where(hit, np.arange(n)[:, None], n)
    win = np.full((m, c), n, np.int64)
    np.minimum.at(win, inverse, rows)
    return y, win.astype(np.int32)


def reduce_grad(d_sites, inverse, m, mode, winners=None):
    """the gradient of ``reduce_features`` w.r.t. the features: [N, C] float32"""
    d = np.asarray(d_sites, dtype=np.float32)
    inverse = np.asarray(inverse, dtype=np.int64)
    n = inverse.shape[0]
    g = d[inverse]
    if mode == "sum":
        return g
    if mode == "average":
        return (g / np.bincount(inverse, minlength=m).astype(np.float32)[inverse][:, None]).astype(np.float32)
    if mode == "max":
        return np.where(winners[inverse] == np.arange(n)[:, None], g, np.float32(0)).astype(np.float32)
    first = np.full(m, n, np.int64)
    np.minimum.at(first, inverse, np.arange(n))
    return np.where((first[inverse] == np.arange(n))[:, None], g, np.float32(0)).astype(np.float32)


def slice_grad(d_points, inverse, m):
    """the gradient of site_features[inverse] w.r.t. the site features: the sum fold of the point gradients"""
    return reduce_features(d_points, inverse, m, "sum")[0]


def site_labels(labels, inverse, m, ignore_label=-100):
    """the label all points of a site share, ignore_label where they differ"""
    labels = np.asarray(labels, dtype=np.int64)
    inverse = np.asarray(inverse, dtype=np.int64)
    lo = np.full(m, np.iinfo(np.int64).max, np.int64)
    hi = np.full(m, np.iinfo(np.int64).min, np.int64)
    np.minimum.at(lo, inverse, labels)
    np.maximum.at(hi, inverse, labels)
    return np.where(lo == hi, lo, ignore_label)
