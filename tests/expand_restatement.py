"""NumPy restatements of the caller-chosen output sites: the sites of an expanding layer and the key order of a
coordinate list.  Nothing here imports ``vdetr_amd`` or touches the GPU.

Definition.  The output sites of a layer with ``expand_coordinates=True`` are exactly the sites u of the output lattice whose row
of the kernel map is not empty.  The map of a convolution reads, for output site u and offset k, the input site u + offset_k * ts
(transposed: u - offset_k * out_ts).  So an input site v is read through k from
  not transposed (stride 1)   u = v - offset_k * ts      (the MINUS: an even cube or a custom region is not symmetric)
  transposed                  u = v + offset_k * out_ts  (the children of a generative transposed convolution)
``offsets`` are the generator's scaled offsets (dilation included), in units of the stride named above.
"""
import numpy as np

import sparse_modules_restatement as R

# name -> (scaled offsets, transposed, the layer's stride): the transposed forms read sites of stride 2 * out_ts
REGIONS = {
    "cube3": (R.cube_offsets(3), False, 1),
    "cube2": (R.cube_offsets(2), False, 1),            # asymmetric: the case that catches a wrong sign
    "cross3": (R.cross_offsets(3), False, 1),
    "custom-x": ([(1, 0, 0)], False, 1),
    "cube3-d2": (R.scale_reach(R.cube_offsets(3), 2), False, 1),
    "tr-cube2-s2": (R.cube_offsets(2), True, 2),
    "tr-cube3-s2": (R.cube_offsets(3), True, 2),
}


def strides(region, out_ts):
    """(ts, out_ts) of a region's layer writing at ``out_ts``"""
    _, transposed, stride = REGIONS[region]
    return (out_ts * stride, out_ts) if transposed else (out_ts, out_ts)


def candidates(in_sites, offsets, ts, out_ts, transposed):
    """[N * K, 4] int64, site-major: one row per (input site, offset), duplicates kept"""
    s = np.asarray(in_sites, dtype=np.int64).reshape(-1, 4)
    off = np.asarray(offsets, dtype=np.int64).reshape(-1, 3)
    step = off * out_ts if transposed else -off * ts
    c = np.repeat(s[:, None, :], len(off), 1)
    c[:, :, 1:] += step[None]
    return c.reshape(-1, 4)


def expanded_sites(in_sites, offsets, ts, out_ts, transposed):
    """the unique candidates in (batch, x, y, z) order, [M, 4] int64"""
    c = candidates(in_sites, offsets, ts, out_ts, transposed)
    return np.unique(c, axis=0) if len(c) else c


def target_sites(coords):
    """(sites [M, 4] unique in (batch, x, y, z) order, inverse [len(coords)]: sites[inverse] == coords)"""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    if not len(c):
        return c, np.zeros(0, dtype=np.int64)
    sites, inverse = np.unique(c, axis=0, return_inverse=True)
    return sites, inverse.reshape(-1)


def reach(offsets, ts, out_ts, transposed):
    """what the kernel map adds to an OUTPUT site to find its input site, per offset (``neighbour_table``'s third argument)"""
    f = -out_ts if transposed else ts
    return [(x * f, y * f, z * f) for x, y, z in offsets]
