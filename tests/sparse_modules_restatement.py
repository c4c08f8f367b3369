"""Float64 restatements of the sparse module library (kernel regions, pooling, InstanceNorm, residual blocks), written from
their definitions over a dictionary from coordinate to row, and the inputs the tests share.  Nothing here imports
``vdetr_amd.minkowski`` or ``vdetr_amd.sparse_ops``, and nothing here touches the GPU.

Definitions.  A kernel is a list of offsets; the reach of offset k is offset * dilation * tensor_stride (for the
transposed forms -offset * dilation * out_stride); nbr[k][u] is the input row at out_site[u] + reach[k] or -1; N(u) the k with a row.
  sum  y[u] = sum over N(u), ascending k;  avg: times 1 / |N(u)| (0 when empty);  max: per channel, arg = the LOWEST k attaining it
  backward  dx[i] = sum over k, ascending, of dy[u] (avg: * 1/|N(u)|; max: where arg[u][c] == k) over the u with nbr[k][u] == i
  InstanceNorm  per scene and channel: (x - mean) * rsqrt(biased var + eps) * weight + bias, eps = 1e-6
"""
import functools

import numpy as np
import torch

import norm_cases as NC

F64, F32 = torch.float64, torch.float32
IN_EPS = 1e-6


# ---- kernel regions ------------------------------------------------------------------------------------------------------------
def _triple(v):
    return (v, v, v) if isinstance(v, int) else tuple(v)


def _span(k):
    return list(range(-(k // 2), k // 2 + 1)) if k % 2 else list(range(k))


def cube_offsets(size):
    sx, sy, sz = _triple(size)
    return [(x, y, z) for z in _span(sz) for y in _span(sy) for x in _span(sx)]


def cross_offsets(size):
    out = [(0, 0, 0)]
    for axis, k in enumerate(_triple(size)):
        assert k % 2 == 1
        for d in range(1, k // 2 + 1):
            for sign in (-1, 1):
                o = [0, 0, 0]
                o[axis] = sign * d
                out.append(tuple(o))
    return out


# ---- sites and maps ------------------------------------------------------------------------------------------------------------
def sort_sites(coords):
    """unique rows in (batch, x, y, z) order"""
    return np.unique(np.asarray(coords, dtype=np.int64), axis=0)


def strided_sites(coords, ts):
    c = np.asarray(coords, dtype=np.int64).copy()
    c[:, 1:] = np.floor_divide(c[:, 1:], ts) * ts
    return sort_sites(c)


def neighbour_table(in_sites, out_sites, reach):
    """nbr [K, nout] int64 through a dictionary"""
    index = {tuple(int(v) for v in c): i for i, c in enumerate(in_sites)}
    nbr = np.full((len(reach), len(out_sites)), -1, dtype=np.int64)
    for k, (dx, dy, dz) in enumerate(reach):
        for u, (b, x, y, z) in enumerate(out_sites):
            nbr[k, u] = index.get((int(b), int(x) + dx, int(y) + dy, int(z) + dz), -1)
    return torch.from_numpy(nbr)


def scale_reach(offsets, factor):
    return [(x * factor, y * factor, z * factor) for x, y, z in offsets]


# ---- pooling -------------------------------------------------------------------------------------------------------------------
def _gathered(x, nbr):
    pad = torch.cat((x, x.new_zeros((1, x.shape[1]))))
    return pad[torch.where(nbr >= 0, nbr, torch.full_like(nbr, x.shape[0]))]  # [K, nout, C]


def pool_forward(x, nbr, mode, dtype=F64, defect=None):
    """-> (y [nout, C], inv_count [nout] (avg) or None, arg [nout, C] int64 (max) or None)"""
    K, nout = nbr.shape
    x = x.to(dtype)
    valid = nbr >= 0
    g = _gathered(x, nbr)
    cnt = valid.sum(0)
    if mode in ("sum", "avg"):
        y = torch.zeros((nout, x.shape[1]), dtype=dtype)
        for k in range(K):
            y = y + g[k]
        if mode == "sum":
            return y, None, None
        if defect == "avg_by_K":
            inv = torch.full((nout,), 1.0 / K, dtype=dtype)
        else:
            inv = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1).to(dtype), torch.zeros(nout, dtype=dtype))
        return y * inv[:, None], inv, None
    g = torch.where(valid[:, :, None], g, torch.full_like(g, -float("inf")))
    y = g.max(0).values
    hit = g == y[None]
    if defect == "tie_highest":
        arg = K - 1 - hit.flip(0).to(torch.int8).argmax(0)
    else:
        arg = hit.to(torch.int8).argmax(0)  # the first True: the lowest k
    empty = cnt == 0
    y = torch.where(empty[:, None], torch.zeros_like(y), y)
    arg = torch.where(empty[:, None], torch.full_like(arg, -1), arg)
    return y, None, arg


def pool_backward(dy, nbr, nin, mode, inv_count=None, arg=None, dtype=F64):
    K, nout = nbr.shape
    dy = dy.to(dtype)
    dx = torch.zeros((nin, dy.shape[1]), dtype=dtype)
    for k in range(K):
        u = torch.nonzero(nbr[k] >= 0)[:, 0]
        i = nbr[k][u]
        c = dy[u]
        if mode == "avg":
            c = c * inv_count.to(dtype)[u][:, None]
        elif mode == "max":
            c = c * (arg[u] == k).to(dtype)
        dx[i] = dx[i] + c  # (one reader per (i, k) on a lattice: no duplicate index)
    return dx


def pool_bound_forward(x, nbr, inv_count=None):
    """(K + 1) 2^-24 sum_k |x_k| (1 / |N|): the sequential-sum bound plus one rounding for the scale"""
    K = nbr.shape[0]
    s = _gathered(x.to(F64).abs(), nbr).sum(0)
    if inv_count is not None:
        s = s * inv_count.to(F64)[:, None]
    return (K + 1) * 2.0 ** -24 * s


def pool_bound_backward(dy, nbr, nin, inv_count=None):
    K = nbr.shape[0]
    return (K + 1) * 2.0 ** -24 * pool_backward(dy.abs(), nbr, nin, "avg" if inv_count is not None else "sum", inv_count)


# ---- pooling inputs ----------------------------------------------------------------------------------------------------------------
def cloud(n, seed, batch=2, extent=6, ts=1):
    rng = np.random.default_rng(seed)
    c = np.concatenate((rng.integers(0, batch, (n, 1)), rng.integers(-extent, extent, (n, 3)) * ts), 1)
    return sort_sites(c)


CLOUDS = ("two", "forty", "one")
# (name, transposed, offsets, dilation, stride)
GEOMETRIES = {
    "cube2-s2": (False, cube_offsets(2), 1, 2),
    "cube3-s1": (False, cube_offsets(3), 1, 1),
    "cube3-s2": (False, cube_offsets(3), 1, 2),
    "cross3-s1-d2": (False, cross_offsets(3), 2, 1),
    "custom-s1": (False, [(1, 0, 0), (0, 5, 0), (-1, -1, 0)], 1, 1),   # no centre: many sites have no neighbour at all
    "tr-cube2-s2": (True, cube_offsets(2), 1, 2),
    "tr-cube3-s2": (True, cube_offsets(3), 1, 2),
}


@functools.lru_cache(maxsize=None)
def fine_sites(name):
    """the sites of tensor stride 1: two scenes with a site at the edge of the key range; 40 sites; a single site"""
    if name == "two":
        c = np.concatenate((cloud(600, 11), [[0, -32768, 0, 32767], [1, 32767, -32768, 5]]))
        return sort_sites(c)
    if name == "forty":
        return cloud(44, 5, extent=3)[:40]
    return np.array([[0, 2, -3, 1]], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def pool_geometry(cloud_name, geometry):
    """(in_sites, out_sites, nbr [K, nout]) of a geometry on a cloud: the non-transposed forms read the fine sites, the transposed
    ones read the stride-2 sites and write the fine ones"""
    transposed, offsets, dilation, stride = GEOMETRIES[geometry]
    fine = fine_sites(cloud_name)
    if not transposed:
        out = strided_sites(fine, stride) if stride > 1 else fine
        return fine, out, neighbour_table(fine, out, scale_reach(offsets, dilation * 1))
    coarse = strided_sites(fine, stride)
    return coarse, fine, neighbour_table(coarse, fine, scale_reach(offsets, -dilation * 1))


def inverse_table(nbr, nin):
    inv = torch.full((nbr.shape[0], nin), -1, dtype=torch.int64)
    for k in range(nbr.shape[0]):
        u = torch.nonzero(nbr[k] >= 0)[:, 0]
        inv[k, nbr[k][u]] = u
    return inv


@functools.lru_cache(maxsize=None)
def pool_inputs(cloud_name, geometry, C):
    """(x [nin, C], dy [nout, C]): x drawn from 8 distinct values, so that maxima tie"""
    ins, outs, _ = pool_geometry(cloud_name, geometry)
    g = torch.Generator().manual_seed(len(ins) * 131 + C)
    values = torch.tensor([-1.5, -1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 2.0])
    x = values[torch.randint(0, 8, (len(ins), C), generator=g)]
    dy = torch.randn(len(outs), C, generator=g)
    return x, dy


# ---- InstanceNorm ------------------------------------------------------------------------------------------------------------------
def inorm_eval(x, sizes, gamma, beta, dy, dtype=F64, order="torch", defect=None, eps=IN_EPS):
    """forward and backward over the scenes of `sizes` rows each (a size of 0: a batch index without a site)"""
    x, dy, gamma, beta = x.to(dtype), dy.to(dtype), gamma.to(dtype), beta.to(dtype)
    y, dx = torch.zeros_like(x), torch.zeros_like(x)
    dg, db = torch.zeros_like(gamma), torch.zeros_like(beta)
    a = 0
    for n in sizes:
        if n == 0:
            continue
        xs, g = x[a:a + n], dy[a:a + n]
        src, m = (x, x.shape[0]) if defect == "whole_batch" else (xs, n)
        mean = NC._sum(src, (0,), order) / m
        var = NC._sum((src - mean) ** 2, (0,), order) / (max(m - 1, 1) if defect == "unbiased" else m)
        invstd = torch.rsqrt(var + eps)
        xh = (xs - mean) * invstd
        y[a:a + n] = xh * gamma + beta
        sg, sgx = NC._sum(g, (0,), order), NC._sum(g * xh, (0,), order)
        dx[a:a + n] = gamma * invstd * (g - sg / n - xh * (sgx / n))
        dg, db = dg + sgx, db + sg
        a += n
    return {"y": y.to(F64), "dx": dx.to(F64), "dweight": dg.to(F64), "dbias": db.to(F64)}


INORM_SCENES = {"two": (310, 257), "single": (300, 1, 150), "absent": (200, 0, 130), "one": (1,), "wide": (23, 17), "big": (1700, 1300)}
INORM_CASES = ([(s, C) for s in ("two", "single", "absent", "one") for C in (4, 20, 64)] + [("wide", 512), ("big", 64)])


@functools.lru_cache(maxsize=None)
def inorm_case(scenes, C):
    """x [N, C] whose (scene, channel) columns cycle through norm_cases' four kinds, affine parameters, dy, the element kinds and
    the analytic term of the columns whose variance is exactly 0 (constant, or a scene of one site)"""
    sizes = INORM_SCENES[scenes]
    g = torch.Generator().manual_seed(sum(sizes) * 7 + C)
    cols, kinds = [], []
    for s, n in enumerate(sizes):
        if n == 0:
            continue
        k = NC.kinds_of(C, shift=s)
        flat, _ = NC._fill(k, n, g)
        cols.append(flat.t())
        kinds.append(np.repeat(np.array([NC.KINDS.index(v) for v in k])[None], n, 0))
    x = torch.cat(cols).contiguous()
    gamma, beta = NC.affine(C, g)
    dy = torch.randn(x.shape, generator=g)
    group = np.concatenate(kinds)
    # |x_hat| of a flat column: the mean at most 2 ulp off the value, invstd <= 1 / sqrt(eps)
    xb_rows, a = [], 0
    for n in sizes:
        if n == 0:
            continue
        xs = x[a:a + n].to(F64)
        flat_c = (xs.amax(0) == xs.amin(0)).to(F64)
        xb = torch.tensor([2.0 * NC.ulp32(v) / np.sqrt(IN_EPS) if v > 0 else 0.0 for v in xs.abs().amax(0).tolist()], dtype=F64) * flat_c
        xb_rows.append(xb[None].expand(n, C))
        a += n
    xb = torch.cat(xb_rows)
    gabs = dy.abs().to(F64)
    extra = {"y": xb * gamma.abs().to(F64), "dweight": (xb * gabs).sum(0),
             "dx": xb * xb / np.sqrt(IN_EPS) * gamma.abs().to(F64) * float(gabs.max())}
    return {"sizes": sizes, "x": x, "gamma": gamma, "beta": beta, "dy": dy, "groups": {"y": group, "dx": group}, "extra": extra}


def inorm_reference(case):
    return inorm_eval(case["x"], case["sizes"], case["gamma"], case["beta"], case["dy"])


def inorm_restatements(case, orders=NC.ORDERS, **kw):
    return [inorm_eval(case["x"], case["sizes"], case["gamma"], case["beta"], case["dy"], dtype=F32, order=o, **kw) for o in orders]


# ---- convolution, BatchNorm and the residual blocks (float64, torch autograd) ------------------------------------------------------------
def conv(x, w, nbr):
    """out [nout, Cout] = sum_k x[nbr[k]] @ w[k]; w [K, Cin, Cout] or [Cin, Cout] (K = 1)"""
    w = w if w.dim() == 3 else w[None]
    return torch.einsum("knc,kcd->nd", _gathered(x, nbr), w)


def batch_norm(x, w, b, eps=1e-5):
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return (x - mean) * torch.rsqrt(var + eps) * w + b


def instance_norm(x, sizes, w, b, eps=IN_EPS):
    out, a = [], 0
    for n in sizes:
        if n == 0:
            continue
        xs = x[a:a + n]
        mean = xs.mean(0)
        var = ((xs - mean) ** 2).mean(0)
        out.append((xs - mean) * torch.rsqrt(var + eps) * w.reshape(-1) + b.reshape(-1))
        a += n
    return torch.cat(out)


def norm(P, prefix, kind, x, sizes):
    """kind "BN" | "IN" | "INBN" with the parameters `prefix`.* of the dictionary P"""
    if kind == "BN":
        return batch_norm(x, P[prefix + ".bn.weight"], P[prefix + ".bn.bias"])
    if kind == "IN":
        return instance_norm(x, sizes, P[prefix + ".weight"], P[prefix + ".bias"])
    x = instance_norm(x, sizes, P[prefix + ".0.weight"], P[prefix + ".0.bias"])
    return batch_norm(x, P[prefix + ".1.bn.weight"], P[prefix + ".1.bn.bias"])


def scene_sizes(sites, nscenes):
    return tuple(int((sites[:, 0] == s).sum()) for s in range(nscenes))


def block_forward(P, kind, bottleneck, x, maps, sizes_in, sizes_out):
    """the residual block on float64 parameters P: maps = {"conv1", "conv2" (, "conv3"), "downsample"} -> nbr tables.  The strided
    layer is conv1 (basic) / conv2 (bottleneck); the skip path is a 1x1x1 strided convolution and a BatchNorm."""
    residual = batch_norm(conv(x, P["downsample.0.kernel"], maps["downsample"]), P["downsample.1.bn.weight"], P["downsample.1.bn.bias"])
    if not bottleneck:
        out = torch.relu(norm(P, "norm1", kind, conv(x, P["conv1.kernel"], maps["conv1"]), sizes_out))
        out = norm(P, "norm2", kind, conv(out, P["conv2.kernel"], maps["conv2"]), sizes_out)
    else:
        out = torch.relu(norm(P, "norm1", kind, conv(x, P["conv1.kernel"], maps["conv1"]), sizes_in))
        out = torch.relu(norm(P, "norm2", kind, conv(out, P["conv2.kernel"], maps["conv2"]), sizes_out))
        out = norm(P, "norm3", kind, conv(out, P["conv3.kernel"], maps["conv3"]), sizes_out)
    return torch.relu(out + residual)
