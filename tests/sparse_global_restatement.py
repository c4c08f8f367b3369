"""Float64 restatements of the ops between a sparse tensor's table and one row per scene (global pooling, broadcast, the
squeeze-excite layer and the SE basic block's tail), written from their definitions per scene slice, and the inputs the tests
share.  Nothing here imports ``vdetr_amd``, and nothing here touches the GPU.

Definitions.  Scene s of `sizes` is the next sizes[s] rows (a size of 0: a batch index without a site).
  pooling   sum; avg = sum * (1 / n); max = np.max with arg = np.argmax + the scene's first row (ties: the lowest row; a NaN wins,
            the lowest NaN row; a column of -inf: the first row); a scene without rows: y = 0, arg = -1
            backward  dx = dy[s] (sum), dy[s] * (1 / n) (avg), dy[s, c] where arg[s, c] is the row, else 0 (max)
  broadcast add y = x + g[s]; mul y = x * g[s]; cat y = (x | g[s])
            backward  dx = dy, dy * g[s], dy[:, :Cx];  dg[s] = sum dy, sum dy * x, sum dy[:, Cx:]  (0 for a scene without rows)
  SE layer  gate[s] = sigmoid(W2 relu(W1 avg_s(x) + b1) + b2) (a scene without rows: the formula at 0);  y = x * gate[s]
            (+ residual) (then ReLU)
"""
import functools

import numpy as np
import torch

import norm_cases as NC
import sparse_modules_restatement as R

F64, F32 = torch.float64, torch.float32
POOL_MODES = ("sum", "avg", "max")
BCAST_MODES = ("add", "mul", "cat")
DEFECTS = ("avg_by_total_N", "tie_highest", "seg_off_by_one", "mul_grad_without_x", "gate_without_relu")


def scene_ranges(sizes, N=None, defect=None):
    """[(s, first row, end row)]; the defect cuts every scene one row late"""
    out, a = [], 0
    total = sum(sizes) if N is None else N
    for s, n in enumerate(sizes):
        lo, hi = (a, a + n) if defect != "seg_off_by_one" else (min(a + 1, total), min(a + n + 1, total))
        out.append((s, lo, hi))
        a += n
    return out


def _inv(n, dtype):
    return torch.ones((), dtype=dtype) / torch.tensor(float(n), dtype=dtype)


# ---- pooling -----------------------------------------------------------------------------------------------------------------------
def pool_eval(x, sizes, mode, dy, dtype=F64, order="torch", defect=None):
    """forward and backward: {"y" [nseg, C], "dx" [N, C], "arg" [nseg, C] int64 (max)}"""
    x, dy = x.to(dtype), dy.to(dtype)
    N, C = x.shape
    y = torch.zeros((len(sizes), C), dtype=dtype)
    dx = torch.zeros_like(x)
    arg = torch.full((len(sizes), C), -1, dtype=torch.int64)
    for s, a, e in scene_ranges(sizes, N, defect):
        n = e - a
        if n <= 0:
            continue
        xs = x[a:e]
        if mode == "max":
            v = xs.numpy()
            if defect == "tie_highest":
                top = np.max(v, axis=0)
                hit = (v == top[None]) | (np.isnan(v) & np.isnan(top)[None])
                k = n - 1 - np.argmax(hit[::-1], axis=0)
            else:
                k = np.argmax(v, axis=0)
            y[s] = torch.from_numpy(np.max(v, axis=0).copy())
            arg[s] = torch.from_numpy(k + a)
            rows = torch.arange(a, e)[:, None]
            dx[a:e] = torch.where(rows == arg[s][None], dy[s][None].expand(n, C), torch.zeros((), dtype=dtype))
            continue
        total = NC._sum(xs, (0,), order)
        if mode == "sum":
            y[s] = total
            dx[a:e] = dy[s]
        else:
            inv = _inv(N if defect == "avg_by_total_N" else n, dtype)
            y[s] = total * inv
            dx[a:e] = dy[s] * inv
    out = {"y": y, "dx": dx}
    if mode == "max":
        out["arg"] = arg
    return out


# ---- broadcast ---------------------------------------------------------------------------------------------------------------------
def broadcast_eval(x, g, sizes, mode, dy, dtype=F64, order="torch", defect=None):
    """forward and backward: {"y", "dx" [N, Cx], "dg" [nseg, Cg]}"""
    x, g, dy = x.to(dtype), g.to(dtype), dy.to(dtype)
    N, Cx = x.shape
    Cg = g.shape[1]
    y = torch.zeros((N, Cx + Cg if mode == "cat" else Cx), dtype=dtype)
    dx = torch.zeros_like(x)
    dg = torch.zeros_like(g)
    for s, a, e in scene_ranges(sizes, N, defect):
        if e <= a:
            continue
        xs, d = x[a:e], dy[a:e]
        if mode == "add":
            y[a:e], dx[a:e], dg[s] = xs + g[s], d, NC._sum(d, (0,), order)
        elif mode == "mul":
            y[a:e], dx[a:e] = xs * g[s], d * g[s]
            dg[s] = NC._sum(d if defect == "mul_grad_without_x" else d * xs, (0,), order)
        else:
            y[a:e] = torch.cat((xs, g[s][None].expand(e - a, Cg)), 1)
            dx[a:e], dg[s] = d[:, :Cx], NC._sum(d[:, Cx:], (0,), order)
    return {"y": y, "dx": dx, "dg": dg}


# ---- the squeeze-excite layer ----------------------------------------------------------------------------------------------------------
def se_gate(x, sizes, w1, b1, w2, b2, order="torch", defect=None):
    """gate [nseg, C] in x's dtype (differentiable)"""
    rows = []
    for s, a, e in scene_ranges(sizes, x.shape[0], defect):
        p = NC._sum(x[a:e], (0,), order) * _inv(e - a, x.dtype) if e > a else x.new_zeros(x.shape[1])
        h = w1 @ p + b1
        if defect != "gate_without_relu":
            h = torch.relu(h)
        rows.append(torch.sigmoid(w2 @ h + b2))
    return torch.stack(rows)


def se_layer_eval(x, sizes, w1, b1, w2, b2, residual=None, relu=False, dtype=F64, order="torch", defect=None):
    """{"gate" [nseg, C], "y" [N, C]}: y = x * gate[s] (+ residual) (ReLU)"""
    x, w1, b1, w2, b2 = (t.to(dtype) for t in (x, w1, b1, w2, b2))
    gate = se_gate(x, sizes, w1, b1, w2, b2, order, defect)
    y = torch.zeros_like(x)
    for s, a, e in scene_ranges(sizes, x.shape[0], defect):
        y[a:e] = x[a:e] * gate[s]
    if residual is not None:
        y = y + residual.to(dtype)
    if relu:
        y = torch.relu(y)
    return {"gate": gate, "y": y}


def _batch_norm(P, prefix, x, training, eps=1e-5):
    if training:
        return R.batch_norm(x, P[prefix + ".bn.weight"], P[prefix + ".bn.bias"], eps)
    invstd = torch.rsqrt(P[prefix + ".bn.running_var"] + eps)
    return (x - P[prefix + ".bn.running_mean"]) * invstd * P[prefix + ".bn.weight"] + P[prefix + ".bn.bias"]


def se_basic_block(P, x, nbr, sizes, order="torch", defect=None, training=True):
    """SEBasicBlock (BatchNorm, stride 1, no downsample) on the parameters P (a state dict in the dtype of x): conv -> BN -> ReLU
    -> conv -> BN -> SE -> + x -> ReLU.  Differentiable.  ``training`` False: the BatchNorms use their running statistics."""
    out = torch.relu(_batch_norm(P, "norm1", R.conv(x, P["conv1.kernel"], nbr), training))
    out = _batch_norm(P, "norm2", R.conv(out, P["conv2.kernel"], nbr), training)
    gate = se_gate(out, sizes, P["se.fc.0.linear.weight"], P["se.fc.0.linear.bias"], P["se.fc.2.linear.weight"],
                   P["se.fc.2.linear.bias"], order, defect)
    scaled = torch.cat([out[a:e] * gate[s] for s, a, e in scene_ranges(sizes, x.shape[0])])
    return torch.relu(scaled + x)


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def chunk_sizes(chunk_rows):
    """three scenes built from the kernel's chunk-row function (rows per chunk of a table of N rows): one spans three chunks, one
    ends exactly on a chunk boundary, one is a single chunk plus one row"""
    r = 16
    for _ in range(8):
        sizes = (2 * r + 5, 2 * r, r + 1)
        if chunk_rows(sum(sizes)) == r:
            return sizes
        r = chunk_rows(sum(sizes))
    raise AssertionError("no table whose chunk rows reproduce themselves")


CASES = [(s, C) for s in ("two", "single", "absent", "one") for C in (4, 20, 64)] + [("wide", 512), ("big", 64)]
CHUNK_CASES = [("chunks", 20), ("chunks", 64)]
_SIZES = dict(R.INORM_SCENES)


def set_chunk_sizes(sizes):
    _SIZES["chunks"] = tuple(sizes)
    case.cache_clear()


@functools.lru_cache(maxsize=None)
def case(scenes, C):
    """x [N, C] (norm_cases' four column kinds), the per-scene rows g, upstream gradients, SE weights (H = max(C // 4, 1)), and
    x_max: x with, in every scene, column 0 holding its maximum twice (rows 1 and n - 1: different chunks in a large scene),
    column 1 all -inf, column 2 a +inf, column 3 a NaN in a middle row with a larger finite value after it"""
    sizes = _SIZES[scenes]
    N, nseg = sum(sizes), len(sizes)
    gen = torch.Generator().manual_seed(N * 11 + C)
    cols = []
    for s, n in enumerate(sizes):
        if n:
            flat, _ = NC._fill(NC.kinds_of(C, shift=s), n, gen)
            cols.append(flat.t())
    x = torch.cat(cols).contiguous()
    H = max(C // 4, 1)
    out = {"sizes": sizes, "x": x, "g": torch.randn(nseg, C, generator=gen), "g_cat": torch.randn(nseg, 8, generator=gen),
           "dy": torch.randn(N, C, generator=gen), "dy_cat": torch.randn(N, C + 8, generator=gen),
           "dy_pool": torch.randn(nseg, C, generator=gen), "residual": torch.randn(N, C, generator=gen),
           "w1": torch.randn(H, C, generator=gen) / C ** 0.5 * 0.004, "b1": torch.randn(H, generator=gen) * 0.3,
           "w2": torch.randn(C, H, generator=gen) / H ** 0.5, "b2": torch.randn(C, generator=gen) * 0.3}
    xm = x.clone()
    a = 0
    for n in sizes:
        if n:
            xm[a + min(1, n - 1), 0] = xm[a + n - 1, 0] = 1e4
            xm[a:a + n, 1] = -float("inf")
            xm[a + n // 2, 2] = float("inf")
            xm[a + n // 2, 3] = float("nan")
            if n - 1 > n // 2:
                xm[a + n - 1, 3] = 1e5
        a += n
    out["x_max"] = xm
    return out


def same(a, b):
    """equal element for element, a NaN equal to a NaN"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.shape != b.shape:
        return False
    if not a.is_floating_point():
        return bool(torch.equal(a.to(torch.int64), b.to(torch.int64)))
    a, b = a.to(F64), b.to(F64)
    return bool(torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), 0.0, a), torch.where(b.isnan(), 0.0, b)))
