"""Float64 restatement of the channelwise (depthwise) sparse convolution, written from its definition over the neighbour table,
a float32 restatement that follows the kernels' order, and the bounds the GPU tests hold the kernels to.  The clouds, geometries
and inputs are those of ``sparse_modules_restatement``.  Nothing here imports ``vdetr_amd`` or touches the GPU.

Definition.  W is [K, C]: one weight per offset and channel.  With N(u) = {k : nbr[k][u] >= 0}:
  forward  y[u][c]  = (sum over k in N(u) of W[k][c] * x[nbr[k][u]][c]) + b[c]
  dx       dx[i][c] = sum over the (k, u) with nbr[k][u] == i of W[k][c] * dy[u][c]
  dW       dW[k][c] = sum over the u with k in N(u) of x[nbr[k][u]][c] * dy[u][c];     db[c] = sum_u dy[u][c]
The kernels' order (forward, dx): the sum starts at +0 and takes one fmaf per present term in ascending k; the bias is added last.

Bounds, u = 2^-24, derived and not measured (no margin).  Forward: K fused multiply-adds and the bias add are K + 1 roundings of
partial sums no larger than S = sum_k |W x| + |b|: (K + 2) u S covers them with their second-order terms.  dx: K roundings,
(K + 1) u sum_k |W dy|.  dW[k][c]: n_k terms (the pairs of offset k) summed in ANY order are at most n_k roundings along a path,
(n_k + 1) u sum_u |x dy|; db[c]: nout terms, nout u sum_u |dy|.
"""
import numpy as np
import torch

from sparse_modules_restatement import CLOUDS, GEOMETRIES, cloud, inverse_table, pool_geometry, pool_inputs  # noqa: F401  (shared inputs)

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24


def weights(K, C, seed=0, bias=True):
    """(W [K, C], b [C] or None), float32"""
    g = torch.Generator().manual_seed(1000 * K + C + seed)
    w = torch.randn(K, C, generator=g) * 0.5
    return w, (torch.randn(C, generator=g) if bias else None)


# ---- float64, from the definition --------------------------------------------------------------------------------------------------
def forward(x, w, nbr, b=None):
    K, nout = nbr.shape
    x, w = x.to(F64), w.to(F64)
    y = torch.zeros((nout, x.shape[1]), dtype=F64)
    for k in range(K):
        u = torch.nonzero(nbr[k] >= 0)[:, 0]
        y[u] = y[u] + w[k] * x[nbr[k][u]]
    return y if b is None else y + b.to(F64).reshape(-1)


def grad_input(dy, w, nbr, nin):
    dy, w = dy.to(F64), w.to(F64)
    dx = torch.zeros((nin, dy.shape[1]), dtype=F64)
    for k in range(nbr.shape[0]):
        u = torch.nonzero(nbr[k] >= 0)[:, 0]
        i = nbr[k][u]
        dx[i] = dx[i] + w[k] * dy[u]  # (one reader per (i, k) on a lattice: no duplicate index)
    return dx


def grad_weight(x, dy, nbr):
    x, dy = x.to(F64), dy.to(F64)
    dw = torch.zeros((nbr.shape[0], x.shape[1]), dtype=F64)
    for k in range(nbr.shape[0]):
        u = torch.nonzero(nbr[k] >= 0)[:, 0]
        dw[k] = (x[nbr[k][u]] * dy[u]).sum(0)
    return dw


def grad_bias(dy):
    return dy.to(F64).sum(0)


# ---- float32, in the kernels' order -------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf on float32 numpy arrays, correctly rounded: the product of two float32 is exact in float64; the float64 sum is rounded
    to ODD (TwoSum gives its exact error), so that the second rounding to float32 cannot land on a false tie."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    even = (s.view(np.int64) & 1) == 0
    nudged = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, nudged, s).astype(np.float32)


def _fma_chain(src, w, table):
    """acc[r] = fmaf(w[k], src[table[k][r]], acc[r]) over the present k, ascending, from +0"""
    K, n = table.shape
    src, w = src.to(F32).numpy(), w.to(F32).numpy()
    acc = np.zeros((n, src.shape[1]), dtype=np.float32)
    tab = table.numpy()
    for k in range(K):
        has = tab[k] >= 0
        rows = src[np.where(has, tab[k], 0)] if src.shape[0] else np.zeros_like(acc)
        acc = np.where(has[:, None], fma32(np.broadcast_to(w[k][None], rows.shape), rows, acc), acc)
    return acc


def forward32(x, w, nbr, b=None):
    acc = _fma_chain(x, w, nbr)
    if b is not None:
        acc = acc + b.to(F32).reshape(-1).numpy()[None]
    return torch.from_numpy(acc)


def grad_input32(dy, w, nbr, nin):
    return torch.from_numpy(_fma_chain(dy, w, inverse_table(nbr, nin)))


# ---- bounds -----------------------------------------------------------------------------------------------------------------------------
def bound_forward(x, w, nbr, b=None):
    s = forward(x.abs(), w.abs(), nbr, None if b is None else b.abs())
    return (nbr.shape[0] + 2) * U * s


def bound_forward_dense(x, w, nbr, b=None):
    """the dense float32 convolution on the diagonal kernel [K, C, C]: its products with the zeros off the diagonal and their
    additions are exact, which leaves K rounded products, K rounded additions and the bias add: (2 K + 2) u S"""
    s = forward(x.abs(), w.abs(), nbr, None if b is None else b.abs())
    return (2 * nbr.shape[0] + 2) * U * s


def bound_input(dy, w, nbr, nin):
    return (nbr.shape[0] + 1) * U * grad_input(dy.abs(), w.abs(), nbr, nin)


def bound_weight(x, dy, nbr):
    n_k = (nbr >= 0).sum(1).to(F64)
    return (n_k + 1)[:, None] * U * grad_weight(x.abs(), dy.abs(), nbr)


def bound_bias(dy):
    return dy.shape[0] * U * dy.to(F64).abs().sum(0)


def diagonal_kernel(w):
    """[K, C] -> the dense kernel [K, C, C] with w[k] on the diagonal: the same operator for ``R.conv``"""
    return torch.diag_embed(w)
