"""The restatement of the channelwise convolution (tests/channelwise_restatement.py) against a definition the project already
trusts: ``R.conv`` of tests/sparse_modules_restatement.py with the kernel expanded to its diagonal [K, C, C], and torch autograd
through that expression.  No GPU needed."""
import numpy as np
import pytest
import torch

import channelwise_restatement as CW
import sparse_modules_restatement as R

FORWARD = [g for g in R.GEOMETRIES if not g.startswith("tr-")]


def _close(a, b, rel=1e-12):
    return bool(((a - b).abs() <= rel * max(float(b.abs().max()), 1e-300)).all())


@pytest.mark.parametrize("geometry", sorted(R.GEOMETRIES))
@pytest.mark.parametrize("cloud,C", [("two", 4), ("forty", 20), ("one", 4)])
def test_float64_restatement_is_the_diagonal_dense_convolution(cloud, C, geometry):
    ins, outs, nbr = R.pool_geometry(cloud, geometry)
    x, dy = R.pool_inputs(cloud, geometry, C)
    w, b = CW.weights(nbr.shape[0], C)
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    y = R.conv(x64, CW.diagonal_kernel(w64), nbr) + b64
    assert _close(CW.forward(x, w, nbr, b), y.detach())
    assert _close(CW.forward(x, w, nbr), (y - b64).detach())
    gx, gw, gb = torch.autograd.grad(y, (x64, w64, b64), dy.double())
    assert _close(CW.grad_input(dy, w, nbr, len(ins)), gx)
    assert _close(CW.grad_weight(x, dy, nbr), gw)
    assert _close(CW.grad_bias(dy), gb)


def test_fma32_rounds_once():
    one = np.float32(1)
    # a * b = 2^-24 - 2^-64, c = 1 + 2^-23: the exact sum lies just below a float32 tie that the float64 sum lands on
    a = np.array([2.0 ** -12 * (1 + 2.0 ** -20)], dtype=np.float32)
    b = np.array([2.0 ** -12 * (1 - 2.0 ** -20)], dtype=np.float32)
    c = np.array([1 + 2.0 ** -23], dtype=np.float32)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert naive[0] == one + np.float32(2.0 ** -22) and CW.fma32(a, b, c)[0] == c[0]
    assert CW.fma32(a, -b, -c)[0] == -c[0]
    # exact cases stay exact
    g = np.random.default_rng(0)
    p, q, r = (g.integers(-2048, 2048, 1000).astype(np.float32) for _ in range(3))
    assert np.array_equal(CW.fma32(p, q, r), p * q + r)


@pytest.mark.parametrize("geometry", FORWARD)
def test_float32_restatement_stays_within_the_bounds(geometry):
    """the kernels' order in float32 against float64: the derived bounds hold for the restatement itself"""
    ins, outs, nbr = R.pool_geometry("two", geometry)
    x, dy = R.pool_inputs("two", geometry, 20)
    w, b = CW.weights(nbr.shape[0], 20)
    y32 = CW.forward32(x, w, nbr, b)
    assert bool(((y32.double() - CW.forward(x, w, nbr, b)).abs() <= CW.bound_forward(x, w, nbr, b)).all())
    dx32 = CW.grad_input32(dy, w, nbr, len(ins))
    assert bool(((dx32.double() - CW.grad_input(dy, w, nbr, len(ins))).abs() <= CW.bound_input(dy, w, nbr, len(ins))).all())
    empty = (nbr >= 0).sum(0) == 0
    assert torch.equal(y32[empty], b[None].expand(int(empty.sum()), -1))
    assert torch.equal(CW.forward32(x, w, nbr)[empty], torch.zeros(int(empty.sum()), 20))
