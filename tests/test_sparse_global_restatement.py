"""The instrument of tests/test_gpu_sparse_global.py discriminates (CPU only): the float64 restatement of global pooling,
broadcast and the squeeze-excite layer agrees with plain loops written from the definitions; a float32 restatement with ONE
defect is rejected by the rule the GPU file applies (norm_cases.compare, imported; equality for what is one rounding), while a
summation order taken out of the yardstick passes; and what the definitions lean on in NumPy is asserted."""
import math

import numpy as np
import pytest
import torch

import norm_cases as NC
import sparse_global_restatement as G

SMALL = [(s, 4) for s in ("two", "single", "absent", "one")]
HELD_OUT = (("tree", 64), "torch", 4)


def _others(order):
    return tuple(o for o in NC.ORDERS if o != order)


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.all(np.abs(a - b) <= 1e-11 * max(1.0, float(np.abs(b).max()))), what


@pytest.mark.parametrize("scenes,C", SMALL)
def test_pooling_restatement_agrees_with_plain_loops(scenes, C):
    c = G.case(scenes, C)
    sizes, x, dy = c["sizes"], c["x"].double().tolist(), c["dy_pool"].double().tolist()
    for mode in ("sum", "avg"):
        got = G.pool_eval(c["x"], sizes, mode, c["dy_pool"])
        y = [[0.0] * C for _ in sizes]
        dx = [[0.0] * C for _ in x]
        a = 0
        for s, n in enumerate(sizes):
            for ch in range(C):
                t = 0.0
                for i in range(a, a + n):
                    t += x[i][ch]
                scale = 1.0 if mode == "sum" or n == 0 else 1.0 / n
                y[s][ch] = t * scale
                for i in range(a, a + n):
                    dx[i][ch] = dy[s][ch] * scale
            a += n
        _close(got["y"].numpy(), y, mode)
        _close(got["dx"].numpy(), dx, mode)
    xm = c["x_max"].double().tolist()
    got = G.pool_eval(c["x_max"], sizes, "max", c["dy_pool"])
    a = 0
    for s, n in enumerate(sizes):
        for ch in range(C):
            best, row = None, -1
            for i in range(a, a + n):  # the first NaN, else the first of the largest values
                v = xm[i][ch]
                if best is None or (math.isnan(v) and not math.isnan(best)) or (not math.isnan(best) and v > best):
                    best, row = v, i
            want = 0.0 if n == 0 else best
            have = float(got["y"][s, ch])
            assert (math.isnan(want) and math.isnan(have)) or want == have, (s, ch)
            assert int(got["arg"][s, ch]) == row, (s, ch)
            for i in range(a, a + n):
                assert float(got["dx"][i, ch]) == (dy[s][ch] if i == row else 0.0)
        a += n


@pytest.mark.parametrize("scenes,C", SMALL)
def test_broadcast_and_gate_restatements_agree_with_plain_loops(scenes, C):
    c = G.case(scenes, C)
    sizes = c["sizes"]
    scene_of = [s for s, n in enumerate(sizes) for _ in range(n)]
    x, g, gc = c["x"].double().numpy(), c["g"].double().numpy(), c["g_cat"].double().numpy()
    for mode in G.BCAST_MODES:
        gg, dy = (gc, c["dy_cat"]) if mode == "cat" else (g, c["dy"])
        got = G.broadcast_eval(c["x"], torch.from_numpy(gg), sizes, mode, dy)
        d = dy.double().numpy()
        y, dx, dg = [], [], np.zeros_like(gg)
        for i, s in enumerate(scene_of):
            if mode == "add":
                y.append(x[i] + gg[s]), dx.append(d[i])
                dg[s] += d[i]
            elif mode == "mul":
                y.append(x[i] * gg[s]), dx.append(d[i] * gg[s])
                dg[s] += d[i] * x[i]
            else:
                y.append(np.concatenate((x[i], gg[s]))), dx.append(d[i][:C])
                dg[s] += d[i][C:]
        _close(got["y"].numpy(), np.array(y), mode)
        _close(got["dx"].numpy(), np.array(dx), mode)
        _close(got["dg"].numpy(), dg, mode)
    got = G.se_layer_eval(c["x"], sizes, c["w1"], c["b1"], c["w2"], c["b2"], c["residual"], True)
    w1, b1, w2, b2 = (c[k].double().numpy() for k in ("w1", "b1", "w2", "b2"))
    a, gates = 0, []
    for n in sizes:
        p = x[a:a + n].sum(0) / n if n else np.zeros(C)
        h = np.maximum(w1 @ p + b1, 0.0)
        gates.append(1.0 / (1.0 + np.exp(-(w2 @ h + b2))))
        a += n
    _close(got["gate"].numpy(), np.array(gates), "gate")
    res = c["residual"].double().numpy()
    y = np.array([np.maximum(x[i] * gates[s] + res[i], 0.0) for i, s in enumerate(scene_of)])
    _close(got["y"].numpy(), y, "se y")


def test_argmax_returns_the_first_nan_row_and_the_first_of_equal_maxima():
    """what the max definition leans on in NumPy"""
    nan, inf = float("nan"), float("inf")
    col = np.array([[1.0, 5.0, -inf, 2.0], [nan, 5.0, -inf, inf], [7.0, 1.0, -inf, nan], [nan, 5.0, -inf, 1e30]], dtype=np.float32)
    assert np.argmax(col, axis=0).tolist() == [1, 0, 0, 2]
    top = np.max(col, axis=0)
    assert np.isnan(top[0]) and top[1] == 5.0 and top[2] == -inf and np.isnan(top[3])
    assert np.argmax(np.array([3.0, inf, nan, inf], dtype=np.float32)) == 2 and np.argmax(np.array([-inf, -inf])) == 0


def _pool_rule(scenes, C, mode, got_kw, names=("y",)):
    c = G.case(scenes, C)
    args = (c["x"], c["sizes"], mode, c["dy_pool"])
    order = got_kw.get("order", "torch")
    rests = [G.pool_eval(*args, dtype=G.F32, order=o) for o in _others(order)]
    return NC.compare(G.pool_eval(*args, dtype=G.F32, **got_kw), G.pool_eval(*args), rests, names, label=f"{scenes} {C} {mode}")


def _bcast_rule(scenes, C, mode, got_kw):
    c = G.case(scenes, C)
    args = (c["x"], c["g_cat"] if mode == "cat" else c["g"], c["sizes"], mode, c["dy_cat"] if mode == "cat" else c["dy"])
    order = got_kw.get("order", "torch")
    rests = [G.broadcast_eval(*args, dtype=G.F32, order=o) for o in _others(order)]
    return NC.compare(G.broadcast_eval(*args, dtype=G.F32, **got_kw), G.broadcast_eval(*args), rests, ("dg",), label=f"{scenes} {C} {mode}")


def _se_rule(scenes, C, got_kw):
    c = G.case(scenes, C)
    args = (c["x"], c["sizes"], c["w1"], c["b1"], c["w2"], c["b2"], c["residual"], True)
    order = got_kw.get("order", "torch")
    rests = [G.se_layer_eval(*args, dtype=G.F32, order=o) for o in _others(order)]
    return NC.compare(G.se_layer_eval(*args, dtype=G.F32, **got_kw), G.se_layer_eval(*args), rests, ("gate", "y"), label=f"{scenes} {C} se")


@pytest.mark.parametrize("scenes,C", [("two", 20), ("single", 64), ("absent", 4), ("big", 64)])
def test_a_held_out_order_passes_the_rule(scenes, C):
    for order in HELD_OUT:
        for mode in ("sum", "avg"):
            _pool_rule(scenes, C, mode, dict(order=order))
        for mode in G.BCAST_MODES:
            _bcast_rule(scenes, C, mode, dict(order=order))
        _se_rule(scenes, C, dict(order=order))


@pytest.mark.parametrize("scenes,C", [("two", 20), ("single", 64), ("big", 64)])
def test_planted_defects_fail_the_rule(scenes, C):
    assert set(G.DEFECTS) == {"avg_by_total_N", "tie_highest", "seg_off_by_one", "mul_grad_without_x", "gate_without_relu"}
    with pytest.raises(AssertionError):
        _pool_rule(scenes, C, "avg", dict(defect="avg_by_total_N"))
    for mode in ("sum", "avg"):
        with pytest.raises(AssertionError):
            _pool_rule(scenes, C, mode, dict(defect="seg_off_by_one"))
    with pytest.raises(AssertionError):
        _bcast_rule(scenes, C, "add", dict(defect="seg_off_by_one"))
    with pytest.raises(AssertionError):
        _bcast_rule(scenes, C, "mul", dict(defect="mul_grad_without_x"))
    with pytest.raises(AssertionError):
        _se_rule(scenes, C, dict(defect="gate_without_relu"))
    # what is one rounding is held to equality: the planted tie (column 0) separates the lowest row from the highest
    c = G.case(scenes, C)
    good = G.pool_eval(c["x_max"], c["sizes"], "max", c["dy_pool"], dtype=G.F32)
    bad = G.pool_eval(c["x_max"], c["sizes"], "max", c["dy_pool"], dtype=G.F32, defect="tie_highest")
    assert G.same(good["y"], bad["y"]) and not G.same(good["arg"], bad["arg"]) and not G.same(good["dx"], bad["dx"])
    off = G.pool_eval(c["x_max"], c["sizes"], "max", c["dy_pool"], dtype=G.F32, defect="seg_off_by_one")
    assert not G.same(good["arg"], off["arg"])


def test_chunk_case_is_built_from_a_chunk_row_function():
    sizes = G.chunk_sizes(lambda n: max(16, -(-(-(-n // 64)) // 16) * 16))
    r = sizes[2] - 1
    assert sizes == (2 * r + 5, 2 * r, r + 1) and -(-sizes[0] // r) >= 3 and sizes[1] % r == 0
