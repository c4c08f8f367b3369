"""Cases, float64 references, fp32 restatements and the tolerance rule of the dense norm launches (add_ln.hip, bn_act.hip,
relu_dropout): shared by tests/test_norm_cases.py (CPU: the instrument discriminates) and tests/test_gpu_norm_parity.py (the
kernels).  Nothing here touches the GPU or the code under test.

Inputs.  Rows ([rows, C], LayerNorm) or channels ([B, C, N], BatchNorm) cycle through four kinds: plain (mean 0, sigma 1),
large mean (+-50 ... +-1000, sigma 1 ... 3), tiny (sigma 1e-4: variance 1e-8, far below eps = 1e-5) and constant (every element
3.5).  The channel means are the only thing that separates a two-pass variance from E[x^2] - mean^2.

References are written out by formula in float64.  The fp32 restatements are the same two-pass formulas in float32 on the
CPU, in twelve summation orders (torch's own; 2 ... 256 strided partial sums added up by torch; 16 / 64 / 256 strided partial
sums added up pairwise, the shape of a wave's all-reduce), and for BatchNorm's y also in the shift form y = x * a + sh
(a = gamma * invstd, sh = beta - mean * a) that bn_act.hip documents.  They are the yardstick, never the thing tested: the error
of a restatement is the elementwise maximum over those evaluations, so that one lucky rounding does not set the bar.  (The mean
of 130 values near 50 is one of two or three neighbouring floats whichever order adds them up, and d_gamma = sum g x_hat moves by
(mean error) invstd d_beta.  The nine orders that torch adds up all land 0.2 ulp above the true mean of [1, 5, 130]'s third
channel, the pairwise ones 0.8 below, 1.2 above and 0.2 above; on the CPU, with three orders as the yardstick and a fourth held
out as a stand-in kernel, the stand-in needed up to 8.4 times their error over 12 seeds of the BatchNorm cases; with eleven and
the pairwise 64 held out, at most 1.9 over 10 seeds.  tests/test_norm_cases.py holds orders out in the same way.)

The rule (`tolerance`):  max|kernel - ref64| <= FACTOR * max|restatement32 - ref64| + FACTOR * ulp32(max|ref64|), per tensor and
per row / channel kind.  Constant rows / channels add an analytic term from |x_hat| <= 2 ulp32(value) / sqrt(eps): the
restatement's error there can be exactly 0 while a kernel that multiplies by a rounded 1/C is one ulp off in the mean.
"""
import functools
import math

import numpy as np
import torch

EPS = 1e-5
MOMENTUM = 0.1
# Margin over the measured error of the restatement (summation order, hardware rsqrt); never above 16, where the mutants of
# tests/test_norm_cases.py must still fail.
FACTOR = 4
KINDS = ("plain", "large", "tiny", "const")
CONST_VALUE = 3.5
_LARGE_MEANS = (50.0, -100.0, 300.0, -1000.0, 1000.0, -50.0, 100.0, -300.0)
ORDERS = ("torch", 2, 4, 8, 16, 32, 64, 128, 256, ("tree", 16), ("tree", 64), ("tree", 256))
F64 = torch.float64
F32 = torch.float32


# ---- dropout: the kernels' documented scale ----------------------------------------------------------------------------------
def drop_threshold(p):
    """t = round(p * 65536) clamped to [1, 65535] (drop_stream.h: drop_rate; p travels as a float32); 0 without dropout"""
    if p <= 0.0:
        return 0
    t = int(float(np.float32(p)) * 65536.0 + 0.5)
    return min(max(t, 1), 65535)


def drop_scale(p):
    """65536 / (65536 - t): the unbiased scale for the mask's true keep probability q = (65536 - t) / 65536"""
    return 65536.0 / (65536.0 - drop_threshold(p))


def keep_prob(p):
    return (65536.0 - drop_threshold(p)) / 65536.0


def composite_p(p1, p2):
    """two independent Bernoulli masks in a row: one mask with keep probability (1 - p1)(1 - p2)"""
    return 1.0 - (1.0 - p1) * (1.0 - p2)


def ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def xhat_const_bound(value=CONST_VALUE):
    """|x_hat| of a constant row: the mean is at most 2 ulp off the value, 1/sqrt(var + eps) <= 1/sqrt(eps)"""
    return 2.0 * ulp32(value) / math.sqrt(EPS)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def kinds_of(count, shift=0):
    return [KINDS[(i + shift) % 4] for i in range(count)]


def _fill(kinds, width, g):
    """[len(kinds), width] float32 rows of the given kinds, and each row's sigma"""
    rows, sig = [], []
    nlarge = 0
    for k in kinds:
        z = torch.randn(width, generator=g, dtype=F64)
        if k == "plain":
            v, s = z, 1.0
        elif k == "large":
            s = 1.0 + 2.0 * float(torch.rand(1, generator=g))
            v = _LARGE_MEANS[nlarge % len(_LARGE_MEANS)] + s * z
            nlarge += 1
        elif k == "tiny":
            v, s = 1e-4 * z, 1e-4
        else:
            v, s = torch.full((width,), CONST_VALUE, dtype=F64), 0.0
        rows.append(v)
        sig.append(s)
    return torch.stack(rows).to(F32), sig


def affine(C, g, beta_floor=0.0):
    """gamma in 0.5 ... 1.5, beta in -1 ... 1 (|beta| >= beta_floor: the sign of a constant channel's pre-activation is beta's)"""
    gamma = 0.5 + torch.rand(C, generator=g)
    u = torch.rand(C, generator=g)
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    beta = sign * (beta_floor + (1.0 - beta_floor) * u)
    return gamma.to(F32), beta.to(F32)


class LnCase:
    """x [rows, C], the residual branch r (sized to the row's sigma so that y keeps the row's kind; 0 in constant rows),
    upstream gradients for y / out / out2 and two affine maps"""

    def __init__(self, rows, C, seed=0, shift=0):
        g = torch.Generator().manual_seed(1000003 * rows + 31 * C + seed)
        self.rows, self.C = rows, C
        self.kinds = kinds_of(rows, shift)
        self.x, sig = _fill(self.kinds, C, g)
        self.r = (torch.randn(rows, C, generator=g, dtype=F64) * 0.5 * torch.tensor(sig, dtype=F64)[:, None]).to(F32)
        self.gamma, self.beta = affine(C, g)
        self.gamma2, self.beta2 = affine(C, g)
        self.d_y, self.d_out, self.d_out2 = (torch.randn(rows, C, generator=g) for _ in range(3))
        self.group = np.array([KINDS.index(k) for k in self.kinds])[:, None]  # broadcasts over [rows, C]
        self.const_rows = np.array([k == "const" for k in self.kinds])


def _sum(t, dims, order):
    """sum over `dims` (moved last and flattened) in the given order: torch's; L strided partial sums added up by torch; or
    ("tree", L): L strided partial sums added up pairwise"""
    t = t.movedim(dims, tuple(range(-len(dims), 0))).flatten(-len(dims)) if len(dims) > 1 else t.movedim(dims[0], -1)
    if order == "torch":
        return t.sum(-1)
    tree = isinstance(order, tuple)
    lanes = order[1] if tree else order
    n = t.shape[-1]
    pad = (-n) % lanes
    if pad:
        t = torch.cat((t, t.new_zeros(t.shape[:-1] + (pad,))), -1)
    t = t.reshape(t.shape[:-1] + (-1, lanes)).cumsum(-2)[..., -1, :]  # each lane sequential
    if not tree:
        return t.sum(-1)
    while t.shape[-1] > 1:  # a butterfly of adjacent pairs: the shape of a wave's DPP all-reduce
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def ln_forward(c, keep, p, dtype=F64, has_r=True, dual=True, order="torch", defect=None):
    """y = x + keep r scale;  two-pass mean / variance;  out = (y - mean) rsqrt(var + eps) gamma + beta;  out2 likewise"""
    x = c.x.to(dtype)
    y = x
    scale = drop_scale(p)
    if has_r:
        y = x + (keep.to(dtype) * c.r.to(dtype) * scale if p > 0 else c.r.to(dtype))
    mean = (_sum(y, (1,), order) / c.C)[:, None]
    if defect == "one_pass":
        var = (_sum(y * y, (1,), order) / c.C)[:, None] - mean * mean
    else:
        var = (_sum((y - mean) ** 2, (1,), order) / c.C)[:, None]
    rstd = 1.0 / (torch.sqrt(var.clamp_min(0)) + EPS) if defect == "eps_outside" else torch.rsqrt(var + EPS)
    xhat = (y - mean) * rstd
    res = {"out": xhat * c.gamma.to(dtype) + c.beta.to(dtype), "xhat": xhat, "rstd": rstd}
    if has_r:
        res["y"] = y
    if dual:
        res["out2"] = xhat * c.gamma2.to(dtype) + c.beta2.to(dtype)
    return res


def ln_backward(c, fwd, keep, p, subset, dtype=F64, has_r=True, dual=True, order="torch", defect=None):
    """gradients of sum(y d_y + out d_out + out2 d_out2) over the tensors named in `subset`"""
    xhat, rstd = fwd["xhat"], fwd["rstd"]
    zero = torch.zeros_like(xhat)
    go = c.d_out.to(dtype) if "d_out" in subset else zero
    go2 = c.d_out2.to(dtype) if (dual and "d_out2" in subset) else zero
    gy = c.d_y.to(dtype) if (has_r and "d_y" in subset) else zero
    t = go * c.gamma.to(dtype)
    if defect != "dual_ignores_out2":
        t = t + go2 * c.gamma2.to(dtype)
    m1 = (_sum(t, (1,), order) / c.C)[:, None]
    m2 = (_sum(t * xhat, (1,), order) / c.C)[:, None]
    total = gy + rstd * (t - m1 - (0 if defect == "drop_xhat_term" else xhat * m2))
    res = {"d_x": total, "d_gamma": _sum(go * xhat, (0,), order), "d_beta": _sum(go, (0,), order)}
    if has_r:
        scale = 1.0 if defect == "dr_unscaled" else drop_scale(p)
        res["d_r"] = total * keep.to(dtype) * scale if p > 0 else total
    if dual:
        res["d_gamma2"], res["d_beta2"] = _sum(go2 * xhat, (0,), order), _sum(go2, (0,), order)
    return res


def ln_eval(c, keep, p, subset=("d_y", "d_out", "d_out2"), **kw):
    """forward and backward in one dictionary of float64 tensors"""
    fwd = ln_forward(c, keep, p, **kw)
    res = dict(fwd, **ln_backward(c, fwd, keep, p, subset, **kw))
    res.pop("xhat"), res.pop("rstd")
    return {k: v.to(F64) for k, v in res.items()}


def ln_restatements(c, keep, p, subset=("d_y", "d_out", "d_out2"), has_r=True, dual=True, orders=ORDERS):
    return [ln_eval(c, keep, p, subset, dtype=F32, has_r=has_r, dual=dual, order=o) for o in orders]


def ln_groups_and_extra(c, ref, subset=("d_y", "d_out", "d_out2"), dual=True):
    """per tensor: the row kinds (None for the parameter sums, which add up every row) and the analytic term of the constant
    rows: x_hat moves by at most xb there, so out by xb |gamma|, d_gamma by xb sum |d_out| over those rows, and d_x only in
    second order (rstd xb^2 max|t|: x_hat and mean(t x_hat) are both 0 in exact arithmetic)"""
    xb = xhat_const_bound()
    cr = torch.from_numpy(c.const_rows)
    rowmask = cr[:, None].to(F64)
    go = c.d_out.abs().to(F64) if "d_out" in subset else torch.zeros(c.rows, c.C, dtype=F64)
    go2 = c.d_out2.abs().to(F64) if (dual and "d_out2" in subset) else torch.zeros(c.rows, c.C, dtype=F64)
    tmax = float((go * c.gamma.abs() + go2 * c.gamma2.abs()).max())
    second = xb * xb / math.sqrt(EPS) * tmax * rowmask * drop_scale(0.5)  # (generous for d_r's scale: p <= 0.5 everywhere)
    groups = {k: c.group for k in ("y", "out", "out2", "d_x", "d_r")}
    extra = {"out": xb * c.gamma.abs().to(F64) * rowmask, "out2": xb * c.gamma2.abs().to(F64) * rowmask,
             "d_x": second, "d_r": second,
             "d_gamma": xb * (go * rowmask).sum(0), "d_gamma2": xb * (go2 * rowmask).sum(0)}
    return groups, extra


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------------
class BnCase:
    """x [B, C, N] (channel kinds cycling), gamma / beta, running statistics, the bias of a convolution in front, dy.
    `relu_margin`: x is nudged so that no fp64 pre-activation lies within its channel's y-tolerance of zero (see `nudge`)."""

    def __init__(self, B, C, N, seed=0, shift=0, const_ok=True):
        g = torch.Generator().manual_seed(7919 * B + 104729 * C + N + seed)
        self.B, self.C, self.N = B, C, N
        # without an affine map a constant channel's pre-activation is exactly 0, ambiguous by construction: plain instead
        self.kinds = [k if (const_ok or k != "const") else "plain" for k in kinds_of(C, shift)]
        flat, _ = _fill(self.kinds, B * N, g)
        self.x = flat.reshape(C, B, N).permute(1, 0, 2).contiguous()
        self.gamma, self.beta = affine(C, g, beta_floor=0.05)
        self.rm0, self.rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
        self.pre_bias = torch.randn(C, generator=g) * 3
        self.dy = torch.randn(B, C, N, generator=g)
        self.group = np.array([KINDS.index(k) for k in self.kinds])[None, :, None]
        self.group_c = self.group.reshape(C)
        xd = self.x.to(F64)
        self.flat_channels = np.array((xd.amax((0, 2)) == xd.amin((0, 2))).tolist())  # variance exactly 0 (constant, or n = 1)
        self.flat_value = xd.abs().amax((0, 2))
        self.ambiguous = {}


def bn_forward(c, keep, p, dtype=F64, training=True, relu=True, affine_on=True, pre_bias=False, order="torch", defect=None,
               x=None):
    """biased variance for normalising, unbiased (n / (n - 1), factor 1 at n = 1) with momentum for the running statistics;
    pre_bias enters the running mean only, and is subtracted from it in eval mode; optional affine, ReLU, dropout"""
    x = (c.x if x is None else x).to(dtype)
    n = c.B * c.N
    shape = (1, c.C, 1)
    pb = c.pre_bias.to(dtype) if pre_bias else torch.zeros(c.C, dtype=dtype)
    res = {}
    if training:
        mean = _sum(x, (0, 2), order) / n
        if defect == "one_pass":
            var = _sum(x * x, (0, 2), order) / n - mean * mean
        else:
            var = _sum((x - mean.reshape(shape)) ** 2, (0, 2), order) / n
        unbiased = var if defect == "biased_running_var" else var * (n / max(n - 1, 1))
        res["running_mean"] = (1 - MOMENTUM) * c.rm0.to(dtype) + MOMENTUM * (mean + pb)
        res["running_var"] = (1 - MOMENTUM) * c.rv0.to(dtype) + MOMENTUM * unbiased
    else:
        mean = c.rm0.to(dtype) + pb if defect == "pre_bias_added" else c.rm0.to(dtype) - pb
        var = c.rv0.to(dtype)
    invstd = 1.0 / (torch.sqrt(var.clamp_min(0)) + EPS) if defect == "eps_outside" else torch.rsqrt(var + EPS)
    ga = c.gamma.to(dtype) if affine_on else torch.ones(c.C, dtype=dtype)
    be = c.beta.to(dtype) if affine_on else torch.zeros(c.C, dtype=dtype)
    xhat = (x - mean.reshape(shape)) * invstd.reshape(shape)
    z = xhat * ga.reshape(shape) + be.reshape(shape)
    a = ga * invstd
    z_shift = x * a.reshape(shape) + (be - mean * a).reshape(shape)  # the form bn_act.hip evaluates
    kscale = keep.to(dtype) * drop_scale(p) if p > 0 else 1.0
    act = (lambda v: torch.relu(v)) if relu else (lambda v: v)
    res.update(y=act(z) * kscale, y_shift=act(z_shift) * kscale, z=z, xhat=xhat, invstd=invstd, ga=ga)
    return res


def bn_backward(c, fwd, keep, p, dtype=F64, relu=True, order="torch", defect=None):
    """dx = gamma invstd (g - mean(g) - x_hat mean(g x_hat)),  d_gamma = sum g x_hat,  d_beta = sum g"""
    n = c.B * c.N
    shape = (1, c.C, 1)
    g = c.dy.to(dtype)
    if p > 0:
        g = g * keep.to(dtype) * drop_scale(p)
    if relu:
        g = g * (fwd["z"] > 0).to(dtype)
    xhat = fwd["xhat"]
    db, dg = _sum(g, (0, 2), order), _sum(g * xhat, (0, 2), order)
    last = 0 if defect == "drop_xhat_term" else xhat * (dg / n).reshape(shape)
    dx = (fwd["ga"] * fwd["invstd"]).reshape(shape) * (g - (db / n).reshape(shape) - last)
    return {"dx": dx, "d_gamma": dg, "d_beta": db}


def bn_eval(c, keep, p, backward=True, **kw):
    fkw = dict(kw)
    fwd = bn_forward(c, keep, p, **fkw)
    res = dict(fwd)
    if backward:
        res.update(bn_backward(c, fwd, keep, p, **{k: v for k, v in kw.items() if k in ("dtype", "relu", "order", "defect")}))
    for k in ("xhat", "invstd", "ga"):
        res.pop(k)
    return {k: v.to(F64) for k, v in res.items()}


def bn_restatements(c, keep, p, backward=True, orders=ORDERS, **kw):
    """one evaluation per summation order; y additionally in the shift form (as a second entry with the other tensors alike)"""
    out = []
    for o in orders:
        r = bn_eval(c, keep, p, backward, dtype=F32, order=o, **kw)
        out.append(r)
        out.append(dict(r, y=r["y_shift"]))
    return out


def bn_groups_and_extra(c, p=0.0, training=True, affine_on=True):
    """channel kinds for every tensor ([B, C, N] and [C] alike) and the analytic term of the channels whose variance is 0"""
    groups = {"y": c.group, "dx": c.group, "d_gamma": c.group_c, "d_beta": c.group_c, "running_mean": c.group_c,
              "running_var": c.group_c}
    if not training:
        return groups, {}
    flat = torch.from_numpy(c.flat_channels).to(F64)
    xb = torch.tensor([xhat_const_bound(v) if v > 0 else 0.0 for v in c.flat_value.tolist()], dtype=F64) * flat
    ga = c.gamma.abs().to(F64) if affine_on else torch.ones(c.C, dtype=F64)
    s = drop_scale(p)
    gabs = c.dy.abs().to(F64) * s
    extra = {"y": (xb * ga * s)[None, :, None].expand(c.B, c.C, c.N),
             "d_gamma": xb * gabs.sum((0, 2)),
             "dx": (xb * xb / math.sqrt(EPS) * ga * gabs.amax((0, 2)))[None, :, None].expand(c.B, c.C, c.N)}
    return groups, extra


# ---- the tolerance rule ----------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().to(F64).numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def restatement_error(ref, rests):
    """elementwise max over the restatements of |restatement32 - ref64|"""
    ref = _np(ref)
    err = np.zeros_like(ref)
    for r in rests:
        err = np.maximum(err, np.abs(_np(r) - ref))
    return err


def tolerance(ref, rests, group=None, extra=None, factor=FACTOR):
    """the tolerance of every element of `ref`:  factor * max|restatement32 - ref64| + factor * ulp32(max|ref64|), both maxima
    over the element's group (row / channel kind; the whole tensor without `group`), plus the analytic term `extra`"""
    assert factor <= 16
    ref = _np(ref)
    rerr = restatement_error(ref, rests)
    gid = np.zeros(ref.shape, dtype=np.int64) if group is None else np.broadcast_to(np.asarray(group), ref.shape)
    tol = np.zeros_like(ref)
    for k in np.unique(gid):
        m = gid == k
        tol[m] = factor * rerr[m].max() + factor * ulp32(np.abs(ref[m]).max())
    if extra is not None:
        tol = tol + np.broadcast_to(_np(extra), ref.shape)
    return tol


def compare(got, ref, rests, names, groups=None, extra=None, factor=FACTOR, label="", ratios=None):
    """assert the rule for every tensor in `names`; `rests` is a list of dictionaries (the restatements).  Returns
    {name: (kernel error, restatement error, factor used)} and, with `ratios`, keeps the worst of them under `label`."""
    groups, extra = groups or {}, extra or {}
    out, bad = {}, []
    for n in names:
        r = _np(ref[n])
        g = _np(got[n]).reshape(r.shape)
        rs = [x[n] for x in rests]
        tol = tolerance(r, rs, groups.get(n), extra.get(n), factor)
        err = np.abs(g - r)
        kerr, rerr = float(err.max()), float(restatement_error(r, rs).max())
        used = float((err / tol).max()) * factor  # the factor this tensor would have needed (the rule allows `factor`)
        out[n] = (kerr, rerr, used)
        if ratios is not None:
            prev = ratios.setdefault(label, {}).get(n, (0.0, 0.0, 0.0))
            ratios[label][n] = max(prev, out[n], key=lambda v: v[2])
        if not np.all(np.isfinite(g)) or np.any(err > tol):
            i = np.unravel_index(np.argmax(err - tol), err.shape)
            bad.append(f"{label} {n}: |kernel - ref| {err[i]:.3e} > tol {tol[i]:.3e} at {i} (ref {r[i]:.6g}, got {g[i]:.6g}; "
                       f"max err {kerr:.3e}, restatement {rerr:.3e})")
    assert not bad, "\n".join(bad)
    return out


# ---- ReLU margins ------------------------------------------------------------------------------------------------------------------
def _y_tolerance_per_channel(c, x, **kw):
    """the y-tolerance of every channel for the inputs x, without dropout (dropout only scales y and its tolerance alike)"""
    ref = bn_eval(c, None, 0.0, backward=False, x=x, **kw)
    rests = []
    for o in ORDERS:
        r = bn_eval(c, None, 0.0, backward=False, x=x, dtype=F32, order=o, **kw)
        rests += [r, dict(r, y=r["y_shift"])]
    # on the pre-activation itself (a ReLU would hide the negative half): relu=False in kw
    tol = tolerance(ref["y"], [r["y"] for r in rests], c.group)
    return ref["y"], tol


def nudge(c, training=True, affine_on=True, pre_bias=False):
    """Moves every x whose fp64 pre-activation z lies within its channel's y-tolerance of zero away from it (to 8 tolerances,
    through dz/dx = gamma invstd), at most three times; records the number of ambiguous elements that are left (asserted 0 by
    tests/test_norm_cases.py for every case of the GPU file).  Established on the reference alone."""
    key = (training, affine_on, pre_bias)
    if key in c.ambiguous:
        return c.ambiguous[key]
    kw = dict(training=training, relu=False, affine_on=affine_on, pre_bias=pre_bias)
    x = c.x.clone()
    left = None
    for trip in range(4):
        z, tol = _y_tolerance_per_channel(c, x, **kw)
        zz = z.numpy()
        amb = np.abs(zz) < tol
        left = int(amb.sum())
        if left == 0 or trip == 3:
            break
        fwd = bn_forward(c, None, 0.0, x=x, **kw)
        slope = (fwd["ga"] * fwd["invstd"]).reshape(1, c.C, 1).expand_as(x).numpy()
        sgn = np.where(zz >= 0, 1.0, -1.0)
        step = sgn * (8 * tol - np.abs(zz)) / slope
        xn = x.to(F64).numpy().copy()
        # with batch statistics a channel of constant value keeps its value (its z is beta, which `affine` keeps away from 0)
        movable = amb & ~np.broadcast_to(c.flat_channels[None, :, None], amb.shape) if training else amb
        xn[movable] += step[movable]
        x = torch.from_numpy(xn).to(F32)
    c.x = x
    c.ambiguous[key] = left
    return left


# ---- relu_dropout --------------------------------------------------------------------------------------------------------------------
def relu_dropout_case(n, seed=0):
    """n values of both signs with exact zeros and -0.0 sprinkled in, and an upstream gradient"""
    g = torch.Generator().manual_seed(seed + n)
    x = torch.randn(n, generator=g)
    x[0::7] = 0.0
    x[3::11] = -0.0
    return x, torch.randn(n, generator=g)


def relu_dropout_ref(x, dy, keep, p):
    s = drop_scale(p)
    k = keep.to(F64) if p > 0 else torch.ones_like(x, dtype=F64)
    pos = (x > 0).to(F64)
    return {"y": x.to(F64) * pos * k * s, "dx": dy.to(F64) * pos * k * s}


# ---- binomial bounds of the masks ----------------------------------------------------------------------------------------------------
def keep_sigma(p, n):
    q = keep_prob(p)
    return math.sqrt(q * (1.0 - q) / n)


# ---- the case lists of the GPU file, and the dispatch arm each one reaches (restated in tests/test_norm_cases.py) ---------------------
LN_C = (256, 512, 768, 1024)
LN_ROWS = (1, 8, 9, 16, 17, 33)
_LN_COMBOS = ((False, 0.0, False), (True, 0.1, True), (False, 0.1, True), (True, 0.0, True), (True, 0.0, False), (False, 0.0, True))


def _ln_cases():
    """(rows, C, dual, p, has_r): every C with every rows value; the six (dual, p, residual) combinations rotate so that each C
    meets each of them, dual with dropout included"""
    out = []
    for ci, C in enumerate(LN_C):
        for ri, rows in enumerate(LN_ROWS):
            dual, p, has_r = _LN_COMBOS[(ci + ri) % len(_LN_COMBOS)]
            out.append((rows, C, dual, p, has_r))
    out += [(1041, 256, True, 0.1, True), (1041, 1024, False, 0.0, False)]  # 66 partial rows: the reduction's second trip
    return out


LN_CASES = _ln_cases()
LN_SUBSETS = (("d_y",), ("d_out",), ("d_out2",), ("d_y", "d_out", "d_out2"))   # at C = 512, dual

# (pass index) -> (rows, C, dual, first LayerNorm's index, has_r): 36 passes (35 of them parked), three widths, groups sharing a first norm
LN_DEFERRED = [(17 if i % 5 else 33, (256, 512, 1024)[i % 3], i % 4 == 1, (i % 3) * 10 + (i // 3) % 3, i % 2 == 0) for i in range(36)]

BN_CASES = [(1, 6, 256), (2, 5, 128), (8, 4, 32), (2, 9, 256), (1, 4, 1024), (4, 7, 256), (4, 5, 512), (2, 3, 2048), (16, 4, 256),
            (3, 5, 256), (1, 4, 1280), (1, 4, 4352), (2, 6, 130), (1, 3, 255), (1, 5, 7), (1, 2, 1)]
BN_P = (0.0, 0.3)
# (B, C, N, relu, p, affine, pre_bias): each variant on one register arm and one sweep arm
BN_VARIANTS = [(4, 7, 256, False, 0.3, True, False), (3, 5, 256, False, 0.3, True, False),
               (4, 7, 256, True, 0.0, False, False), (3, 5, 256, True, 0.3, False, False),
               (4, 7, 256, True, 0.3, True, True), (3, 5, 256, True, 0.0, True, True)]
BN_EVAL = [(2, 6, 130, True, True), (2, 6, 130, False, True), (4, 7, 256, True, False)]  # (B, C, N, relu, affine); pre_bias always
BN_CROSSED = (1, 4, 1024)
BN_RECORDS = ([(1, (5, 64, 70)[i % 3], 512) if i % 2 else (2, (5, 64, 70)[i % 3], 256) for i in range(14)],
              [(1, 5, 130), (2, 64, 65), (1, 70, 130)])
RELU_DROPOUT_N = (4, 1020, 4 * (524288 + 77))


@functools.lru_cache(maxsize=None)
def ln_case(rows, C, seed=0):
    return LnCase(rows, C, seed, shift=C // 256 - 1 + rows)


@functools.lru_cache(maxsize=None)
def bn_case(B, C, N, training=True, affine_on=True, pre_bias=False, seed=0):
    """the case's inputs, nudged for the ReLU margin of this (mode, affine, pre_bias): one object per combination"""
    c = BnCase(B, C, N, seed, shift=B + N, const_ok=affine_on or not training)
    left = nudge(c, training, affine_on, pre_bias)
    assert left == 0, f"{left} ambiguous ReLU elements left in {(B, C, N, training, affine_on, pre_bias)}"
    return c
