"""Cases, float64 references, fp32 restatements and arms of the decoder layer's row-block launches (csrc/rowblock.hip: rb_qkv,
rb_proj_q, rb_ffn, rb_ffn0 and their backward launches): shared by tests/test_rowblock_cases.py (CPU: the instrument discriminates)
and tests/test_gpu_rowblock_parity.py (the kernels).  Nothing here touches the GPU or the code under test.

Cases.  (nQ, B) with rows = nQ * B and C = 256; rows are numbered as the sequence-first tensors lay them out (row = q * B + b), and
every per-row tensor here is [rows, 256] in THAT order, the batch-first operands of the attention cores included (`to_bf` /
`from_bf` convert).  The residual rows (tgt; for ffn0 the input x) cycle through the four row kinds of norm_cases; a, pos, weights
(scale 1/16), biases, LayerNorm affines and upstream gradients are plain.

References are written out by formula in float64.  The fp32 restatements are the same formulas in float32 on the CPU: LayerNorm sums
in NC.ORDERS, each 256-long contraction as torch.mm, as 2 ... 64 strided partial sums, as one sequential fused-multiply-add chain
over k (the order rowblock.hip documents for v_mfma_f32_16x16x4_f32) and as that chain in the order the kernel feeds its matrix
instructions (k = 16 m + 4 kg + e: step (m, e) adds the four lane groups kg).  They are the yardstick, never the thing tested.  The
rule is NC.tolerance / NC.compare, unchanged, per tensor and per row kind.

ReLU gates.  b1 is moved per column (at most three trips) until no fp64 pre-activation lies within its own rule-tolerance of zero,
under every dropout configuration the GPU file uses (the masks are host masks of a fixed {seed, offset}: STATE); the count left is
recorded per case and asserted 0 by tests/test_rowblock_cases.py.
"""
import functools
import math

import numpy as np
import torch

import drop_stream_restatement as R
import norm_cases as NC

C = 256
F64, F32 = NC.F64, NC.F32
SHAPES = ((1, 1), (15, 1), (16, 1), (17, 1), (32, 1), (8, 2), (9, 2), (11, 3))
# the step's {seed, offset} the GPU file establishes (torch.manual_seed(STATE[0]); reset_rng(); begin_step()) and reads back
STATE = (20240611, 0)
SALTS = {"drop1": 1101, "drop2": 1102, "drop3": 1103, "act": 1104, "ffn0_act": 1105, "ffn0_res": 1106}
P = 0.1                           # every dropout module's p where dropout is on
P2 = NC.composite_p(P, P)         # proj_drop and dropout2: one mask
MM_ORDERS = ("mm", 2, 4, 8, 16, 32, 64, "fma", "mfma")
EVALS = tuple((MM_ORDERS[i % len(MM_ORDERS)], o) for i, o in enumerate(NC.ORDERS))   # (contraction order, LayerNorm sum order)
_MFMA_K = [16 * m + 4 * kg + e for m in range(16) for e in range(4) for kg in range(4)]


def to_bf(rows2d, B):
    """[nQ * B, C] rows (q, b) -> batch-first [B, nQ, C]"""
    return rows2d.reshape(-1, B, rows2d.shape[-1]).transpose(0, 1).contiguous()


def from_bf(t, B):
    """batch-first [B, nQ, C] -> rows (q, b)"""
    return t.transpose(0, 1).reshape(-1, t.shape[-1])


def _inverted(rows2d, nQ, B):
    """the rows as a kernel would leave them whose batch-major mapping is inverted: row r lands where row (r % nQ) * B + r / nQ belongs"""
    r = torch.arange(nQ * B)
    out = torch.empty_like(rows2d)
    out[(r % nQ) * B + r // nQ] = rows2d
    return out


def arm_of(shape):
    """which geometry of the 16-row workgroups a case reaches (labels of the ratio table): scenes, blocks, and the row groups g
    (rows 4 g .. 4 g + 3 of the last block) that hold rows past the end"""
    nQ, B = shape
    rows = nQ * B
    tail = rows % 16
    dead = [g for g in range(4) if tail and 4 * g + 3 >= tail]
    return {"scenes": B, "blocks": -(-rows // 16), "tail": tail, "dead_groups": tuple(dead),
            "label": f"B {B}, {rows} rows" + (f" (tail {tail})" if tail else " (full)")}


# ---- the arms of the GPU file --------------------------------------------------------------------------------------------------
# qkv: (shape, pos given, pos requires grad, d_alias in the loss, which of q / k / v are in the loss)
QKV_ARMS = [(s, True, True, True, "qkv") for s in SHAPES] + [
    ((17, 1), False, False, False, "qkv"), ((9, 2), False, False, False, "qkv"),
    ((17, 1), True, False, False, "qkv"), ((11, 3), True, False, False, "qkv"),
    ((16, 1), True, True, False, "qkv"), ((8, 2), True, True, False, "qkv"),
    ((17, 1), True, True, True, "q"), ((11, 3), True, True, True, "qk"), ((15, 1), True, True, True, "v"), ((9, 2), True, True, True, "kv")]
# proj_q: (shape, p, pos given, loss on "y" / "q" / "yq", a requires grad)
PROJQ_ARMS = [(s, P, True, "yq", True) for s in SHAPES] + [
    ((17, 1), 0.0, True, "yq", True), ((9, 2), 0.0, True, "yq", True), ((1, 1), 0.0, True, "yq", True),
    ((15, 1), P, False, "yq", True), ((11, 3), P, False, "yq", True),
    ((17, 1), P, True, "y", True), ((8, 2), P, True, "y", True), ((17, 1), P, True, "q", True), ((11, 3), P, True, "q", True),
    ((17, 1), P, True, "yq", False), ((8, 2), P, True, "yq", False)]
# ffn: (shape, mode, two output norms, loss on a subset of "z", "1", "2"); mode "drop": dropout2 / proj_drop / dropout / dropout3 all
# at P (composite p2), "p0": training with every p = 0, "eval"
FFN_ARMS = [(s, "drop", True, "z12") for s in SHAPES] + [
    ((17, 1), "drop", False, "z1"), ((11, 3), "drop", False, "z1"),
    ((17, 1), "drop", True, "z"), ((17, 1), "drop", True, "1"), ((17, 1), "drop", True, "2"), ((11, 3), "p0", True, "2"), ((9, 2), "drop", True, "z"),
    ((17, 1), "p0", True, "z12"), ((8, 2), "p0", True, "z12"), ((1, 1), "p0", True, "z12"),
    ((17, 1), "eval", True, "z12"), ((11, 3), "eval", True, "z12")]
# ffn0: (shape, p, loss on a subset of "z", "1")
FFN0_ARMS = [(s, P, "z1") for s in SHAPES] + [
    ((17, 1), 0.0, "z1"), ((11, 3), 0.0, "z1"), ((17, 1), P, "z"), ((17, 1), P, "1"), ((9, 2), 0.0, "z"), ((11, 3), P, "1")]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
class RbCase:
    def __init__(self, nQ, B, seed=0):
        g = torch.Generator().manual_seed(7001 * nQ + 131 * B + seed)
        self.nQ, self.B, self.rows = nQ, B, nQ * B
        rows = self.rows
        self.kinds = NC.kinds_of(rows, nQ + B)
        self.group = np.array([NC.KINDS.index(k) for k in self.kinds])[:, None]
        self.const_rows = np.array([k == "const" for k in self.kinds])
        self.tgt, _ = NC._fill(self.kinds, C, g)       # the residual rows of qkv (there: norm1's output), proj_q and ffn
        self.x0, _ = NC._fill(self.kinds, C, g)        # ffn0's input
        plain = lambda s=1.0: (torch.randn(rows, C, generator=g) * s).to(F32)  # noqa: E731
        self.a, self.pos = plain(), plain(0.5)
        self.W = {n: (torch.randn(C, C, generator=g) / 16).to(F32) for n in ("q", "k", "v", "o", "c", "p", "1", "2", "f1", "f2")}
        self.b = {n: (torch.randn(C, generator=g) * 0.5).to(F32) for n in ("q", "k", "v", "o", "c", "p", "1", "2", "f1", "f2")}
        self.ln = {n: NC.affine(C, g) for n in ("n2", "n3", "p1", "p2", "f", "fp")}
        self.d = {n: plain() for n in ("q", "k", "v", "alias", "y", "qout", "z", "o1", "o2", "fz", "fo1")}
        self.ambiguous = None

    @functools.lru_cache(maxsize=None)
    def keep(self, name, p):
        """the host mask of stream `name` at STATE: [rows, 256] float64 (None without dropout)"""
        if p <= 0:
            return None
        g = R.stream(SALTS[name], 0, STATE)
        if name in ("act", "ffn0_act"):
            k = R.keep_flat(self.rows * C, p, g).reshape(self.rows, C)
        else:
            k = R.keep_add_ln(self.rows, C, p, g)
        return torch.from_numpy(np.ascontiguousarray(k)).to(F64)


# ---- one evaluation: dtype, contraction order, LayerNorm sum order, optionally ONE defect --------------------------------------------
class Ev:
    def __init__(self, dtype=F64, mm="mm", order="torch", defect=None):
        self.dtype, self.mm, self.order, self.defect = dtype, mm, order, defect

    def c(self, t):
        return None if t is None else t.to(self.dtype)

    def sum(self, t, dim):
        return NC._sum(t, (dim,), self.order)

    def _contract(self, x, wt, acc0=None):
        """x [r, K] times wt [K, N] with the sum over K in this evaluation's order; acc0: what the accumulators hold already (a
        chain carries on from it, as rb_qkv_bwd_kernel's does through its three products; every other order adds it at the end)"""
        how = self.mm
        K = x.shape[1]
        if acc0 is not None and not (how in ("fma", "mfma") and self.dtype != F64):
            return acc0 + self._contract(x, wt)
        if how == "mm" or self.dtype == F64:
            return x @ wt
        if how in ("fma", "mfma"):
            ks = _MFMA_K if (how == "mfma" and K == C) else range(K)
            xd, wd = x.to(F64), wt.to(F64)
            acc = torch.zeros(x.shape[0], wt.shape[1], dtype=self.dtype) if acc0 is None else acc0
            for k in ks:  # the product of two floats is exact in float64: one rounding per step
                acc = (acc.to(F64) + xd[:, k, None] * wd[k][None, :]).to(self.dtype)
            return acc
        L = how
        pad = (-K) % L
        if pad:
            x = torch.cat((x, x.new_zeros(x.shape[0], pad)), 1)
            wt = torch.cat((wt, wt.new_zeros(pad, wt.shape[1])), 0)
        xs, ws = x.reshape(x.shape[0], -1, L), wt.reshape(-1, L, wt.shape[1])
        acc = torch.zeros(x.shape[0], L, wt.shape[1], dtype=self.dtype)
        for s in range(xs.shape[1]):  # every lane sequential
            acc = acc + xs[:, s, :, None] * ws[s][None]
        return acc.sum(1)

    def lin(self, x, W, b=None):
        y = self._contract(x, W.t().contiguous())
        return y if b is None else y + b

    def back(self, d, W, acc0=None):
        """dX = dY W (+ acc0)"""
        return self._contract(d, W, acc0)

    def wgrad(self, dy, x):
        """dW = dY^T X (the sum runs over the rows)"""
        return self._contract(dy.t().contiguous(), x)

    def ln(self, y, affine):
        ga, be = (self.c(t) for t in affine)
        mean = (self.sum(y, 1) / C)[:, None]
        var = (self.sum((y - mean) ** 2, 1) / C)[:, None]
        rstd = torch.rsqrt(var + NC.EPS)
        xhat = (y - mean) * rstd
        return xhat * ga + be, xhat, rstd

    def ln_bwd(self, gos, gammas, xhat, rstd, din):
        """gos: the gradients of the norm's affine outputs (one or two).  Returns the total gradient of the normalised tensor and
        (d_gamma, d_beta) per output."""
        t = sum(go * self.c(ga) for go, ga in zip(gos, gammas))
        m1 = (self.sum(t, 1) / C)[:, None]
        m2 = (self.sum(t * xhat, 1) / C)[:, None]
        dx = din + rstd * (t - m1 - (0 if self.defect == "drop_xhat_term" else xhat * m2))
        sums = []
        for go in gos:
            dg, db = self.sum(go * xhat, 0), self.sum(go, 0)
            if self.defect == "tail_dup" and xhat.shape[0] % 16:  # the copy of the last row a tail block computes on, counted once
                dg, db = dg + go[-1] * xhat[-1], db + go[-1]
            sums.append((dg, db))
        return dx, sums


def _scaled(keep, p, ev):
    """keep * scale as a tensor, or 1.0 without dropout"""
    return 1.0 if (p <= 0 or keep is None) else keep.to(ev.dtype) * NC.drop_scale(p)


def _used(c, ev, name, on):
    t = ev.c(c.d[name])
    return t if on else torch.zeros_like(t)


# ---- qkv ---------------------------------------------------------------------------------------------------------------------------
def qkv_eval(c, ev, pos=True, alias=True, use="qkv"):
    """x = t + pos;  q = x Wq^T + bq, k = x Wk^T + bk, v = t Wv^T + bv;  d_t = dq Wq + dk Wk + dv Wv, d_pos = dq Wq + dk Wk + d_alias"""
    W, b = {n: ev.c(c.W[n]) for n in "qkv"}, {n: ev.c(c.b[n]) for n in "qkv"}
    t = ev.c(c.tgt)
    x = t + ev.c(c.pos) if pos else t
    res = {"q": ev.lin(x, W["q"], b["q"]), "k": ev.lin(x, W["k"], b["k"]),
           "v": ev.lin(x if ev.defect == "v_from_x" else t, W["v"], b["v"])}
    if ev.defect == "qout_bmajor" and c.B > 1:
        res["q"] = _inverted(res["q"], c.nQ, c.B)
    dq, dk, dv = (_used(c, ev, n, n in use) for n in "qkv")
    d_x = ev.back(dk, W["k"], ev.back(dq, W["q"]))   # one accumulator through the three products
    res["d_t"] = ev.back(dv, W["v"], d_x)
    if pos:
        da = ev.c(c.d["alias"]) if alias else 0
        res["d_pos"] = d_x + da
        if ev.defect == "alias_in_dt":
            res["d_t"] = res["d_t"] + da
    for n, dy, xx in (("q", dq, x), ("k", dk, x), ("v", dv, t)):
        res["d_W" + n], res["d_b" + n] = ev.wgrad(dy, xx), ev.sum(dy, 0)
    return res


def qkv_names(pos, pos_grad):
    return ["q", "k", "v", "d_t"] + (["d_pos"] if (pos and pos_grad) else []) + [f"d_{k}{n}" for n in "qkv" for k in "Wb"]


# ---- proj_q ------------------------------------------------------------------------------------------------------------------------
def projq_eval(c, ev, p=P, pos=True, use="yq"):
    """y = tgt + keep1 s1 (a Wo^T + bo);  t2 = LN2(y);  q = (t2 + pos) Wq^T + bq"""
    Wo, Wc, bo, bc = ev.c(c.W["o"]), ev.c(c.W["c"]), ev.c(c.b["o"]), ev.c(c.b["c"])
    a = ev.c(c.a)
    ks = _scaled(c.keep("drop1", p), p, ev)
    y = ev.c(c.tgt) + ks * ev.lin(a, Wo, bo)
    t2, xhat, rstd = ev.ln(y, c.ln["n2"])
    xq = t2 + ev.c(c.pos) if pos else t2
    res = {"y": y, "q": ev.lin(xq, Wc, bc)}
    if ev.defect == "qout_bmajor" and c.B > 1:
        res["q"] = _inverted(res["q"], c.nQ, c.B)
    dq, dy = _used(c, ev, "qout", "q" in use), _used(c, ev, "y", "y" in use)
    d_xq = ev.back(dq, Wc)
    res["d_Wc"], res["d_bc"] = ev.wgrad(dq, xq), ev.sum(dq, 0)
    if pos:
        res["d_pos"] = d_xq
    d_y, ((res["d_g2"], res["d_be2"]),) = ev.ln_bwd([d_xq], [c.ln["n2"][0]], xhat, rstd, dy)
    res["d_tgt"] = d_y
    d_proj = d_y * (c.keep("drop1", p).to(ev.dtype) if (ev.defect == "dproj_unscaled" and p > 0) else ks)
    res["d_a"] = ev.back(d_proj, Wo)
    if ev.defect == "da_bmajor" and c.B > 1:
        res["d_a"] = _inverted(res["d_a"], c.nQ, c.B)
    res["d_Wo"], res["d_bo"] = ev.wgrad(d_proj, a), ev.sum(d_proj, 0)
    res["_d_proj"] = d_proj
    return res


def projq_names(pos, use, a_grad):
    return (["y", "q", "d_tgt", "d_Wo", "d_bo", "d_g2", "d_be2"] + (["d_a"] if a_grad else []) +
            (["d_Wc", "d_bc"] + (["d_pos"] if pos else []) if "q" in use else []))


# ---- ffn ---------------------------------------------------------------------------------------------------------------------------
FFN_MODES = {"drop": (P2, P, P), "p0": (0.0, 0.0, 0.0), "eval": (0.0, 0.0, 0.0)}   # (p2, pa, p3)


def ffn_eval(c, ev, mode="drop", two=True, use="z12"):
    """y = tgt + keep2 s2 (a Wp^T + bp);  t2 = LN3(y);  h = keepA sA relu(t2 W1^T + b1);  z = y + keep3 s3 (h W2^T + b2);
    o1 = P1(z), o2 = P2(z)"""
    p2, pa, p3 = FFN_MODES[mode]
    Wp, W1, W2 = (ev.c(c.W[n]) for n in "p12")
    bp, b1, b2 = (ev.c(c.b[n]) for n in "p12")
    a = ev.c(c.a)
    k2 = c.keep("drop2", p2)
    s2 = _scaled(k2, p2, ev)
    if ev.defect == "p2_alone" and p2 > 0:  # the scale of dropout2.p alone behind the composite mask
        s2 = k2.to(ev.dtype) * NC.drop_scale(P)
    kA, k3 = c.keep("act", pa), c.keep("drop3", p3)
    sA, s3 = _scaled(kA, pa, ev), _scaled(k3, p3, ev)
    y = ev.c(c.tgt) + s2 * ev.lin(a, Wp, bp)
    t2, xhat, rstd = ev.ln(y, c.ln["n3"])
    pre = ev.lin(t2, W1, b1)
    gate = (pre > 0).to(ev.dtype)
    h = sA * gate * pre
    z = y + s3 * ev.lin(h, W2, b2)
    o1, zhat, zrstd = ev.ln(z, c.ln["p1"])
    res = {"y": y, "pre": pre, "z": z, "o1": o1}
    gos, gammas = [_used(c, ev, "o1", "1" in use)], [c.ln["p1"][0]]
    if two:
        res["o2"] = zhat * ev.c(c.ln["p2"][0]) + ev.c(c.ln["p2"][1])
        if ev.defect != "ignore_o2":
            gos.append(_used(c, ev, "o2", "2" in use))
            gammas.append(c.ln["p2"][0])
    d_z, sums = ev.ln_bwd(gos, gammas, zhat, zrstd, _used(c, ev, "z", "z" in use))
    res["d_gp1"], res["d_bp1"] = sums[0]
    if two:
        res["d_gp2"], res["d_bp2"] = sums[1] if len(sums) > 1 else (torch.zeros(C, dtype=ev.dtype), torch.zeros(C, dtype=ev.dtype))
    d_lin2 = d_z * s3
    res["d_W2"], res["d_b2"] = ev.wgrad(d_lin2, h), ev.sum(d_lin2, 0)
    d_lin1 = ev.back(d_lin2, W2) * gate * (NC.drop_scale(pa) if ev.defect == "act_nokeep" else sA)
    res["d_W1"], res["d_b1"] = ev.wgrad(d_lin1, t2), ev.sum(d_lin1, 0)
    d_y, ((res["d_g3"], res["d_be3"]),) = ev.ln_bwd([ev.back(d_lin1, W1)], [c.ln["n3"][0]], xhat, rstd, d_z)
    res["d_tgt"] = d_y
    d_proj = d_y * (k2.to(ev.dtype) if (ev.defect == "dproj_unscaled" and p2 > 0) else s2)
    res["d_a"] = ev.back(d_proj, Wp)
    if ev.defect == "da_bmajor" and c.B > 1:
        res["d_a"] = _inverted(res["d_a"], c.nQ, c.B)
    res["d_Wp"], res["d_bp"] = ev.wgrad(d_proj, a), ev.sum(d_proj, 0)
    res.update(_d_proj=d_proj, _d_lin2=d_lin2, _d_lin1=d_lin1)
    return res


def ffn_names(two):
    return (["z", "o1", "d_a", "d_tgt", "d_Wp", "d_bp", "d_W1", "d_b1", "d_W2", "d_b2", "d_g3", "d_be3", "d_gp1", "d_bp1"] +
            (["o2", "d_gp2", "d_bp2"] if two else []))


# ---- ffn0 --------------------------------------------------------------------------------------------------------------------------
def ffn0_eval(c, ev, p=P, use="z1"):
    """t2 = LN(x);  h = keepA sA relu(t2 W1^T + b1);  z = t2 + keep3 s3 (h W2^T + b2);  o1 = P(z)"""
    W1, W2, b1, b2 = ev.c(c.W["f1"]), ev.c(c.W["f2"]), ev.c(c.b["f1"]), ev.c(c.b["f2"])
    kA, k3 = c.keep("ffn0_act", p), c.keep("ffn0_res", p)
    sA, s3 = _scaled(kA, p, ev), _scaled(k3, p, ev)
    x = ev.c(c.x0)
    t2, xhat, rstd = ev.ln(x, c.ln["f"])
    pre = ev.lin(t2, W1, b1)
    gate = (pre > 0).to(ev.dtype)
    h = sA * gate * pre
    z = (x if ev.defect == "ffn0_res_x" else t2) + s3 * ev.lin(h, W2, b2)
    o1, zhat, zrstd = ev.ln(z, c.ln["fp"])
    res = {"pre": pre, "z": z, "o1": o1}
    d_z, ((res["d_gp"], res["d_bep"]),) = ev.ln_bwd([_used(c, ev, "fo1", "1" in use)], [c.ln["fp"][0]], zhat, zrstd, _used(c, ev, "fz", "z" in use))
    d_lin2 = d_z * s3
    res["d_W2"], res["d_b2"] = ev.wgrad(d_lin2, h), ev.sum(d_lin2, 0)
    d_lin1 = ev.back(d_lin2, W2) * gate * (NC.drop_scale(p) if ev.defect == "act_nokeep" else sA)
    res["d_W1"], res["d_b1"] = ev.wgrad(d_lin1, t2), ev.sum(d_lin1, 0)
    g_t2 = ev.back(d_lin1, W1) + (0 if ev.defect == "ffn0_no_res_grad" else d_z)  # t2 feeds lin1 AND the residual
    res["d_x"], ((res["d_g"], res["d_be"]),) = ev.ln_bwd([g_t2], [c.ln["f"][0]], xhat, rstd, torch.zeros_like(x))
    res.update(_g_t2=g_t2, _d_lin1=d_lin1, _d_lin2=d_lin2, _h=h, _zrstd=zrstd)
    return res


FFN0_NAMES = ["z", "o1", "d_x", "d_W1", "d_b1", "d_W2", "d_b2", "d_g", "d_be", "d_gp", "d_bep"]


def ffn0_extra(c, ref, p):
    """the analytic term of ffn0's constant rows (the only LayerNorm here that sees one: proj_q and ffn normalise tgt + branch).
    x_hat moves by at most xb there, so t2 by dt = xb |gamma|; that reaches z directly and through |W1|, |W2|, o1 through z,
    d_gamma through sum |g_t2| over those rows, the weight gradients through their operands t2 and h, d_x in second order.
    (With C = 256 the mean of a constant row is exact in every order, 3.5 * 256 and 1 / 256 being exact: the term is a formality.)"""
    if not c.const_rows.any():
        return {}
    xb = NC.xhat_const_bound()
    rowmask = torch.from_numpy(c.const_rows)[:, None].to(F64)
    s = NC.drop_scale(p)
    dt = xb * c.ln["f"][0].abs().to(F64)[None, :] * rowmask
    dh = s * (dt @ c.W["f1"].abs().to(F64).t())
    dz = dt + s * (dh @ c.W["f2"].abs().to(F64).t())
    gp = c.ln["fp"][0].abs().to(F64)
    tmax = float((ref["_g_t2"].abs() * c.ln["f"][0].abs().to(F64)).max())
    return {"z": dz, "o1": 2.0 * ref["_zrstd"] * gp[None, :] * dz.amax(1, keepdim=True),
            "d_g": xb * (ref["_g_t2"].abs() * rowmask).sum(0),
            "d_W1": (ref["_d_lin1"].abs() * rowmask).t() @ dt, "d_W2": (ref["_d_lin2"].abs() * rowmask).t() @ dh,
            "d_x": xb * xb / math.sqrt(NC.EPS) * tmax * rowmask}


# ---- references, yardsticks, groups ------------------------------------------------------------------------------------------------
EVAL_FN = {"qkv": qkv_eval, "proj_q": projq_eval, "ffn": ffn_eval, "ffn0": ffn0_eval}
_PARAM = ("d_W", "d_b", "d_g")   # parameter gradients add up every row: no row kinds


def _f64(res):
    return {k: v.to(F64) for k, v in res.items()}


def reference(c, launch, **kw):
    return _f64(EVAL_FN[launch](c, Ev(), **kw))


def restatements(c, launch, evals=EVALS, **kw):
    if launch == "qkv":  # no LayerNorm: one evaluation per contraction order
        evals = tuple({mm: (mm, o) for mm, o in evals}.values())
    return [_f64(EVAL_FN[launch](c, Ev(F32, mm, o), **kw)) for mm, o in evals]


def restate(c, launch, mm="mm", order="torch", defect=None, **kw):
    """ONE fp32 evaluation (a stand-in kernel: a held-out order, or a mutant)"""
    return _f64(EVAL_FN[launch](c, Ev(F32, mm, order, defect), **kw))


def groups_of(c, names):
    return {n: c.group for n in names if not n.startswith(_PARAM)}


# ---- ReLU margins ------------------------------------------------------------------------------------------------------------------
_GATES = (("ffn", "1", [dict(mode="drop"), dict(mode="p0")]), ("ffn0", "f1", [dict(p=P)]))   # ("eval" computes what "p0" computes)


def _ambiguous(c, launch, configs):
    amb = np.zeros((c.rows, C), dtype=bool)
    need = np.zeros((c.rows, C))
    for kw in configs:
        ref = reference(c, launch, **kw)["pre"]
        tol = NC.tolerance(ref, [r["pre"] for r in restatements(c, launch, **kw)], c.group)
        z = ref.numpy()
        a = np.abs(z) < tol
        need = np.where(a & ~amb, np.where(z >= 0, 1.0, -1.0) * (8 * tol - np.abs(z)), need)
        amb |= a
    return amb, need


def nudge(c):
    """Moves b1 of ffn and of ffn0, per column, until no fp64 pre-activation lies within its row kind's rule-tolerance of zero under
    any dropout configuration of the GPU file (to 8 tolerances, at most three trips); records the number of ambiguous elements left.
    Established on the reference alone."""
    left = {}
    for launch, bias, configs in _GATES:
        for trip in range(4):
            amb, need = _ambiguous(c, launch, configs)
            left[launch] = int(amb.sum())
            if left[launch] == 0 or trip == 3:
                break
            cols = np.nonzero(amb.any(0))[0]
            b = c.b[bias].to(F64).numpy().copy()
            for j in cols:  # the first ambiguous element of the column decides the direction; the next trip looks again
                i = int(np.argmax(amb[:, j]))
                b[j] += need[i, j]
            c.b[bias] = torch.from_numpy(b).to(F32)
    c.ambiguous = left
    return left


@functools.lru_cache(maxsize=None)
def case(nQ, B, seed=0):
    c = RbCase(nQ, B, seed)
    nudge(c)
    return c
