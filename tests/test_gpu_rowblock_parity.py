"""The decoder layer's row-block launches (csrc/rowblock.hip through rowblock.qkv / proj_q / ffn / ffn0 on a real GlobalDecoderLayer /
FFNLayer) against float64 references written out by formula, at every arm, tail block, scene count and mask: tests/rowblock_cases.py
holds the cases, the references, the fp32 yardstick and the arm lists; tests/test_rowblock_cases.py shows that the rule rejects subtly
wrong kernels.  The fused backward launches and the separate backward launches behind the fused forward (FUSED_BWD) are both held to
float64 (ffn0 has one backward only).

The keep masks are HOST masks (tests/drop_stream_restatement.py at the step's {seed, offset}, read back after reset_rng() /
begin_step()): the references never see a kernel's own mask.  The four masks are also read out of the launches bit for bit by a
choice of weights.  ffn0 draws both of its masks with one dropout module: its activation mask is read out where the residual mask
keeps (z = keep3 s3 * keepA sA), its residual mask everywhere.

`pytest -s` prints the measured kernel error / restatement error per arm and tensor."""
import functools
import itertools

import numpy as np
import pytest
import torch

import drop_stream_restatement as R
import norm_cases as NC
import rowblock_cases as RC
from helpers import args_ns

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = RC.C
RATIOS = {}  # arm -> tensor -> (kernel error, restatement error, factor used): the worst case of the arm
REACHED = {}  # arm -> the geometries (RC.arm_of) of the cases that ran it
ALN_SALTS = (RC.SALTS["drop1"], RC.SALTS["drop2"], RC.SALTS["drop3"])


@pytest.fixture(scope="module", autouse=True)
def _print_ratios():
    yield
    print("\narm | cases | tensor: kernel error / restatement error (factor of the rule it used; the rule allows %d)" % NC.FACTOR)
    for arm in sorted(RATIOS):
        by_use = sorted(RATIOS[arm].items(), key=lambda kv: -kv[1][2])
        print(f"{arm} | {'; '.join(sorted(REACHED[arm]))} | " + ", ".join(f"{n} {k:.1e} / {r:.1e} ({u:.2f})" for n, (k, r, u) in by_use))


@pytest.fixture(autouse=True)
def state(monkeypatch):
    """a fresh generator at the seed the cases' ReLU margins were established for; returns the unsigned {seed, offset} of the step"""
    from vdetr_amd import attention as A
    from vdetr_amd import heads as HD
    from vdetr_amd import vdetr_transformer as T
    monkeypatch.setitem(HD._fresh, "on", False)  # (no decoder forward here: ffn0 rewrites its own weight images)
    # the ~300 layers built here draw their attention salts from a counter of their own: the process-wide one, and with it the
    # dropout masks of every test that runs after this file, stay what they are without it (every salt used here is passed in)
    monkeypatch.setattr(T, "_salt_counter", itertools.count(1 << 20))
    torch.manual_seed(RC.STATE[0])
    A.reset_rng()
    A.begin_step(torch.device(DEV))
    s = tuple(int(v) & 0xFFFFFFFFFFFFFFFF for v in A.current_rng(torch.device(DEV)).cpu().tolist())
    assert s == RC.STATE, "the host masks of rowblock_cases are those of another step"
    return s


# ---- the modules, with the case's parameters copied in ---------------------------------------------------------------------------
def _put(param, value):
    with torch.no_grad():
        param.copy_(value.reshape(param.shape))


def _post(affine):
    m = torch.nn.LayerNorm(C, eps=NC.EPS).to(DEV)
    _put(m.weight, affine[0]), _put(m.bias, affine[1])
    return m


def _decoder_layer(c=None):
    from vdetr_amd.vdetr_transformer import GlobalDecoderLayer
    layer = GlobalDecoderLayer(d_model=C, nhead=4, dim_feedforward=C, dropout=RC.P, pos_for_key=False, args=args_ns()).to(DEV).train()
    assert layer.norm2.eps == layer.norm3.eps == NC.EPS
    if c is not None:
        sa, ca = layer.self_attn, layer.multihead_attn
        _put(sa.in_proj_weight, torch.cat([c.W[n] for n in "qkv"])), _put(sa.in_proj_bias, torch.cat([c.b[n] for n in "qkv"]))
        for lin, n in ((sa.out_proj, "o"), (ca.q, "c"), (ca.proj, "p"), (layer.linear1, "1"), (layer.linear2, "2")):
            _put(lin.weight, c.W[n]), _put(lin.bias, c.b[n])
        for ln, n in ((layer.norm2, "n2"), (layer.norm3, "n3")):
            _put(ln.weight, c.ln[n][0]), _put(ln.bias, c.ln[n][1])
    return layer


def _ffn_layer(p, c=None):
    from vdetr_amd.vdetr_transformer import FFNLayer
    layer = FFNLayer(C, dim_feedforward=C, dropout=p).to(DEV).train()
    assert layer.norm.eps == NC.EPS
    if c is not None:
        for lin, n in ((layer.linear1, "f1"), (layer.linear2, "f2")):
            _put(lin.weight, c.W[n]), _put(lin.bias, c.b[n])
        _put(layer.norm.weight, c.ln["f"][0]), _put(layer.norm.bias, c.ln["f"][1])
    return layer


def _set_p(layer, p):
    for m in (layer.dropout1, layer.dropout2, layer.dropout3, layer.dropout, layer.multihead_attn.proj_drop):
        m.p = p


def _seq(t, c, grad=True):
    """[rows, C] -> the sequence-first device tensor [nQ, B, C]"""
    return t.reshape(c.nQ, c.B, C).to(DEV).requires_grad_(grad)


def _bf(t, c, grad=False):
    return RC.to_bf(t, c.B).to(DEV).requires_grad_(grad)


def _rows(t, c, bf=False):
    if t is None:
        return None
    t = t.detach()
    return (RC.from_bf(t, c.B) if bf else t.reshape(c.rows, C)).cpu()


@functools.lru_cache(maxsize=2)
def _yardstick(launch, shape, kw_items):
    """the float64 reference and the fp32 restatements of one (launch, case, arm): shared by the fused and the unfused run"""
    c, kw = RC.case(*shape), dict(kw_items)
    ref = RC.reference(c, launch, **kw)
    return ref, RC.restatements(c, launch, **kw), (RC.ffn0_extra(c, ref, kw.get("p", RC.P)) if launch == "ffn0" else None)


def _compare(got, launch, shape, kw, names, label):
    c = RC.case(*shape)
    ref, rests, extra = _yardstick(launch, shape, tuple(sorted(kw.items())))
    missing = [n for n in names if got.get(n) is None]
    assert not missing, f"{label}: no {missing}"
    REACHED.setdefault(label, set()).add(RC.arm_of(shape)["label"])
    NC.compare(got, ref, rests, names, RC.groups_of(c, names), extra, label=label, ratios=RATIOS)
    return ref


def _fused(monkeypatch, fused):
    from vdetr_amd import rowblock as RB
    monkeypatch.setattr(RB, "FUSED_BWD", fused)
    return "fused bwd" if fused else "separate bwd"


# ---- qkv ---------------------------------------------------------------------------------------------------------------------------
def _qkv_run(c, pos, pos_grad, alias, use):
    from vdetr_amd import rowblock as RB
    layer = _decoder_layer(c)
    sa = layer.self_attn
    t = _seq(c.tgt, c)
    pos_t = _seq(c.pos, c, pos_grad) if pos else None
    q, k, v, al = RB.qkv(t, pos_t, sa, c.B, RB.images(layer))
    assert q.shape == (c.B, c.nQ, C) and (al is None) == (not pos)
    outs = {"q": q, "k": k, "v": v}
    loss = sum((outs[n] * _bf(c.d[n], c)).sum() for n in use)
    if alias:
        loss = loss + (al * _seq(c.d["alias"], c, False)).sum()
    loss.backward()
    got = {n: _rows(outs[n], c, True) for n in "qkv"}
    got["d_t"] = _rows(t.grad, c)
    if pos and pos_grad:
        got["d_pos"] = _rows(pos_t.grad, c)
    gw, gb = sa.in_proj_weight.grad.view(3, C, C), sa.in_proj_bias.grad.view(3, C)
    for i, n in enumerate("qkv"):
        got["d_W" + n], got["d_b" + n] = gw[i], gb[i]
    return got


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("shape,pos,pos_grad,alias,use", RC.QKV_ARMS, ids=lambda v: str(v).replace(" ", ""))
def test_qkv_matches_fp64(monkeypatch, shape, pos, pos_grad, alias, use, fused):
    how = _fused(monkeypatch, fused)
    arm = ("no pos" if not pos else "pos without grad" if not pos_grad else "pos + d_alias" if alias else "pos, no d_alias") + f", loss on {use}"
    got = _qkv_run(RC.case(*shape), pos, pos_grad, alias, use)
    _compare(got, "qkv", shape, dict(pos=pos, alias=alias, use=use), RC.qkv_names(pos, pos_grad), f"qkv | {arm} | {how}")
    for n in "qkv":  # a gradient that never arrived is a zero operand, not an omitted one
        if n not in use:
            assert float(got["d_W" + n].abs().max()) == 0 and float(got["d_b" + n].abs().max()) == 0


# ---- proj_q ------------------------------------------------------------------------------------------------------------------------
def _projq_run(c, p, pos, use, a_grad, a_rows=None):
    from vdetr_amd import rowblock as RB
    layer = _decoder_layer(c)
    _set_p(layer, p)
    sa, ca = layer.self_attn, layer.multihead_attn
    a = _bf(c.a if a_rows is None else a_rows, c, a_grad)
    tgt = _seq(c.tgt, c)
    pos_t = _seq(c.pos, c) if pos else None
    y, q = RB.proj_q(a, tgt, pos_t, sa.out_proj, ca.q, layer.dropout1, layer.norm2, RC.SALTS["drop1"], c.B, RB.images(layer))
    assert y.shape == (c.nQ, c.B, C) and q.shape == (c.B, c.nQ, C)
    loss = 0
    if "y" in use:
        loss = loss + (y * _seq(c.d["y"], c, False)).sum()
    if "q" in use:
        loss = loss + (q * _bf(c.d["qout"], c)).sum()
    loss.backward()
    return {"y": _rows(y, c), "q": _rows(q, c, True), "d_a": _rows(a.grad, c, True), "d_tgt": _rows(tgt.grad, c),
            "d_pos": _rows(pos_t.grad, c) if pos else None, "d_Wo": sa.out_proj.weight.grad, "d_bo": sa.out_proj.bias.grad,
            "d_Wc": ca.q.weight.grad, "d_bc": ca.q.bias.grad, "d_g2": layer.norm2.weight.grad, "d_be2": layer.norm2.bias.grad}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("shape,p,pos,use,a_grad", RC.PROJQ_ARMS, ids=lambda v: str(v).replace(" ", ""))
def test_proj_q_matches_fp64(monkeypatch, shape, p, pos, use, a_grad, fused):
    how = _fused(monkeypatch, fused)
    arm = f"p {p}, {'pos' if pos else 'no pos'}, loss on {use}" + ("" if a_grad else ", a without grad")
    got = _projq_run(RC.case(*shape), p, pos, use, a_grad)
    _compare(got, "proj_q", shape, dict(p=p, pos=pos, use=use), RC.projq_names(pos, use, a_grad), f"proj_q | {arm} | {how}")
    if not a_grad:
        assert got["d_a"] is None
    if "q" not in use:
        assert got["d_Wc"] is None and got["d_pos"] is None


# ---- ffn ---------------------------------------------------------------------------------------------------------------------------
def _ffn_run(c, mode, two, use, a_rows=None):
    from vdetr_amd import rowblock as RB
    layer = _decoder_layer(c)
    _set_p(layer, 0.0 if mode == "p0" else RC.P)
    layer.train(mode != "eval")
    posts = [_post(c.ln["p1"])] + ([_post(c.ln["p2"])] if two else [])
    a = _bf(c.a if a_rows is None else a_rows, c, True)
    tgt = _seq(c.tgt, c)
    z, o1, o2 = RB.ffn(a, tgt, layer, posts, ALN_SALTS, RC.SALTS["act"], c.B, RB.images(layer))
    assert (o2 is None) == (not two)
    outs = {"z": (z, "z"), "1": (o1, "o1"), "2": (o2, "o2")}
    loss = sum((outs[n][0] * _seq(c.d[outs[n][1]], c, False)).sum() for n in use)
    loss.backward()
    ca = layer.multihead_attn
    got = {"z": _rows(z, c), "o1": _rows(o1, c), "o2": _rows(o2, c), "d_a": _rows(a.grad, c, True), "d_tgt": _rows(tgt.grad, c),
           "d_Wp": ca.proj.weight.grad, "d_bp": ca.proj.bias.grad, "d_W1": layer.linear1.weight.grad, "d_b1": layer.linear1.bias.grad,
           "d_W2": layer.linear2.weight.grad, "d_b2": layer.linear2.bias.grad, "d_g3": layer.norm3.weight.grad, "d_be3": layer.norm3.bias.grad,
           "d_gp1": posts[0].weight.grad, "d_bp1": posts[0].bias.grad}
    if two:
        got["d_gp2"], got["d_bp2"] = posts[1].weight.grad, posts[1].bias.grad
    return got


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("shape,mode,two,use", RC.FFN_ARMS, ids=lambda v: str(v).replace(" ", ""))
def test_ffn_matches_fp64(monkeypatch, shape, mode, two, use, fused):
    how = _fused(monkeypatch, fused)
    arm = {"drop": "p 0.1 (p2 composite)", "p0": "p 0", "eval": "eval"}[mode] + f", {'two norms' if two else 'one norm'}, loss on {use}"
    got = _ffn_run(RC.case(*shape), mode, two, use)
    _compare(got, "ffn", shape, dict(mode=mode, two=two, use=use), RC.ffn_names(two), f"ffn | {arm} | {how}")
    if "1" not in use:
        assert float(got["d_gp1"].abs().max()) == 0 and float(got["d_bp1"].abs().max()) == 0
    if two and "2" not in use:
        assert float(got["d_gp2"].abs().max()) == 0 and float(got["d_bp2"].abs().max()) == 0


# ---- ffn0 --------------------------------------------------------------------------------------------------------------------------
def _ffn0_run(c, p, use):
    from vdetr_amd import rowblock as RB
    layer = _ffn_layer(p, c)
    layer.post_norm = _post(c.ln["fp"])
    x = _seq(c.x0, c)
    z, o1 = RB.ffn0(layer, x, RC.SALTS["ffn0_act"], RC.SALTS["ffn0_res"])
    outs = {"z": (z, "fz"), "1": (o1, "fo1")}
    loss = sum((outs[n][0] * _seq(c.d[outs[n][1]], c, False)).sum() for n in use)
    loss.backward()
    return {"z": _rows(z, c), "o1": _rows(o1, c), "d_x": _rows(x.grad, c), "d_W1": layer.linear1.weight.grad, "d_b1": layer.linear1.bias.grad,
            "d_W2": layer.linear2.weight.grad, "d_b2": layer.linear2.bias.grad, "d_g": layer.norm.weight.grad, "d_be": layer.norm.bias.grad,
            "d_gp": layer.post_norm.weight.grad, "d_bep": layer.post_norm.bias.grad}


@pytest.mark.parametrize("shape,p,use", RC.FFN0_ARMS, ids=lambda v: str(v).replace(" ", ""))
def test_ffn0_matches_fp64(shape, p, use):
    got = _ffn0_run(RC.case(*shape), p, use)
    _compare(got, "ffn0", shape, dict(p=p, use=use), RC.FFN0_NAMES, f"ffn0 | p {p}, loss on {use}")
    if "1" not in use:
        assert float(got["d_gp"].abs().max()) == 0 and float(got["d_bep"].abs().max()) == 0


# ---- forward and backward agree on the masks: exact zeros ------------------------------------------------------------------------------
def _one_hot(c):
    a = torch.zeros(c.rows, C)
    a[torch.arange(c.rows), torch.arange(c.rows)] = 1.0
    return a


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("shape", [(17, 1), (11, 3)], ids=str)
def test_branch_gradient_is_exactly_zero_where_the_branch_was_dropped(monkeypatch, shape, fused):
    """with one-hot rows of `a` (row r = unit vector r) the weight gradient dW = d_proj^T a holds d_proj itself, exactly: column r of
    dW is row r of d_proj.  It must be 0 where the host mask drops the element and (almost surely) non-zero where it keeps it."""
    _fused(monkeypatch, fused)
    c = RC.case(*shape)
    for launch, keep, dW in (("proj_q", c.keep("drop1", RC.P), _projq_run(c, RC.P, True, "yq", True, _one_hot(c))["d_Wo"]),
                             ("ffn", c.keep("drop2", RC.P2), _ffn_run(c, "drop", True, "z12", _one_hot(c))["d_Wp"])):
        d_proj = dW.detach().cpu()[:, :c.rows].t()
        assert float(dW.detach().cpu()[:, c.rows:].abs().max()) == 0, launch
        assert bool((d_proj[keep == 0] == 0).all()), launch
        assert float((d_proj[keep == 1] != 0).double().mean()) > 0.99, launch


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_lone_row_bias_gradients_are_exactly_zero_where_the_masks_drop(monkeypatch, fused):
    """one row: a bias gradient IS that row of d_lin2 / d_lin1 / d_proj"""
    _fused(monkeypatch, fused)
    c = RC.case(1, 1)
    got = _ffn_run(c, "drop", True, "z12")
    ref = RC.reference(c, "ffn", mode="drop")
    for name, dead in (("d_b2", c.keep("drop3", RC.P) == 0), ("d_bp", c.keep("drop2", RC.P2) == 0),
                       ("d_b1", (c.keep("act", RC.P) == 0) | (ref["pre"] <= 0))):
        g = got[name].detach().cpu()
        assert bool((g[dead[0]] == 0).all()) and float((g[~dead[0]] != 0).double().mean()) > 0.99, name
    got = _ffn0_run(c, RC.P, "z1")
    ref = RC.reference(c, "ffn0", p=RC.P)
    for name, dead in (("d_b2", c.keep("ffn0_res", RC.P) == 0), ("d_b1", (c.keep("ffn0_act", RC.P) == 0) | (ref["pre"] <= 0))):
        g = got[name].detach().cpu()
        assert bool((g[dead[0]] == 0).all()) and float((g[~dead[0]] != 0).double().mean()) > 0.99, name


# ---- the masks themselves, read out of the launches bit for bit ------------------------------------------------------------------------
def _scale32(p):
    return np.float32(65536.0) / np.float32(65536 - NC.drop_threshold(p))


def _same_mask(y, want, scale):
    y = y.detach().reshape(want.shape).cpu()
    assert torch.equal(y > 0, torch.from_numpy(np.ascontiguousarray(want)))
    assert torch.equal(y[y > 0], torch.full_like(y[y > 0], float(scale)))


def _readout_layer(lins):
    """a decoder layer with all-zero projections except `lins`: {attribute path: (weight or None for zeros, bias value)}"""
    layer = _decoder_layer()
    sa, ca = layer.self_attn, layer.multihead_attn
    mods = {"o": sa.out_proj, "p": ca.proj, "1": layer.linear1, "2": layer.linear2}
    with torch.no_grad():
        for n, m in mods.items():
            w, b = lins.get(n, (None, 0.0))
            m.weight.zero_() if w is None else m.weight.copy_(w)
            m.bias.fill_(b)
    return layer


@pytest.mark.parametrize("nQ,B", [(17, 1), (11, 3)])
def test_the_four_masks_are_the_host_masks_bit_for_bit(state, nQ, B):
    from vdetr_amd import rowblock as RB
    rows, p = nQ * B, RC.P
    zeros_seq, zeros_bf = torch.zeros(nQ, B, C, device=DEV), torch.zeros(B, nQ, C, device=DEV)
    posts = [torch.nn.LayerNorm(C).to(DEV)]
    eye = torch.eye(C)
    # drop1 through proj_q: a = 0, tgt = 0, bo = 1 -> y = keep1 s1
    layer = _readout_layer({"o": (None, 1.0)})
    y, _ = RB.proj_q(zeros_bf, zeros_seq, None, layer.self_attn.out_proj, layer.multihead_attn.q, layer.dropout1, layer.norm2,
                     RC.SALTS["drop1"], B, RB.images(layer))
    _same_mask(y, R.keep_add_ln(rows, C, p, R.stream(RC.SALTS["drop1"], 0, state)), _scale32(p))
    # drop2 through ffn: bp = 1, W2 = 0, b2 = 0 -> z = y = keep2 s2, the composite of dropout2 and proj_drop
    layer = _readout_layer({"p": (None, 1.0)})
    z = RB.ffn(zeros_bf, zeros_seq, layer, posts, ALN_SALTS, RC.SALTS["act"], B, RB.images(layer))[0]
    _same_mask(z, R.keep_add_ln(rows, C, RC.P2, R.stream(RC.SALTS["drop2"], 0, state)), _scale32(RC.P2))
    # drop3: bp = 0, W2 = 0, b2 = 1 -> z = keep3 s3
    layer = _readout_layer({"2": (None, 1.0)})
    z = RB.ffn(zeros_bf, zeros_seq, layer, posts, ALN_SALTS, RC.SALTS["act"], B, RB.images(layer))[0]
    _same_mask(z, R.keep_add_ln(rows, C, p, R.stream(RC.SALTS["drop3"], 0, state)), _scale32(p))
    # the activation's: dropout2 = dropout3 = proj_drop = 0, W1 = 0, b1 = 1, W2 = I -> z = h = keepA sA
    layer = _readout_layer({"1": (None, 1.0), "2": (eye, 0.0)})
    layer.dropout2.p = layer.dropout3.p = layer.multihead_attn.proj_drop.p = 0.0
    z = RB.ffn(zeros_bf, zeros_seq, layer, posts, ALN_SALTS, RC.SALTS["act"], B, RB.images(layer))[0]
    _same_mask(z, R.keep_flat(rows * C, p, R.stream(RC.SALTS["act"], 0, state)).reshape(rows, C), _scale32(p))


@pytest.mark.parametrize("nQ,B", [(17, 1), (11, 3)])
def test_ffn0_masks_are_the_host_masks_bit_for_bit(state, nQ, B):
    from vdetr_amd import rowblock as RB
    rows, p = nQ * B, RC.P
    keep3 = R.keep_add_ln(rows, C, p, R.stream(RC.SALTS["ffn0_res"], 0, state))
    keepA = R.keep_flat(rows * C, p, R.stream(RC.SALTS["ffn0_act"], 0, state)).reshape(rows, C)
    x = torch.zeros(nQ, B, C, device=DEV)

    def layer_with(w2, b2):
        layer = _ffn_layer(p)
        layer.post_norm = torch.nn.LayerNorm(C).to(DEV)
        with torch.no_grad():  # norm: weight 1, bias 0 on x = 0 -> t2 = 0;  W1 = 0, b1 = 1 -> the pre-activation is 1
            layer.linear1.weight.zero_(), layer.linear1.bias.fill_(1.0)
            layer.linear2.weight.copy_(w2), layer.linear2.bias.fill_(b2)
        return layer
    # the residual mask: W2 = 0, b2 = 1 -> z = keep3 s3
    z, _ = RB.ffn0(layer_with(torch.zeros(C, C), 1.0), x, RC.SALTS["ffn0_act"], RC.SALTS["ffn0_res"])
    _same_mask(z, keep3, _scale32(p))
    # the activation's, where the residual mask keeps: W2 = I, b2 = 0 -> z = keep3 s3 (keepA sA)
    z, _ = RB.ffn0(layer_with(torch.eye(C), 0.0), x, RC.SALTS["ffn0_act"], RC.SALTS["ffn0_res"])
    _same_mask(z, keep3 & keepA, _scale32(p) * _scale32(p))
    assert int((keep3 & ~keepA).sum()) > 0 and int((~keep3 & keepA).sum()) > 0
