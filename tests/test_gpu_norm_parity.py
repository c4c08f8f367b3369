"""The dense norm launches (add_ln.hip, bn_act.hip, relu_dropout) against float64 references written out by formula, at every
dispatch arm, edge shape and bad statistic (large means, variance far below eps, constant rows): tests/norm_cases.py holds the
cases, the references and the tolerance rule; tests/test_norm_cases.py shows that the rule rejects subtly wrong kernels.
Keep masks are read back from the kernels (LayerNorm: x = 0, r = 1; BatchNorm: gamma = 1, beta = 10 on x = 0) and tested on
their own further down.  `pytest -s` prints the measured kernel error / restatement error per arm and tensor."""

import numpy as np
import pytest
import torch

import norm_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL3 = ("d_y", "d_out", "d_out2")
RATIOS = {}  # arm -> tensor -> (kernel error, restatement error, factor used): the worst case of the arm


@pytest.fixture(scope="module", autouse=True)
def _print_ratios():
    yield
    print("\narm | tensor: kernel error / restatement error (factor of the rule it used; the rule allows %d)" % NC.FACTOR)
    for arm in sorted(RATIOS):
        worst = {}
        for n, v in RATIOS[arm].items():
            n = n[-1] if isinstance(n, tuple) else n  # (the parked sums are keyed by (norm, tensor))
            worst[n] = max(worst.get(n, (0.0, 0.0, 0.0)), v, key=lambda t: t[2])
        print(f"{arm} | " + ", ".join(f"{n} {k:.1e} / {r:.1e} ({u:.2f})" for n, (k, r, u) in worst.items()))


@pytest.fixture(autouse=True)
def _fresh_rng():
    from vdetr_amd import attention as A
    A.reset_rng()
    A.begin_step(torch.device(DEV))


def bn_arm(B, N, aligned=True):
    """the dispatch rule of vdetr_bn_act_{fwd,bwd}_f32, restated (labels of the ratio table)"""
    tot = B * N
    if not (N % 4 == 0 and tot % 256 == 0 and aligned):
        return "bn sweep (odd)" if tot > 1 else "bn sweep (n = 1)"
    if tot > 4096:
        return "bn sweep (> 4096)"
    return f"bn reg<{tot // 256}>" if tot // 256 in (1, 2, 4, 8, 16) else "bn sweep (hole)"


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
def _ln_modules(c, dual):
    mods = []
    for ga, be in ((c.gamma, c.beta), (c.gamma2, c.beta2))[:2 if dual else 1]:
        m = torch.nn.LayerNorm(c.C, eps=NC.EPS)
        with torch.no_grad():
            m.weight.copy_(ga), m.bias.copy_(be)
        mods.append(m.to(DEV))
    return mods + [None] * (2 - len(mods))


def _ln_keep(rows, C, drop, salt, also_drop=None):
    """the kernel's own keep mask: x = 0, r = 1 -> y = keep * scale"""
    from vdetr_amd import add_ln as ALN
    ln = torch.nn.LayerNorm(C).to(DEV)
    y0 = ALN.add_dropout_layer_norm(torch.zeros(rows, C, device=DEV), torch.ones(rows, C, device=DEV), drop, ln, salt=salt,
                                    also_drop=also_drop)[0]
    return (y0.detach() > 0).double().cpu(), y0.detach().cpu()


def _ln_run(c, dual, p, has_r, subset, salt, drop=None, also_drop=None, mods=None):
    from vdetr_amd import add_ln as ALN
    ln, ln2 = mods if mods is not None else _ln_modules(c, dual)
    x = c.x.to(DEV).requires_grad_(True)
    got = {}
    if has_r:
        r = c.r.to(DEV).requires_grad_(True)
        if drop is None and p > 0:
            drop = torch.nn.Dropout(p).train()
        outs = ALN.add_dropout_layer_norm(x, r, drop, ln, ln2, salt=salt, also_drop=also_drop)
        got["y"], got["out"] = outs[0], outs[1]
        if dual:
            got["out2"] = outs[2]
    else:
        outs = ALN.layer_norm(x, ln, ln2)
        got["out"] = outs[0] if dual else outs
        if dual:
            got["out2"] = outs[1]
    ups = {"d_y": "y", "d_out": "out", "d_out2": "out2"}
    loss = sum((got[ups[k]] * getattr(c, k).to(DEV)).sum() for k in subset if ups[k] in got)
    loss.backward()
    got["d_x"] = x.grad
    if has_r:
        got["d_r"] = r.grad
    got["d_gamma"], got["d_beta"] = ln.weight.grad, ln.bias.grad
    if dual:
        got["d_gamma2"], got["d_beta2"] = ln2.weight.grad, ln2.bias.grad
    return {k: v.detach() for k, v in got.items() if v is not None}  # (parked parameter sums: no .grad yet)


def _ln_names(dual, has_r):
    return (["y", "d_r"] if has_r else []) + ["out", "d_x", "d_gamma", "d_beta"] + (["out2", "d_gamma2", "d_beta2"] if dual else [])


def _ln_check(c, dual, p, has_r, subset=ALL3, salt=1234, label=None, pref=None, drop=None, also_drop=None):
    """runs the wrappers on the case and holds every tensor against the float64 reference; `pref`: the p of the reference
    (the composite probability with `also_drop`)"""
    pref = p if pref is None else pref
    keep = None
    if pref > 0:
        keep, _ = _ln_keep(c.rows, c.C, drop if drop is not None else torch.nn.Dropout(p).train(), salt, also_drop)
    got = _ln_run(c, dual, p, has_r, subset, salt, drop, also_drop)
    ref = NC.ln_eval(c, keep, pref, subset, has_r=has_r, dual=dual)
    rests = NC.ln_restatements(c, keep, pref, subset, has_r=has_r, dual=dual)
    groups, extra = NC.ln_groups_and_extra(c, ref, subset, dual)
    NC.compare(got, ref, rests, _ln_names(dual, has_r), groups, extra, label=label or f"ln C = {c.C}", ratios=RATIOS)
    if pref > 0:  # forward and backward agree on the mask: the branch gradient is exactly 0 where the branch was dropped
        d_r = got["d_r"].cpu()
        assert bool((d_r[keep == 0] == 0).all()) and float((d_r[keep == 1] != 0).double().mean()) > 0.99
    return got, ref, keep


@pytest.mark.parametrize("rows,C,dual,p,has_r", NC.LN_CASES)
def test_layer_norm_matches_fp64(rows, C, dual, p, has_r):
    _ln_check(NC.ln_case(rows, C), dual, p, has_r)


@pytest.mark.parametrize("subset", NC.LN_SUBSETS, ids=["+".join(s) for s in NC.LN_SUBSETS])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_layer_norm_gradient_subsets(subset, p):
    got, _, _ = _ln_check(NC.ln_case(33, 512), True, p, True, subset)
    if "d_out" not in subset:
        assert float(got["d_gamma"].abs().max()) == 0 and float(got["d_beta"].abs().max()) == 0
    if "d_out2" not in subset:
        assert float(got["d_gamma2"].abs().max()) == 0 and float(got["d_beta2"].abs().max()) == 0


def test_layer_norm_also_drop_is_one_composite_mask():
    rows, C, p1, p2 = 1024, 256, 0.1, 0.2
    pc = NC.composite_p(p1, p2)
    drop, also = torch.nn.Dropout(p1).train(), torch.nn.Dropout(p2).train()
    keep, y0 = _ln_keep(rows, C, drop, 77, also)
    q = NC.keep_prob(pc)
    assert abs(q - (1 - p1) * (1 - p2)) < 2.0 ** -16
    assert abs(float(keep.mean()) - q) <= 5 * NC.keep_sigma(pc, rows * C)
    np.testing.assert_allclose(y0.double().numpy(), (keep * NC.drop_scale(pc)).numpy(), rtol=2.0 ** -23)  # the composite scale
    _ln_check(NC.ln_case(33, 256), True, p1, True, salt=78, pref=pc, drop=drop, also_drop=also, label="ln also_drop")
    # an eval-mode second dropout leaves the first one alone
    _ln_check(NC.ln_case(33, 256), False, p1, True, salt=79, pref=p1, drop=drop, also_drop=torch.nn.Dropout(p2).eval())


def test_layer_norm_eval_mode_dropout_takes_the_p0_path():
    c = NC.ln_case(17, 768)
    got, ref, _ = _ln_check(c, True, 0.3, True, pref=0.0, drop=torch.nn.Dropout(0.3).eval(), label="ln eval dropout")
    assert torch.equal(got["y"].cpu(), c.x + c.r) and torch.equal(got["d_r"], got["d_x"])


def test_layer_norm_parked_sums_match_fp64_and_the_immediate_mode():
    """35 parked backward passes (vdetr_add_ln_param_reduce_batch_f32 takes 32 per launch), widths 256 / 512 / 1024 in one
    flush, groups of passes sharing their first LayerNorm, one dual pass without d_out2 (not parked: summed in its backward)"""
    from vdetr_amd import add_ln as ALN
    from vdetr_amd import runtime
    passes = []
    shared = {}
    for i, (rows, C, dual, first, has_r) in enumerate(NC.LN_DEFERRED):
        c = NC.LnCase(rows, C, seed=100 + i, shift=i)
        if first not in shared:
            shared[first] = (c.gamma, c.beta)
        c.gamma, c.beta = shared[first]
        subset = ("d_y", "d_out") if i == 5 else ALL3
        passes.append((c, dual, first, has_r, subset))
    assert passes[5][1]
    names = ("d_gamma", "d_beta", "d_gamma2", "d_beta2")
    ref, rests, extra = {}, [dict() for _ in NC.ORDERS], {}

    def add(dst, key, t):
        dst[key] = dst[key] + t if key in dst else t.clone()
    for i, (c, dual, first, has_r, subset) in enumerate(passes):
        e = NC.ln_eval(c, None, 0.0, subset, has_r=has_r, dual=dual)
        rs = NC.ln_restatements(c, None, 0.0, subset, has_r=has_r, dual=dual)
        _, ex = NC.ln_groups_and_extra(c, e, subset, dual)
        for n in names[:4 if dual else 2]:
            key = (first, n) if n in ("d_gamma", "d_beta") else (("second", i), n)
            add(ref, key, e[n])
            for dst, r in zip(rests, rs):
                add(dst, key, r[n])
            if n in ex:
                add(extra, key, ex[n])
    res = {}
    for defer in (False, True):
        firsts = {}
        params = {}
        runtime.defer_weight_grads(defer)
        try:
            for i, (c, dual, first, has_r, subset) in enumerate(passes):
                ln, ln2 = _ln_modules(c, dual)
                ln = firsts.setdefault(first, ln)
                _ln_run(c, dual, 0.0, has_r, subset, 0, mods=(ln, ln2))
                params[(first, "d_gamma")], params[(first, "d_beta")] = ln.weight, ln.bias
                if dual:
                    params[(("second", i), "d_gamma2")], params[(("second", i), "d_beta2")] = ln2.weight, ln2.bias
            if defer:
                assert len(ALN.DeferredLnGrads.pending) == len(passes) - 1 == 35
                runtime.flush_weight_grads()
                assert not ALN.DeferredLnGrads.pending
        finally:
            runtime.defer_weight_grads(False)
        res[defer] = {k: p.grad.detach().clone() for k, p in params.items()}
    assert set(res[True]) == set(ref)
    for defer in (False, True):
        NC.compare(res[defer], ref, rests, list(ref), None, extra, label="ln parked sums" if defer else "ln immediate sums",
                   ratios=RATIOS)


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------------
BN_NAMES = ["y", "dx", "d_gamma", "d_beta", "running_mean", "running_var"]


def _misaligned(t):
    """a contiguous copy of t that starts 4 bytes off a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _bn_keep(B, C, N, p, salt):
    """the kernel's own keep mask: gamma = 1, beta = 10 on x = 0 -> y = 10 keep scale"""
    from vdetr_amd.bn_act import bn_act
    y0 = bn_act(torch.zeros(B, C, N, device=DEV), torch.ones(C, device=DEV), torch.full((C,), 10.0, device=DEV), None, None, True,
                NC.EPS, NC.MOMENTUM, relu=True, dropout_p=p, salt=salt)
    return (y0 > 0).double().cpu()


def _bn_run(c, p, relu, affine_on, pre_bias, salt, misalign_x=False, misalign_dy=False):
    from vdetr_amd.bn_act import bn_act
    x = (_misaligned(c.x) if misalign_x else c.x.to(DEV)).detach().requires_grad_(True)
    w = c.gamma.to(DEV).requires_grad_(True) if affine_on else None
    b = c.beta.to(DEV).requires_grad_(True) if affine_on else None
    rm, rv = c.rm0.clone().to(DEV), c.rv0.clone().to(DEV)
    dy = _misaligned(c.dy) if misalign_dy else c.dy.to(DEV)
    assert (x.data_ptr() % 16 != 0) == misalign_x and (dy.data_ptr() % 16 != 0) == misalign_dy
    y = bn_act(x, w, b, rm, rv, True, NC.EPS, NC.MOMENTUM, relu=relu, dropout_p=p, salt=salt,
               pre_bias=c.pre_bias.to(DEV) if pre_bias else None)
    y.backward(gradient=dy)
    got = {"y": y.detach(), "dx": x.grad, "running_mean": rm, "running_var": rv}
    if affine_on:
        got["d_gamma"], got["d_beta"] = w.grad, b.grad
    return got


def _bn_reference(c, keep, p, relu=True, affine_on=True, pre_bias=False):
    kw = dict(relu=relu, affine_on=affine_on, pre_bias=pre_bias)
    ref = NC.bn_eval(c, keep, p, **kw)
    rests = NC.bn_restatements(c, keep, p, **kw)
    groups, extra = NC.bn_groups_and_extra(c, p, True, affine_on)
    return ref, rests, groups, extra


def _bn_check(B, C, N, p, relu=True, affine_on=True, pre_bias=False, salt=77, label=None, **run_kw):
    c = NC.bn_case(B, C, N, True, affine_on, pre_bias)
    keep = _bn_keep(B, C, N, p, salt) if p > 0 else None
    got = _bn_run(c, p, relu, affine_on, pre_bias, salt, **run_kw)
    ref, rests, groups, extra = _bn_reference(c, keep, p, relu, affine_on, pre_bias)
    names = BN_NAMES if affine_on else [n for n in BN_NAMES if n not in ("d_gamma", "d_beta")]
    NC.compare(got, ref, rests, names, groups, extra, label=label or bn_arm(B, N), ratios=RATIOS)
    return got, ref, keep


@pytest.mark.parametrize("p", NC.BN_P)
@pytest.mark.parametrize("B,C,N", NC.BN_CASES)
def test_bn_act_matches_fp64(B, C, N, p):
    _bn_check(B, C, N, p)


@pytest.mark.parametrize("B,C,N,relu,p,affine_on,pre_bias", NC.BN_VARIANTS)
def test_bn_act_variants_match_fp64(B, C, N, relu, p, affine_on, pre_bias):
    """relu=False with dropout, gamma=None, pre_bias: each on a register arm and on a sweep arm"""
    _bn_check(B, C, N, p, relu, affine_on, pre_bias)


def test_bn_act_crossed_arms_regenerate_the_same_mask():
    """The forward picks its arm from the alignment of x / y, the backward from x / dy / dx: a sweep on one side and a register
    arm on the other must draw the same mask from the flat (b N + i) index.  A misaligned x sends BOTH launches to the sweep
    (the backward reads x too); the sweep forward in front of a register backward is reached through forward_record's y_out."""
    from vdetr_amd import bn_act as BNA
    B, C, N = NC.BN_CROSSED
    p, salt = 0.3, 4321
    c = NC.bn_case(B, C, N)
    base, ref, keep = _bn_check(B, C, N, p, salt=salt)
    zeros = base["y"] == 0
    assert 0.2 < float(zeros.double().mean()) < 0.9
    for kw, label in ((dict(misalign_x=True), "bn sweep (misaligned x)"), (dict(misalign_dy=True), "bn reg<4> fwd, sweep bwd")):
        got, _, _ = _bn_check(B, C, N, p, salt=salt, label=label, **kw)
        assert torch.equal(got["y"] == 0, zeros)
    # sweep forward (y off the boundary), register backward
    y_out = _misaligned(torch.zeros(B, C, N))
    rm, rv = c.rm0.clone().to(DEV), c.rv0.clone().to(DEV)
    y, rec = BNA.forward_record(c.x.to(DEV), c.gamma.to(DEV), c.beta.to(DEV), rm, rv, NC.EPS, NC.MOMENTUM, p, salt, y_out=y_out)
    assert y.data_ptr() % 16 != 0 and rec[0].data_ptr() % 16 == 0
    dx, dg, db = BNA.backward_from_record(rec, c.dy.to(DEV))
    got = {"y": y, "dx": dx, "d_gamma": dg, "d_beta": db, "running_mean": rm, "running_var": rv}
    _, rests, groups, extra = _bn_reference(c, keep, p)
    NC.compare(got, ref, rests, BN_NAMES, groups, extra, label="bn sweep fwd, reg<4> bwd", ratios=RATIOS)
    assert torch.equal(y == 0, zeros)


@pytest.mark.parametrize("B,C,N,relu,affine_on", NC.BN_EVAL)
def test_bn_act_eval_mode_matches_fp64(B, C, N, relu, affine_on):
    from vdetr_amd.bn_act import bn_act
    c = NC.bn_case(B, C, N, False, affine_on, True)
    rm, rv = c.rm0.clone().to(DEV), c.rv0.clone().to(DEV)
    y = bn_act(c.x.to(DEV), c.gamma.to(DEV) if affine_on else None, c.beta.to(DEV) if affine_on else None, rm, rv, False, NC.EPS,
               NC.MOMENTUM, relu=relu, pre_bias=c.pre_bias.to(DEV))
    kw = dict(training=False, relu=relu, affine_on=affine_on, pre_bias=True)
    ref = NC.bn_eval(c, None, 0.0, False, **kw)
    rests = NC.bn_restatements(c, None, 0.0, False, **kw)
    NC.compare({"y": y}, ref, rests, ["y"], {"y": c.group}, label="bn eval", ratios=RATIOS)
    assert torch.equal(rm.cpu(), c.rm0) and torch.equal(rv.cpu(), c.rv0)


def test_bn_act_backward_from_records_matches_fp64():
    """vdetr_bn_act_bwd_batch_f32: 14 records are two launches (12 per launch) of a register arm with C = 5 / 64 / 70 under one
    grid sized by the largest; a second call with B N = 130 takes the batched sweep"""
    from vdetr_amd import bn_act as BNA
    for shapes, label in zip(NC.BN_RECORDS, ("bn batch reg<2>", "bn batch sweep")):
        recs, dys, dxs, meta = [], [], [], []
        for i, (B, C, N) in enumerate(shapes):
            c = NC.bn_case(B, C, N)
            p, salt = (0.3, 900 + i) if i % 2 == 0 else (0.0, 0)
            keep = _bn_keep(B, C, N, p, salt) if p > 0 else None
            rm, rv = c.rm0.clone().to(DEV), c.rv0.clone().to(DEV)
            y, rec = BNA.forward_record(c.x.to(DEV), c.gamma.to(DEV), c.beta.to(DEV), rm, rv, NC.EPS, NC.MOMENTUM, p, salt)
            recs.append(rec), dys.append(c.dy.to(DEV)), dxs.append(torch.empty(B, C, N, device=DEV))
            meta.append((c, keep, p, y, rm, rv))
        outs = BNA.backward_from_records(recs, dys, dxs)
        assert len(outs) == len(shapes)
        for (c, keep, p, y, rm, rv), (dx, dg, db) in zip(meta, outs):
            ref, rests, groups, extra = _bn_reference(c, keep, p)
            got = {"y": y, "dx": dx, "d_gamma": dg, "d_beta": db, "running_mean": rm, "running_var": rv}
            NC.compare(got, ref, rests, BN_NAMES, groups, extra, label=label, ratios=RATIOS)


@pytest.mark.parametrize("B,C,N", [(4, 7, 256), (2, 6, 130)])
def test_bn_act_backward_sees_nothing_through_a_dropped_element(B, C, N):
    """forward and backward agree on the mask: an upstream gradient that is non-zero only where the forward dropped the
    element leaves dx, d_gamma and d_beta exactly 0"""
    from vdetr_amd.bn_act import bn_act
    p, salt = 0.3, 55
    keep = _bn_keep(B, C, N, p, salt)
    c = NC.bn_case(B, C, N)
    x = c.x.to(DEV).requires_grad_(True)
    w, b = c.gamma.to(DEV).requires_grad_(True), c.beta.to(DEV).requires_grad_(True)
    y = bn_act(x, w, b, None, None, True, NC.EPS, NC.MOMENTUM, relu=False, dropout_p=p, salt=salt)
    assert torch.equal((y != 0).cpu(), keep.bool())
    y.backward(gradient=(c.dy * (1 - keep).float()).to(DEV))
    assert float(x.grad.abs().max()) == 0 and float(w.grad.abs().max()) == 0 and float(b.grad.abs().max()) == 0


# ---- relu_dropout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("n", NC.RELU_DROPOUT_N)
def test_relu_dropout_matches_fp64(n, p):
    from vdetr_amd.bn_act import relu_dropout
    x, dy = NC.relu_dropout_case(n)
    drop = torch.nn.Dropout(p).train()
    keep = None
    if p > 0:
        keep = (relu_dropout(torch.ones(n, device=DEV), drop, salt=9) > 0).double().cpu()
        assert abs(float(keep.mean()) - NC.keep_prob(p)) <= 5 * NC.keep_sigma(p, n) or n < 100
    xd = x.to(DEV).requires_grad_(True)
    y = relu_dropout(xd, drop, salt=9)
    y.backward(gradient=dy.to(DEV))
    ref = NC.relu_dropout_ref(x, dy, keep, p)
    s32 = torch.tensor(NC.drop_scale(p), dtype=torch.float32)
    k32 = keep.float() if p > 0 else torch.ones(n)
    rest = {"y": x * (x > 0) * k32 * s32, "dx": dy * (x > 0) * k32 * s32}
    got = {"y": y.detach(), "dx": xd.grad}
    NC.compare(got, ref, [rest], ["y", "dx"], label="relu_dropout", ratios=RATIOS)
    dead = (x <= 0) | ((keep == 0) if p > 0 else torch.zeros(n, dtype=torch.bool))  # 0.0, -0.0, negatives, dropped: exactly 0
    assert bool((got["y"].cpu()[dead] == 0).all()) and bool((got["dx"].cpu()[dead] == 0).all())
    assert not torch.signbit(got["y"].cpu()[x == 0]).any()
    if p == 0:
        assert torch.equal(got["y"].cpu(), torch.relu(x)) and torch.equal(got["dx"].cpu(), dy * (x > 0))


# ---- the masks themselves ------------------------------------------------------------------------------------------------------------
def _mask_ln(p, salt):
    return _ln_keep(1024, 512, torch.nn.Dropout(p).train(), salt)[0]


def _mask_bn(p, salt):
    return _bn_keep(2, 256, 512, p, salt).permute(1, 0, 2).reshape(256, 1024)  # [channel, element of the channel]


def _mask_bn_sweep(p, salt):
    return _bn_keep(3, 256, 341, p, salt).permute(1, 0, 2).reshape(256, 1023)


def _mask_relu_dropout(p, salt):
    from vdetr_amd.bn_act import relu_dropout
    return (relu_dropout(torch.ones(1024, 256, device=DEV), torch.nn.Dropout(p).train(), salt=salt) > 0).double().cpu()


@pytest.mark.parametrize("p", [0.1, 0.3])
@pytest.mark.parametrize("draw", [_mask_ln, _mask_bn, _mask_bn_sweep, _mask_relu_dropout], ids=["add_ln", "bn_reg", "bn_sweep", "relu_dropout"])
def test_dropout_masks_are_bernoulli_in_every_direction(draw, p):
    """a mask that ignored the row, the channel or the salt would pass a mean test: keep fraction overall (5 sigma), of every
    row and every column (6 sigma; binomial with q = (65536 - t) / 65536), rows and salts independent, and reproducible"""
    from vdetr_amd import attention as A
    q = NC.keep_prob(p)
    m = draw(p, 11)
    rows, cols = m.shape
    assert set(m.unique().tolist()) == {0.0, 1.0}
    assert abs(float(m.mean()) - q) <= 5 * NC.keep_sigma(p, rows * cols)
    assert float((m.mean(1) - q).abs().max()) <= 6 * NC.keep_sigma(p, cols)
    assert float((m.mean(0) - q).abs().max()) <= 6 * NC.keep_sigma(p, rows)
    indep = q * q + (1 - q) * (1 - q)  # two independent masks agree with this probability
    sig = lambda n: 0.5 / np.sqrt(n)   # noqa: E731  (an upper bound of the agreement's sigma)
    assert not torch.equal(m[0], m[1]) and not torch.equal(m[:, 0], m[:, 1])
    assert abs(float((m[1:] == m[:-1]).double().mean()) - indep) <= 6 * sig((rows - 1) * cols)       # adjacent rows
    assert abs(float((m[:, 1:] == m[:, :-1]).double().mean()) - indep) <= 6 * sig(rows * (cols - 1))  # adjacent columns
    other = draw(p, 12)
    assert not torch.equal(m, other)
    assert abs(float((m == other).double().mean()) - indep) <= 6 * sig(rows * cols)
    assert torch.equal(draw(p, 11), m)  # the same step, the same salt
    A.reset_rng()
    A.begin_step(torch.device(DEV))
    assert torch.equal(draw(p, 11), m)  # a fresh generator at the same seed
    A.begin_step(torch.device(DEV))
    assert not torch.equal(draw(p, 11), m)  # the next step draws anew


def test_bn_masks_do_not_depend_on_the_arm():
    """the register arm and the sweep draw from the flat (b N + i) index of the channel: [2, C, 512] and [1, C, 1024] are the
    same elements; a misaligned x (sweep) gives the register arm's mask"""
    from vdetr_amd.bn_act import bn_act
    p, salt, C = 0.3, 31, 6
    a = _bn_keep(2, C, 512, p, salt).permute(1, 0, 2).reshape(C, 1024)
    b = _bn_keep(1, C, 1024, p, salt).reshape(C, 1024)
    assert torch.equal(a, b)
    x = _misaligned(torch.zeros(1, C, 1024))
    y = bn_act(x, torch.ones(C, device=DEV), torch.full((C,), 10.0, device=DEV), None, None, True, NC.EPS, NC.MOMENTUM, relu=True,
               dropout_p=p, salt=salt)
    assert torch.equal((y > 0).double().cpu().reshape(C, 1024), a)
    # ... and the first 1020 elements of a channel do not depend on the channel's length (sweep, N % 4 != 0)
    d = _bn_keep(1, C, 1021, p, salt).reshape(C, 1021)
    assert torch.equal(d[:, :1020], a[:, :1020])
