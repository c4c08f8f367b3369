"""The instrument of tests/test_gpu_norm_parity.py discriminates (CPU only): fp32 restatements with ONE defect each are rejected
by the same comparison that accepts the unmodified restatement; no GPU case has an ambiguous ReLU element; the GPU case lists
name every dispatch arm of add_ln.hip / bn_act.hip (the dispatch rules are restated here, not imported)."""
import collections

import pytest
import torch

import norm_cases as NC

ALL3 = ("d_y", "d_out", "d_out2")


def _keep(shape, p, seed=5):
    if p <= 0:
        return None
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) < NC.keep_prob(p)).to(torch.float64)


def _ln_names(dual, has_r):
    return (["y", "d_r"] if has_r else []) + ["out", "d_x", "d_gamma", "d_beta"] + (["out2", "d_gamma2", "d_beta2"] if dual else [])


HELD_OUT = (("tree", 64), "torch", 4)  # orders taken OUT of the yardstick and held against the rest of it like a kernel


def _others(got_kw):
    return tuple(o for o in NC.ORDERS if o != got_kw.get("order"))


def _ln_check(rows, C, dual, p, has_r, got_kw, subset=ALL3, factor=NC.FACTOR):
    c = NC.ln_case(rows, C)
    keep = _keep((rows, C), p)
    ref = NC.ln_eval(c, keep, p, subset, has_r=has_r, dual=dual)
    rests = NC.ln_restatements(c, keep, p, subset, has_r=has_r, dual=dual, orders=_others(got_kw))
    groups, extra = NC.ln_groups_and_extra(c, ref, subset, dual)
    got = NC.ln_eval(c, keep, p, subset, dtype=NC.F32, has_r=has_r, dual=dual, **got_kw)
    return NC.compare(got, ref, rests, _ln_names(dual, has_r), groups, extra, factor, label=f"ln{(rows, C, dual, p, has_r)}")


BN_NAMES = ["y", "dx", "d_gamma", "d_beta", "running_mean", "running_var"]


def _bn_check(B, C, N, p, got_kw, relu=True, affine_on=True, pre_bias=False, training=True, factor=NC.FACTOR):
    c = NC.bn_case(B, C, N, training, affine_on, pre_bias)
    keep = _keep((B, C, N), p)
    kw = dict(relu=relu, affine_on=affine_on, pre_bias=pre_bias, training=training)
    ref = NC.bn_eval(c, keep, p, training, **kw)
    rests = NC.bn_restatements(c, keep, p, training, orders=_others(got_kw), **kw)
    groups, extra = NC.bn_groups_and_extra(c, p, training, affine_on)
    got = NC.bn_eval(c, keep, p, training, dtype=NC.F32, **kw, **got_kw)
    return NC.compare(got, ref, rests, BN_NAMES if training else ["y"], groups, extra, factor, label=f"bn{(B, C, N, p)}")


def test_dropout_scale_is_the_unbiased_one_and_close_to_the_ideal():
    for p in (0.1, 0.2, 0.3, NC.composite_p(0.1, 0.2), 1e-6, 0.999999):
        t = NC.drop_threshold(p)
        assert 1 <= t <= 65535
        assert NC.drop_scale(p) * NC.keep_prob(p) == pytest.approx(1.0, abs=1e-15)
    for p in (0.1, 0.2, 0.3, NC.composite_p(0.1, 0.2)):
        assert abs(NC.drop_scale(p) * (1.0 - p) - 1.0) <= 2.0 ** -15, p
    assert NC.drop_threshold(0.0) == 0 and NC.drop_scale(0.0) == 1.0


@pytest.mark.parametrize("rows,C,dual,p,has_r", NC.LN_CASES)
def test_layer_norm_restatement_is_accepted(rows, C, dual, p, has_r):
    """an order of the restatement, taken out of the yardstick, passes against the remaining ones: the rule does not hang on
    one lucky rounding"""
    for order in HELD_OUT:
        _ln_check(rows, C, dual, p, has_r, dict(order=order))


@pytest.mark.parametrize("B,C,N", NC.BN_CASES)
def test_batch_norm_restatement_is_accepted(B, C, N):
    for p in NC.BN_P:
        for order in HELD_OUT:
            _bn_check(B, C, N, p, dict(order=order))


def test_batch_norm_variant_and_eval_restatements_are_accepted():
    for B, C, N, relu, p, affine_on, pre_bias in NC.BN_VARIANTS:
        _bn_check(B, C, N, p, {}, relu=relu, affine_on=affine_on, pre_bias=pre_bias)
    for B, C, N, relu, affine_on in NC.BN_EVAL:
        _bn_check(B, C, N, 0.0, {}, relu=relu, affine_on=affine_on, pre_bias=True, training=False)


# ---- the "wrong kernels": each must be rejected, at the rule's factor and at the largest factor the rule may ever take --------
@pytest.mark.parametrize("factor", [NC.FACTOR, 16])
@pytest.mark.parametrize("defect,rows,C,dual,p,has_r", [
    ("one_pass", 17, 512, True, 0.0, True),
    ("eps_outside", 16, 256, False, 0.0, False),
    ("drop_xhat_term", 9, 768, True, 0.1, True),
    ("dual_ignores_out2", 33, 1024, True, 0.1, True),
    ("dr_unscaled", 8, 256, True, 0.1, True),
])
def test_layer_norm_mutants_are_rejected(defect, rows, C, dual, p, has_r, factor):
    _ln_check(rows, C, dual, p, has_r, {}, factor=factor)  # the same case passes without the defect
    with pytest.raises(AssertionError, match="kernel - ref"):
        _ln_check(rows, C, dual, p, has_r, dict(defect=defect), factor=factor)


@pytest.mark.parametrize("factor", [NC.FACTOR, 16])
@pytest.mark.parametrize("defect,B,C,N,p,training", [
    ("one_pass", 4, 7, 256, 0.0, True),
    ("one_pass", 1, 4, 4352, 0.3, True),
    ("biased_running_var", 2, 5, 128, 0.0, True),
    ("biased_running_var", 1, 4, 4352, 0.0, True),
    ("eps_outside", 2, 9, 256, 0.3, True),
    ("drop_xhat_term", 4, 5, 512, 0.3, True),
    ("pre_bias_added", 2, 6, 130, 0.0, False),
])
def test_batch_norm_mutants_are_rejected(defect, B, C, N, p, training, factor):
    kw = dict(training=training, pre_bias=not training, factor=factor)
    _bn_check(B, C, N, p, {}, **kw)
    with pytest.raises(AssertionError, match="kernel - ref"):
        _bn_check(B, C, N, p, dict(defect=defect), **kw)


def test_one_pass_variance_is_rejected_by_the_large_mean_rows_alone():
    """the plain rows of the same tensor do not see a one-pass variance: the per-kind rule is what catches it"""
    c = NC.ln_case(33, 256)
    ref = NC.ln_eval(c, None, 0.0, has_r=False, dual=False)
    bad = NC.ln_eval(c, None, 0.0, dtype=NC.F32, has_r=False, dual=False, defect="one_pass")
    err = (bad["out"] - ref["out"]).abs().amax(1)
    kinds = c.kinds
    large = max(float(e) for e, k in zip(err, kinds) if k == "large")
    plain = max(float(e) for e, k in zip(err, kinds) if k == "plain")
    assert large > 100 * plain


# ---- ReLU margins ------------------------------------------------------------------------------------------------------------------
def test_no_gpu_case_has_an_ambiguous_relu_element():
    combos = {(B, C, N, True, True, False) for B, C, N in NC.BN_CASES + [NC.BN_CROSSED]}
    combos |= {(B, C, N, True, a, pb) for B, C, N, _, _, a, pb in NC.BN_VARIANTS}
    combos |= {(B, C, N, False, a, True) for B, C, N, _, a in NC.BN_EVAL}
    combos |= {(B, C, N, True, True, False) for lst in NC.BN_RECORDS for B, C, N in lst}
    for B, C, N, training, affine_on, pre_bias in sorted(combos):
        c = NC.bn_case(B, C, N, training, affine_on, pre_bias)
        assert c.ambiguous[(training, affine_on, pre_bias)] == 0, (B, C, N, training, affine_on, pre_bias)
        # ... and the guarantee is about the tensors handed to the kernel: recount on the stored x
        z, tol = NC._y_tolerance_per_channel(c, c.x, training=training, relu=False, affine_on=affine_on, pre_bias=pre_bias)
        assert int((z.abs().numpy() < tol).sum()) == 0


def test_nudging_leaves_the_channel_kinds_intact():
    c = NC.bn_case(4, 7, 256)
    x = c.x.double()
    mean, std = x.mean((0, 2)), x.std((0, 2))
    for k, m, s in zip(c.kinds, mean.tolist(), std.tolist()):
        if k == "plain":
            assert abs(m) < 0.2 and 0.8 < s < 1.2
        elif k == "large":
            assert abs(m) >= 45 and 0.8 < s < 3.5
        elif k == "tiny":
            assert abs(m) < 1e-4 and 0.5e-4 < s < 2e-4
        else:
            assert s == 0 and m == NC.CONST_VALUE


# ---- every dispatch arm is named by a case (the rules of vdetr_bn_act_fwd_f32 / vdetr_add_ln_*_f32, restated) ------------------------
def bn_arm(B, N, training=True, aligned=True):
    tot = B * N
    if tot == 1:
        return "n1"
    if not (N % 4 == 0 and tot % 256 == 0) or not aligned or not training:
        return "sweep_odd"
    if tot > 4096:
        return "sweep_big"
    return f"reg{tot // 256}" if tot // 256 in (1, 2, 4, 8, 16) else "sweep_hole"


def test_batch_norm_cases_name_every_arm():
    arms = collections.Counter(bn_arm(B, N) for B, _, N in NC.BN_CASES)
    for arm in ("reg1", "reg2", "reg4", "reg8", "reg16", "sweep_hole", "sweep_big", "sweep_odd", "n1"):
        assert arms[arm] >= 1, (arm, arms)
    assert arms["reg1"] >= 3 and arms["sweep_hole"] >= 2 and arms["sweep_odd"] >= 3
    # reg<1> with scene boundaries inside a wave's float4 walk (n4 < 64), and with idle waves in the last workgroup (C % 4)
    assert any(bn_arm(B, N) == "reg1" and B > 1 and N // 4 < 64 for B, _, N in NC.BN_CASES)
    assert any(bn_arm(B, N) == "reg1" and C % 4 for B, C, N in NC.BN_CASES)
    # every variant (no ReLU with dropout, no affine map, pre_bias) on a register arm and on a sweep arm
    by_variant = collections.defaultdict(set)
    for B, C, N, relu, p, affine_on, pre_bias in NC.BN_VARIANTS:
        by_variant[(relu, affine_on, pre_bias)].add(bn_arm(B, N)[:3])
    assert set(by_variant) == {(False, True, False), (True, False, False), (True, True, True)}
    assert all(v == {"reg", "swe"} for v in by_variant.values()), by_variant
    assert any(p > 0 for _, _, _, relu, p, _, _ in NC.BN_VARIANTS if not relu)
    assert bn_arm(NC.BN_CROSSED[0], NC.BN_CROSSED[2]) == "reg4" and bn_arm(NC.BN_CROSSED[0], NC.BN_CROSSED[2], aligned=False) == "sweep_odd"
    first, second = NC.BN_RECORDS
    assert len(first) > 12 and len({B * N for B, _, N in first}) == 1 and {C for _, C, _ in first} == {5, 64, 70}  # kBnBatch = 12
    assert bn_arm(first[0][0], first[0][2]) == "reg2" and all(N % 4 == 0 for _, _, N in first)
    assert len({B * N for B, _, N in second}) == 1 and second[0][0] * second[0][2] == 130
    assert any(not relu for _, _, _, relu, _ in NC.BN_EVAL) and any(not a for _, _, _, _, a in NC.BN_EVAL)


def test_layer_norm_cases_name_every_arm():
    pairs = {(rows, C) for rows, C, _, _, _ in NC.LN_CASES}
    for C in (256, 512, 768, 1024):  # add_ln_{fwd,bwd}_kernel<C / 256>
        for rows in (1, 8, 9, 16, 17, 33):  # 8 / 16 rows per workgroup forward / backward: full, one over, clamped rows
            assert (rows, C) in pairs
        assert any(c == C and dual and p > 0 for _, c, dual, p, _ in NC.LN_CASES)
        assert any(c == C and not has_r for _, c, _, _, has_r in NC.LN_CASES)
    # ln_param_reduce_body's second trip: more than 64 partial rows of 16 rows each
    big = [(rows, C, dual, p) for rows, C, dual, p, _ in NC.LN_CASES if -(-rows // 16) > 64]
    assert {(C, dual, p > 0) for _, C, dual, p in big} >= {(256, True, True), (1024, False, False)}
    # the batched reduction's second launch (kLnReduceBatch = 32), mixed widths, groups of >= 3 passes sharing a first norm
    assert len(NC.LN_DEFERRED) > 32 and {C for _, C, _, _, _ in NC.LN_DEFERRED} == {256, 512, 1024}
    shared = collections.Counter(first for _, _, _, first, _ in NC.LN_DEFERRED)
    assert min(shared.values()) >= 3 and any(dual for _, _, dual, _, _ in NC.LN_DEFERRED)
    assert len({C for _, C, _, first, _ in NC.LN_DEFERRED if first == NC.LN_DEFERRED[0][3]}) == 1  # one width per shared norm
    assert NC.LN_SUBSETS == (("d_y",), ("d_out",), ("d_out2",), ALL3)


def test_relu_dropout_cases_reach_the_second_grid_stride_trip():
    assert max(NC.RELU_DROPOUT_N) // 4 > 2048 * 256 and any(n // 4 % 256 for n in NC.RELU_DROPOUT_N) and min(NC.RELU_DROPOUT_N) == 4
    x, _ = NC.relu_dropout_case(1020)
    assert (x == 0).any() and torch.signbit(x[x == 0]).any() and (~torch.signbit(x[x == 0])).any() and (x > 0).any() and (x < 0).any()
