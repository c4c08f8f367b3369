"""The instrument of tests/test_gpu_rowblock_parity.py discriminates (CPU only): fp32 restatements of the row-block launches with
ONE defect each are rejected by the same comparison that accepts the unmodified restatement (its own order held out of the
yardstick); no GPU case has an ambiguous ReLU gate; the GPU arm lists name every arm."""
import functools

import pytest

import norm_cases as NC
import rowblock_cases as RC

NAMES = {"qkv": lambda kw: RC.qkv_names(kw.get("pos", True), True), "proj_q": lambda kw: RC.projq_names(kw.get("pos", True), kw.get("use", "yq"), True),
         "ffn": lambda kw: RC.ffn_names(kw.get("two", True)), "ffn0": lambda kw: RC.FFN0_NAMES}


@functools.lru_cache(maxsize=4)
def _evaluated(launch, shape, kw_items):
    """the float64 reference and one fp32 evaluation per entry of RC.EVALS, computed once per (launch, case, arm)"""
    c = RC.case(*shape)
    kw = dict(kw_items)
    return RC.reference(c, launch, **kw), {e: RC.restate(c, launch, e[0], e[1], **kw) for e in RC.EVALS}


def _check(launch, shape, kw, held=("mm", "torch"), defect=None, factor=NC.FACTOR):
    """the evaluation `held` (with `defect`) stands in for the kernel; the yardstick is every evaluation that shares neither its
    contraction order nor its LayerNorm order"""
    c = RC.case(*shape)
    ref, evs = _evaluated(launch, shape, tuple(sorted(kw.items())))
    rests = [r for (mm, o), r in evs.items() if mm != held[0] and o != held[1]]
    assert len(rests) >= 8
    got = evs[held] if defect is None else RC.restate(c, launch, held[0], held[1], defect, **kw)
    names = NAMES[launch](kw)
    extra = RC.ffn0_extra(c, ref, kw.get("p", RC.P)) if launch == "ffn0" else None
    return NC.compare(got, ref, rests, names, RC.groups_of(c, names), extra, factor, label=f"{launch}{shape}")


HELD_OUT = (RC.EVALS[0], RC.EVALS[2], RC.EVALS[7], RC.EVALS[8], RC.EVALS[10])   # mm / torch, 4 / 4, fma / 128, mfma / 256, 2 / tree 64


@pytest.mark.parametrize("shape", RC.SHAPES, ids=str)
@pytest.mark.parametrize("launch", ["qkv", "proj_q", "ffn", "ffn0"])
def test_restatement_is_accepted_with_its_own_order_held_out(launch, shape):
    for held in HELD_OUT:
        _check(launch, shape, {}, held)


def test_arm_variants_of_the_restatement_are_accepted():
    _check("qkv", (9, 2), dict(pos=False, alias=False))
    _check("qkv", (17, 1), dict(use="q"))
    _check("proj_q", (17, 1), dict(p=0.0))
    _check("proj_q", (11, 3), dict(pos=False))
    _check("proj_q", (8, 2), dict(use="y"))
    _check("ffn", (11, 3), dict(mode="p0", use="2"))
    _check("ffn", (17, 1), dict(two=False, use="z1"))
    _check("ffn0", (17, 1), dict(p=0.0))


# (launch, defect, the case that rejects it, the arm)
MUTANTS = [
    ("qkv", "v_from_x", (17, 1), {}),                     # v projected from t + pos
    ("qkv", "alias_in_dt", (16, 1), {}),                  # d_alias also added to d_t
    ("qkv", "qout_bmajor", (11, 3), {}),                  # batch-major mapping inverted: the outputs
    ("proj_q", "qout_bmajor", (9, 2), {}),
    ("proj_q", "da_bmajor", (8, 2), {}),                  # ... and d_a
    ("ffn", "da_bmajor", (11, 3), {}),
    ("proj_q", "tail_dup", (11, 3), {}),                  # the duplicated last row counted in d_gamma / d_beta of a tail block: 1 / 33
    ("ffn", "tail_dup", (17, 1), {}),
    ("ffn0", "tail_dup", (9, 2), {}),
    ("ffn", "ignore_o2", (17, 1), {}),                    # d_o2 ignored
    ("proj_q", "drop_xhat_term", (15, 1), {}),            # the x_hat mean(g x_hat) term dropped
    ("ffn0", "drop_xhat_term", (16, 1), {}),
    ("proj_q", "dproj_unscaled", (17, 1), {}),            # d_proj without the dropout scale
    ("ffn", "dproj_unscaled", (8, 2), {}),
    ("ffn", "p2_alone", (32, 1), {}),                     # p2 = dropout2.p alone although proj_drop.p > 0
    ("ffn", "act_nokeep", (9, 2), {}),                    # the activation gradient gated by the sign alone, not by the keep mask
    ("ffn0", "act_nokeep", (17, 1), {}),
    ("ffn0", "ffn0_res_x", (15, 1), {}),                  # ffn0's residual taken from x instead of LN(x)
    ("ffn0", "ffn0_no_res_grad", (11, 3), {}),            # ffn0's d t2 missing the residual share
]


@pytest.mark.parametrize("factor", [NC.FACTOR, 16])
@pytest.mark.parametrize("launch,defect,shape,kw", MUTANTS, ids=[f"{m[0]}-{m[1]}-{m[2][0]}x{m[2][1]}" for m in MUTANTS])
def test_mutants_are_rejected(launch, defect, shape, kw, factor):
    _check(launch, shape, kw, factor=factor)  # the same case passes without the defect
    with pytest.raises(AssertionError, match="kernel - ref"):
        _check(launch, shape, kw, defect=defect, factor=factor)


def test_the_mutant_list_covers_what_the_issue_names():
    assert {d for _, d, _, _ in MUTANTS} == {"v_from_x", "alias_in_dt", "qout_bmajor", "da_bmajor", "tail_dup", "ignore_o2", "drop_xhat_term",
                                              "dproj_unscaled", "p2_alone", "act_nokeep", "ffn0_res_x", "ffn0_no_res_grad"}
    for launch, defect, shape, _ in MUTANTS:
        if defect in ("qout_bmajor", "da_bmajor"):
            assert shape[1] > 1
        if defect == "tail_dup":
            assert (shape[0] * shape[1]) % 16


def test_no_gpu_case_has_an_ambiguous_relu_gate():
    used = {a[0] for arms in (RC.QKV_ARMS, RC.PROJQ_ARMS, RC.FFN_ARMS, RC.FFN0_ARMS) for a in arms}
    assert used == set(RC.SHAPES)
    for shape in RC.SHAPES:
        c = RC.case(*shape)
        assert c.ambiguous == {"ffn": 0, "ffn0": 0}, (shape, c.ambiguous)
        # ... and the guarantee is about the b1 handed to the kernel: recount on the stored parameters
        for launch, _, configs in RC._GATES:
            assert int(RC._ambiguous(c, launch, configs)[0].sum()) == 0


def test_cases_cover_the_workgroup_geometry():
    arms = [RC.arm_of(s) for s in RC.SHAPES]
    assert [a["blocks"] for a in arms] == [1, 1, 1, 2, 2, 1, 2, 3] and [s[0] * s[1] for s in RC.SHAPES] == [1, 15, 16, 17, 32, 16, 18, 33]
    assert any(a["tail"] == 0 and a["blocks"] == 1 for a in arms) and any(a["tail"] == 0 and a["blocks"] == 2 for a in arms)
    assert any(a["tail"] == 1 and a["blocks"] == 1 for a in arms) and any(a["tail"] == 15 for a in arms)     # a lone row; one short of full
    assert any(a["tail"] == 1 and a["blocks"] == 2 and a["scenes"] == 1 for a in arms)                          # one row into the next block
    assert {g for a in arms for g in a["dead_groups"]} == {0, 1, 2, 3}                                          # a tail inside every row group
    assert {a["scenes"] for a in arms if a["tail"]} >= {1, 2, 3}                                                # rb_bmajor with a tail
    kinds = {k for s in RC.SHAPES for k in RC.case(*s).kinds}
    assert kinds == set(NC.KINDS)


def test_arm_lists_name_every_arm():
    S = set(RC.SHAPES)
    q = RC.QKV_ARMS
    assert {a[0] for a in q if a[1:] == (True, True, True, "qkv")} == S
    assert any(not a[1] for a in q) and any(a[1] and not a[2] for a in q)              # without pos; pos not requiring grad
    assert any(a[1] and a[2] and not a[3] for a in q) and any(a[3] for a in q)         # d_alias absent / present
    assert {len(a[4]) for a in q} == {1, 2, 3}                                         # two, one and none of dq / dk / dv unused
    assert {a[0][1] for a in q} == {1, 2, 3}
    assert all(a[2] or not a[3] for a in q)                                            # (a non-differentiable alias cannot carry a gradient)
    p = RC.PROJQ_ARMS
    assert {a[0] for a in p if a[1:] == (RC.P, True, "yq", True)} == S
    assert {a[1] for a in p} == {0.0, RC.P} and {a[2] for a in p} == {True, False} and {a[3] for a in p} == {"y", "q", "yq"}
    assert any(not a[4] for a in p) and any(a[0][1] > 1 and not a[4] for a in p)
    f = RC.FFN_ARMS
    assert {a[0] for a in f if a[1:] == ("drop", True, "z12")} == S
    assert {a[1] for a in f} == {"drop", "p0", "eval"} and {a[2] for a in f} == {True, False}
    assert {a[3] for a in f if a[2]} >= {"z", "1", "2", "z12"}
    assert RC.FFN_MODES["drop"][0] == NC.composite_p(RC.P, RC.P) > RC.P and RC.FFN_MODES["eval"] == (0.0, 0.0, 0.0)
    f0 = RC.FFN0_ARMS
    assert {a[0] for a in f0 if a[1:] == (RC.P, "z1")} == S
    assert {a[1] for a in f0} == {0.0, RC.P} and {a[2] for a in f0} == {"z", "1", "z1"}
