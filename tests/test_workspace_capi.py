"""The launches whose descriptor carries a bare workspace pointer (no byte count), from the host side.  No GPU needed.

Size functions.  `vdetr_sp_bn_workspace_bytes`, `vdetr_sp_inorm_workspace_bytes`, `vdetr_heads_workspace_bytes`,
`vdetr_add_ln_bwd_workspace_bytes`, `vdetr_colsum_workspace_bytes` and `vdetr_sp_pair_plan_workspace_ints` against
tests/workspace_restatement.py (the grid of the launch that writes times a workgroup's footprint, plus the sums behind the
partials): at least the restated need, non-decreasing in N, zero or sane for negative arguments as include/vdetr_hip.h says.  N
runs over 0 .. 70,000 through every value at which a rows-per-workgroup rule steps and one either side of it.

Alignment.  A non-NULL workspace that is not 16-B aligned (the pair plan: 4 B) is an argument error whose message names the
field, before anything is launched: the pointers here are host addresses, nothing could be launched on them."""
import ctypes
import itertools

import numpy as np
import pytest

import workspace_restatement as WR

WIDTHS = (4, 8, 256, 1024)
SCENES = (0, 1, 3, 16)
HI = 70000


@pytest.fixture(scope="module")
def env():
    from vdetr_amd import _lib
    buf = np.zeros(96, np.uint8)  # an address for the pointer checks; a failed check launches nothing, so nothing follows it
    spare = buf.ctypes.data + (-buf.ctypes.data) % 16
    return _lib, _lib.lib(), spare, buf


def _filled(d, spare, **fields):
    for name, kind in d._fields_:
        if kind is ctypes.c_void_p:
            setattr(d, name, spare)
    for name, value in fields.items():
        setattr(d, name, value)
    return d


def _refused(lib, status, *words):
    msg = lib.vdetr_last_error()
    assert status == 1 and all(w in msg for w in words), (status, msg, words)


# ---- the size functions -------------------------------------------------------------------------------------------------------------
def _swept(size, need, ns, what):
    """size(N) >= need(N) at every N of the sweep, and size never drops as N grows"""
    prev = 0
    for N in ns:
        got, want = size(N), need(N)
        assert got >= want, (what, N, got, want)
        assert got >= prev, (what, N, got, prev)
        prev = got


def test_the_sweep_hits_every_step_of_the_rules():
    assert WR.steps(WR.bn_rows, 0, HI) == [17 * 1024, 33 * 1024, 49 * 1024, 65 * 1024]
    assert [WR.bn_rows(n) for n in (0, 17407, 17408, 33792, 50176, 66560, HI)] == [16, 16, 32, 48, 64, 80, 80]
    assert WR.steps(WR.inorm_stat_rows, 0, HI)[:3] == [1025, 2049, 3073] and WR.inorm_stat_rows(1024) == 16 and WR.inorm_stat_rows(HI) == 1104
    ns = WR.sweep([WR.bn_rows, WR.inorm_stat_rows])
    for s in WR.steps(WR.bn_rows, 0, HI) + WR.steps(WR.inorm_stat_rows, 0, HI):
        assert {s - 1, s, s + 1} <= set(ns), s
    assert ns[0] == 0 and ns[-1] == HI and set(range(2101)) <= set(ns)
    assert WR.steps(lambda r: WR.colsum_splits(2, r, 8), 0, HI) == [64 << k for k in range(8)]  # S = 2 .. 256


def test_sp_bn_workspace_covers_the_partials_and_the_sums(env):
    _, lib, _, _ = env
    ns = WR.sweep([WR.bn_rows])
    for C in WIDTHS:
        _swept(lambda N: lib.vdetr_sp_bn_workspace_bytes(N, C), lambda N: WR.sp_bn_need(N, C), ns, ("sp_bn", C))
    assert lib.vdetr_sp_bn_workspace_bytes(1, 8) == WR.sp_bn_need(1, 8) == 5 * 8 * 4  # one workgroup: [3][C] and the sums
    assert lib.vdetr_sp_bn_workspace_bytes(70, 8) == WR.sp_bn_need(70, 8) == (5 * 3 + 2) * 8 * 4
    assert lib.vdetr_sp_bn_workspace_bytes(-5, 8) == lib.vdetr_sp_bn_workspace_bytes(0, 8) == lib.vdetr_sp_bn_workspace_bytes(1, 8)
    assert lib.vdetr_sp_bn_workspace_bytes(10, -8) == 0 and lib.vdetr_sp_bn_workspace_bytes(10, 0) == 0


def test_sp_inorm_workspace_covers_the_chunks_of_every_split(env):
    _, lib, _, _ = env
    ns = WR.sweep([WR.inorm_stat_rows])
    for C, nseg in itertools.product(WIDTHS, SCENES):
        _swept(lambda N: lib.vdetr_sp_inorm_workspace_bytes(N, C, nseg), lambda N: WR.sp_inorm_need(N, C, nseg), ns, ("sp_inorm", C, nseg))
    # the chunks that scenes cut on their own really have stay inside the grid the need is restated from
    for sizes in ((33, 0, 37), (1,) * 16, (17, 17, 17), (1024, 1), (1, 1040, 1), (15, 16, 17, 0, 1)):
        N, rows = sum(sizes), WR.inorm_stat_rows(sum(sizes))
        chunks = WR.inorm_chunks(sizes, rows)
        assert chunks <= WR.ceil_div(N, rows) + len(sizes)
        assert lib.vdetr_sp_inorm_workspace_bytes(N, 8, len(sizes)) >= chunks * 3 * 8 * 4
    assert lib.vdetr_sp_inorm_workspace_bytes(-5, 8, -1) == lib.vdetr_sp_inorm_workspace_bytes(0, 8, 0) <= 3 * 8 * 4
    assert lib.vdetr_sp_inorm_workspace_bytes(10, -8, 1) == 0
    for nseg in SCENES[:-1]:  # ... and it grows with the scenes
        assert lib.vdetr_sp_inorm_workspace_bytes(70, 8, nseg) < lib.vdetr_sp_inorm_workspace_bytes(70, 8, nseg + 1)


def test_heads_workspace_covers_both_partial_tables(env):
    _, lib, _, _ = env
    ns = sorted(set(range(0, 2101)) | {n + d for n in range(0, HI + 1, 32) for d in (-1, 0, 1) if 0 <= n + d <= HI} | {HI})
    for B, G in itertools.product((1, 2, 4), (1, 5, 8)):
        _swept(lambda N: lib.vdetr_heads_workspace_bytes(B, N, G), lambda N: WR.heads_need(B, N, G), ns, ("heads", B, G))
    assert lib.vdetr_heads_workspace_bytes(1, 64, 5) == WR.heads_need(1, 64, 5) == 2 * 2 * 5 * 256 * 2 * 4
    for bad in ((-1, 64, 5), (1, -64, 5), (1, 64, -5), (0, 64, 5), (1, 0, 5), (1, 64, 0)):
        assert lib.vdetr_heads_workspace_bytes(*bad) == 0, bad


def test_add_ln_bwd_workspace_covers_a_row_of_partials_per_workgroup(env):
    _lib, lib, _, _ = env
    d = _lib.AddLnDesc()

    def size(rows, C):
        d.rows, d.C = rows, C
        return lib.vdetr_add_ln_bwd_workspace_bytes(ctypes.byref(d))

    ns = sorted(set(range(0, 2101)) | {n + k for n in range(0, HI + 1, 16) for k in (-1, 0, 1) if 0 <= n + k <= HI} | {HI})
    for C in WIDTHS:
        _swept(lambda N: size(N, C), lambda N: WR.add_ln_bwd_need(N, C), ns, ("add_ln_bwd", C))
    assert size(77, 256) == WR.add_ln_bwd_need(77, 256) == 5 * 4 * 256 * 4
    assert size(-1, 256) == 0 and size(0, 256) == 0 and size(16, -256) == 0 and size(16, 0) == 0
    assert lib.vdetr_add_ln_bwd_workspace_bytes(None) == 0


def test_colsum_workspace_covers_the_split_partials(env):
    _, lib, _, _ = env
    for n, cols in itertools.product((1, 2, 3, 16), WIDTHS):
        ns = WR.sweep([lambda r: WR.colsum_splits(n, r, cols)])
        _swept(lambda r: lib.vdetr_colsum_workspace_bytes(n, r, cols), lambda r: WR.colsum_need(n, r, cols), ns, ("colsum", n, cols))
    assert lib.vdetr_colsum_workspace_bytes(2, 128, 8) == WR.colsum_need(2, 128, 8) == 2 * 4 * 8 * 4 == 256  # S = 4
    assert lib.vdetr_colsum_workspace_bytes(2, 63, 8) == 0 and lib.vdetr_colsum_workspace_bytes(2, 64, 8) == 2 * 2 * 8 * 4
    assert lib.vdetr_colsum_workspace_bytes(2, 4096, 6) == 0  # columns that are no multiple of four are never split
    for bad in ((-2, 128, 8), (2, -128, 8), (2, 128, -8), (0, 128, 8), (2, 0, 8), (2, 128, 0)):
        assert lib.vdetr_colsum_workspace_bytes(*bad) == 0, bad


def test_pair_plan_workspace_covers_a_count_per_offset_and_block(env):
    _, lib, _, _ = env
    ns = sorted(set(range(0, 2101)) | {n + k for n in range(0, HI + 1, 256) for k in (-1, 0, 1) if 0 <= n + k <= HI} | {HI})
    for K in (1, 27, 125, 1024):
        _swept(lambda N: lib.vdetr_sp_pair_plan_workspace_ints(K, N), lambda N: WR.pair_plan_need_ints(K, N), ns, ("pair_plan", K))
    assert lib.vdetr_sp_pair_plan_workspace_ints(27, 300) == WR.pair_plan_need_ints(27, 300) == 54
    assert lib.vdetr_sp_pair_plan_workspace_ints(27, -5) == lib.vdetr_sp_pair_plan_workspace_ints(27, 0) == 27
    assert lib.vdetr_sp_pair_plan_workspace_ints(-3, 300) == 0 and lib.vdetr_sp_pair_plan_workspace_ints(0, 300) == 0


# ---- the alignment of a bare workspace pointer -----------------------------------------------------------------------------------------
def test_a_misaligned_workspace_is_an_argument_error_that_names_the_field(env):
    _lib, lib, p, _ = env
    odd = p + 8  # a host address that ends in ...8: 8-B aligned and no more
    assert p % 16 == 0 and odd % 16 == 8
    word = b"workspace must be 16-B aligned"

    bn = lambda **kw: _filled(_lib.SpBnDesc(), p, **dict(dict(N=70, C=8, act=1, training=1, eps=1e-5, momentum=0.1), **kw))  # noqa: E731
    _refused(lib, lib.vdetr_sp_bn_act_fwd_f32(ctypes.byref(bn(workspace=odd)), None), b"sp_bn_act_fwd", word)
    _refused(lib, lib.vdetr_sp_bn_act_bwd_f32(ctypes.byref(bn(workspace=odd)), p, p, p, p, p, None), b"sp_bn_act_bwd", word)
    _refused(lib, lib.vdetr_sp_bn_act_bwd_f32(ctypes.byref(bn(workspace=None)), p, p, p, p, p, None), b"sp_bn_act_bwd", b"null pointer")

    inorm = lambda **kw: _filled(_lib.SpInormDesc(), p, **dict(dict(N=70, C=8, nseg=3, eps=1e-6), **kw))  # noqa: E731
    _refused(lib, lib.vdetr_sp_inorm_fwd_f32(ctypes.byref(inorm(workspace=odd)), None), b"sp_inorm_fwd", word)
    _refused(lib, lib.vdetr_sp_inorm_bwd_f32(ctypes.byref(inorm(workspace=odd)), p, p, p, p, None), b"sp_inorm_bwd", word)
    _refused(lib, lib.vdetr_sp_inorm_fwd_f32(ctypes.byref(inorm(workspace=None)), None), b"sp_inorm_fwd", b"workspace is NULL")

    for mode in (_lib.VDETR_POOL_SUM, _lib.VDETR_POOL_AVG, _lib.VDETR_POOL_MAX):
        d = _filled(_lib.SpGlobalPoolDesc(), p, N=70, C=8, nseg=3, mode=mode, workspace=odd)
        _refused(lib, lib.vdetr_sp_global_pool_fwd_f32(ctypes.byref(d), None), b"sp_global_pool_fwd", word)
    for mode in (_lib.VDETR_BCAST_ADD, _lib.VDETR_BCAST_MUL, _lib.VDETR_BCAST_CAT):
        d = _filled(_lib.SpBroadcastDesc(), p, N=70, Cx=8, Cg=8, nseg=3, mode=mode, relu=0, residual=None, workspace=odd)
        _refused(lib, lib.vdetr_sp_broadcast_bwd_f32(ctypes.byref(d), p, p, p, None), b"sp_broadcast_bwd", word)
    d = _filled(_lib.SpSeGateDesc(), p, N=70, C=8, H=4, nseg=3, workspace=odd)
    _refused(lib, lib.vdetr_sp_se_gate_f32(ctypes.byref(d), None), b"sp_se_gate", word)

    cw = lambda **kw: _filled(_lib.SpCwConvDesc(), p, **dict(dict(K=27, nout=133, nin=133, C=8), **kw))  # noqa: E731
    _refused(lib, lib.vdetr_sp_cwconv_wgrad_f32(ctypes.byref(cw(workspace=odd)), p, p, p, None), b"sp_cwconv_wgrad", word)
    _refused(lib, lib.vdetr_sp_cwconv_wgrad_f32(ctypes.byref(cw(workspace=odd)), p, None, p, None), b"sp_cwconv_wgrad", word)  # db alone
    _refused(lib, lib.vdetr_sp_cwconv_wgrad_f32(ctypes.byref(cw(workspace=None)), p, p, p, None), b"sp_cwconv_wgrad", b"workspace is NULL")

    ln = _filled(_lib.AddLnDesc(), p, rows=77, C=256, eps=1e-5, dropout_p=0.0, rng_state=None, r=None, y=None, gamma2=None, beta2=None,
                 out2=None)
    grads = _filled(_lib.AddLnGrads(), p, d_out2=None, d_r=None, d_gamma2=None, d_beta2=None, partials=odd)
    _refused(lib, lib.vdetr_add_ln_bwd_f32(ctypes.byref(ln), ctypes.byref(grads), None), b"add_ln_bwd", b"partials must be 16-B aligned")
    grads.partials = None
    _refused(lib, lib.vdetr_add_ln_bwd_f32(ctypes.byref(ln), ctypes.byref(grads), None), b"add_ln_bwd", b"null pointer")

    for off in (1, 2, 3):  # the pair plan's counts are ints: 4 B
        _refused(lib, lib.vdetr_sp_pair_plan_i32(p, 27, 300, 300, p, p, p, p, p, p + off, None), b"sp_pair_plan",
                 b"workspace must be 4-B aligned")
    _refused(lib, lib.vdetr_sp_pair_plan_i32(p, 27, 300, 300, p, p, p, p, p, None, None), b"sp_pair_plan", b"null pointer")

    heads = _filled(_lib.HeadsDesc(), p, B=1, N=64, G=1, rows=18, p1=0.0, p2=0.0, workspace=odd)  # (the check these follow)
    _refused(lib, lib.vdetr_heads_fwd_f32(ctypes.byref(heads), None), b"heads_fwd", b"16-B aligned")


def test_a_workspace_nobody_reads_is_not_checked(env):
    """launches that do not touch the workspace take any pointer: the checks sit with the launches that carve it.  (All of these
    stop at a later argument check or at an empty table: nothing is launched.)"""
    _lib, lib, p, _ = env
    odd = p + 8
    d = _filled(_lib.SpGlobalPoolDesc(), p, N=0, C=8, nseg=3, mode=_lib.VDETR_POOL_SUM, workspace=odd)
    assert lib.vdetr_sp_global_pool_fwd_f32(ctypes.byref(d), None) == 0  # an empty table is a no-op
    d = _filled(_lib.SpBroadcastDesc(), p, N=70, Cx=8, Cg=8, nseg=3, mode=_lib.VDETR_BCAST_MUL, relu=0, residual=None, workspace=odd)
    assert lib.vdetr_sp_broadcast_bwd_f32(ctypes.byref(d), p, None, None, None) == 0  # neither half wanted: nothing to do
    cw = _filled(_lib.SpCwConvDesc(), p, K=27, nout=0, nin=0, C=8, workspace=odd)
    assert lib.vdetr_sp_cwconv_fwd_f32(ctypes.byref(cw), None) == 0
