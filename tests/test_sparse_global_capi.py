"""The C ABI of csrc/sparse_global.hip (global pooling, broadcast, the squeeze-excite gate): exported and bound, every descriptor
check an error code whose message names the field, before anything is launched; empty tables are no-ops; the workspace functions
grow with N and cover ceil(N / rows) + nseg chunks.  No GPU needed."""
import ctypes

import numpy as np
import pytest

NEW = ("vdetr_sp_global_chunk_rows", "vdetr_sp_global_pool_workspace_bytes", "vdetr_sp_global_pool_fwd_f32",
       "vdetr_sp_global_pool_bwd_f32", "vdetr_sp_broadcast_workspace_bytes", "vdetr_sp_broadcast_fwd_f32",
       "vdetr_sp_broadcast_bwd_f32", "vdetr_sp_se_gate_f32")


@pytest.fixture(scope="module")
def env():
    from vdetr_amd import _lib
    spare = np.zeros(64, np.uint8)  # an address for the pointer checks; a failed check launches nothing, so nothing follows it
    return _lib, _lib.lib(), spare


def _filled(d, spare, **fields):
    for name, kind in d._fields_:
        if kind is ctypes.c_void_p:
            setattr(d, name, spare.ctypes.data)
    for name, value in fields.items():
        setattr(d, name, value)
    return d


def test_entry_points_are_exported_and_bound(env):
    _lib, lib, _ = env
    for sym in NEW:
        assert sym in _lib.exported_symbols() and hasattr(lib, sym), sym
    assert lib.vdetr_abi_version() == 3  # additive
    assert (_lib.VDETR_BCAST_ADD, _lib.VDETR_BCAST_MUL, _lib.VDETR_BCAST_CAT) == (0, 1, 2)


def _refused(lib, status, *words):
    msg = lib.vdetr_last_error()
    assert status == 1 and all(w in msg for w in words), (status, msg, words)


def test_pooling_descriptor_checks(env):
    _lib, lib, spare = env
    good = dict(N=100, C=8, nseg=2, mode=_lib.VDETR_POOL_MAX)
    calls = {b"sp_global_pool_fwd": lambda d: lib.vdetr_sp_global_pool_fwd_f32(ctypes.byref(d), None),
             b"sp_global_pool_bwd": lambda d: lib.vdetr_sp_global_pool_bwd_f32(ctypes.byref(d), spare.ctypes.data, spare.ctypes.data, None)}
    for op, call in calls.items():
        for bad, word in ((dict(C=6), b"C=6"), (dict(C=0), b"C=0"), (dict(C=1028), b"C=1028"), (dict(N=-1), b"N=-1"),
                          (dict(nseg=-2), b"nseg=-2"), (dict(mode=3), b"mode=3"), (dict(seg=None), b"seg is NULL"),
                          (dict(arg=None), b"arg is NULL")):
            _refused(lib, call(_filled(_lib.SpGlobalPoolDesc(), spare, **dict(good, **bad))), op, word)
        assert call(_filled(_lib.SpGlobalPoolDesc(), spare, **dict(good, N=0))) == 0
        assert call(_filled(_lib.SpGlobalPoolDesc(), spare, **dict(good, nseg=0))) == 0
    fwd = calls[b"sp_global_pool_fwd"]
    for bad, word in ((dict(x=None), b"x is NULL"), (dict(y=None), b"y is NULL"), (dict(workspace=None), b"workspace is NULL")):
        _refused(lib, fwd(_filled(_lib.SpGlobalPoolDesc(), spare, **dict(good, **bad))), b"sp_global_pool_fwd", word)
    d = _filled(_lib.SpGlobalPoolDesc(), spare, **good)
    _refused(lib, lib.vdetr_sp_global_pool_bwd_f32(ctypes.byref(d), None, spare.ctypes.data, None), b"dy is NULL")
    _refused(lib, lib.vdetr_sp_global_pool_bwd_f32(ctypes.byref(d), spare.ctypes.data, None, None), b"dx is NULL")
    _refused(lib, lib.vdetr_sp_global_pool_fwd_f32(None, None), b"null descriptor")


def test_broadcast_descriptor_checks(env):
    _lib, lib, spare = env
    p = spare.ctypes.data
    good = dict(N=100, Cx=8, Cg=8, nseg=2, mode=_lib.VDETR_BCAST_MUL, relu=0, residual=None)
    fwd = lambda d: lib.vdetr_sp_broadcast_fwd_f32(ctypes.byref(d), None)  # noqa: E731
    bwd = lambda d: lib.vdetr_sp_broadcast_bwd_f32(ctypes.byref(d), p, p, p, None)  # noqa: E731
    for op, call in ((b"sp_broadcast_fwd", fwd), (b"sp_broadcast_bwd", bwd)):
        for bad, word in ((dict(Cx=6, Cg=6), b"Cx=6"), (dict(Cg=1028, mode=_lib.VDETR_BCAST_CAT), b"Cg=1028"), (dict(Cg=0), b"Cg=0"),
                          (dict(N=-3), b"N=-3"), (dict(nseg=-1), b"nseg=-1"), (dict(mode=7), b"mode=7"), (dict(mode=-1), b"mode=-1"),
                          (dict(Cg=12), b"Cg=12"), (dict(Cg=12, mode=_lib.VDETR_BCAST_ADD), b"Cx=8"), (dict(seg=None), b"seg is NULL"),
                          (dict(mode=_lib.VDETR_BCAST_CAT, residual=p), b"residual")):
            _refused(lib, call(_filled(_lib.SpBroadcastDesc(), spare, **dict(good, **bad))), op, word)
        assert call(_filled(_lib.SpBroadcastDesc(), spare, **dict(good, N=0))) == 0
        assert call(_filled(_lib.SpBroadcastDesc(), spare, **dict(good, nseg=0))) == 0
    for bad, word in ((dict(x=None), b"x is NULL"), (dict(g=None), b"g is NULL"), (dict(y=None), b"y is NULL")):
        _refused(lib, fwd(_filled(_lib.SpBroadcastDesc(), spare, **dict(good, **bad))), b"sp_broadcast_fwd", word)
    for bad, word in ((dict(x=None), b"x is NULL"), (dict(g=None), b"g is NULL"), (dict(workspace=None), b"workspace is NULL")):
        _refused(lib, bwd(_filled(_lib.SpBroadcastDesc(), spare, **dict(good, **bad))), b"sp_broadcast_bwd", word)
    d = _filled(_lib.SpBroadcastDesc(), spare, **good)
    _refused(lib, lib.vdetr_sp_broadcast_bwd_f32(ctypes.byref(d), None, p, p, None), b"dy is NULL")
    assert lib.vdetr_sp_broadcast_bwd_f32(ctypes.byref(d), p, None, None, None) == 0  # neither half wanted: nothing to do
    _refused(lib, lib.vdetr_sp_broadcast_fwd_f32(None, None), b"null descriptor")


def test_gate_descriptor_checks(env):
    _lib, lib, spare = env
    good = dict(N=100, C=16, H=4, nseg=2)
    call = lambda d: lib.vdetr_sp_se_gate_f32(ctypes.byref(d), None)  # noqa: E731
    for bad, word in ((dict(C=18), b"C=18"), (dict(C=2048), b"C=2048"), (dict(H=0), b"H=0"), (dict(H=257), b"H=257"),
                      (dict(N=-1), b"N=-1"), (dict(nseg=-1), b"nseg=-1"), (dict(x=None), b"x is NULL"), (dict(seg=None), b"seg is NULL"),
                      (dict(w1=None), b"w1 is NULL"), (dict(w2=None), b"w2 is NULL"), (dict(gate=None), b"gate is NULL"),
                      (dict(workspace=None), b"workspace is NULL")):
        _refused(lib, call(_filled(_lib.SpSeGateDesc(), spare, **dict(good, **bad))), b"sp_se_gate", word)
    assert call(_filled(_lib.SpSeGateDesc(), spare, **dict(good, N=0))) == 0
    assert call(_filled(_lib.SpSeGateDesc(), spare, **dict(good, nseg=0))) == 0
    _refused(lib, lib.vdetr_sp_se_gate_f32(None, None), b"null descriptor")


def test_workspace_functions_grow_with_n_and_cover_the_chunks(env):
    _, lib, _ = env
    assert lib.vdetr_sp_global_chunk_rows(0) == lib.vdetr_sp_global_chunk_rows(1024) == 16
    assert lib.vdetr_sp_global_chunk_rows(1025) == 32 and lib.vdetr_sp_global_chunk_rows(36000) == 576
    for C, nseg in ((4, 1), (64, 4), (1024, 16)):
        prev_pool = prev_bc = 0
        for N in list(range(0, 2100)) + [4095, 4096, 4097, 36000, 36001, 100000, 2 ** 24, 2 ** 31 - 1]:
            rows = lib.vdetr_sp_global_chunk_rows(N)
            assert rows >= 16 and rows % 16 == 0
            chunks = -(-N // rows) + nseg
            pool, bc = lib.vdetr_sp_global_pool_workspace_bytes(N, C, nseg), lib.vdetr_sp_broadcast_workspace_bytes(N, C, nseg)
            assert pool >= chunks * C * 8 and bc >= chunks * C * 4, (N, C, nseg)  # values and rows / sums
            assert pool >= prev_pool and bc >= prev_bc, (N, C, nseg)
            assert pool <= (64 + nseg) * C * 8  # about 64 partial chunks per table, however large
            prev_pool, prev_bc = pool, bc
    assert lib.vdetr_sp_global_pool_workspace_bytes(-5, 8, -1) == 0 and lib.vdetr_sp_broadcast_workspace_bytes(10, -8, 1) == 0
