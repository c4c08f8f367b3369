"""The C ABI of csrc/sparse_cwconv.hip (the channelwise convolution): exported and bound, every descriptor check an error code
whose message names the field, before anything is launched; empty tables are no-ops; the workspace function grows with nout and
covers ceil(nout / rows) chunks of [K + 1, C].  No GPU needed.  (A weight gradient over nout == 0 still launches its fold, which
writes the zeros: tests/test_gpu_channelwise.py covers it.)"""
import ctypes

import numpy as np
import pytest

NEW = ("vdetr_sp_cwconv_chunk_rows", "vdetr_sp_cwconv_workspace_bytes", "vdetr_sp_cwconv_fwd_f32", "vdetr_sp_cwconv_dgrad_f32",
       "vdetr_sp_cwconv_wgrad_f32")


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


def _refused(lib, status, *words):
    msg = lib.vdetr_last_error()
    assert status == 1 and all(w in msg for w in words), (status, msg, words)


def test_entry_points_are_exported_and_bound(env):
    _lib, lib, _ = env
    for sym in NEW:
        assert sym in _lib.exported_symbols() and hasattr(lib, sym), sym
    assert lib.vdetr_abi_version() == 3  # additive
    assert [n for n, _ in _lib.SpCwConvDesc._fields_] == ["K", "nout", "nin", "C", "x", "nbr", "w", "bias", "y", "workspace"]


def test_descriptor_checks(env):
    _lib, lib, spare = env
    p = spare.ctypes.data
    good = dict(K=27, nout=100, nin=90, C=8)
    calls = {b"sp_cwconv_fwd": lambda d: lib.vdetr_sp_cwconv_fwd_f32(ctypes.byref(d), None),
             b"sp_cwconv_dgrad": lambda d: lib.vdetr_sp_cwconv_dgrad_f32(ctypes.byref(d), p, p, p, None),
             b"sp_cwconv_wgrad": lambda d: lib.vdetr_sp_cwconv_wgrad_f32(ctypes.byref(d), p, p, p, None)}
    for op, call in calls.items():
        for bad, word in ((dict(C=0), b"C=0"), (dict(C=6), b"C=6"), (dict(C=1028), b"C=1028"), (dict(K=0), b"K=0"),
                          (dict(K=128), b"K=128"), (dict(nout=-1), b"nout=-1"), (dict(nin=-4), b"nin=-4")):
            _refused(lib, call(_filled(_lib.SpCwConvDesc(), spare, **dict(good, **bad))), op, word)
    new = lambda **bad: _filled(_lib.SpCwConvDesc(), spare, **dict(good, **bad))  # noqa: E731
    fwd, dgrad, wgrad = calls[b"sp_cwconv_fwd"], calls[b"sp_cwconv_dgrad"], calls[b"sp_cwconv_wgrad"]
    for bad, word in ((dict(x=None), b"x is NULL"), (dict(nbr=None), b"nbr is NULL"), (dict(w=None), b"w is NULL"),
                      (dict(y=None), b"y is NULL")):
        _refused(lib, fwd(new(**bad)), b"sp_cwconv_fwd", word)
    _refused(lib, dgrad(new(w=None)), b"sp_cwconv_dgrad", b"w is NULL")
    d = new()
    _refused(lib, lib.vdetr_sp_cwconv_dgrad_f32(ctypes.byref(d), None, p, p, None), b"sp_cwconv_dgrad", b"inv is NULL")
    _refused(lib, lib.vdetr_sp_cwconv_dgrad_f32(ctypes.byref(d), p, None, p, None), b"sp_cwconv_dgrad", b"dy is NULL")
    _refused(lib, lib.vdetr_sp_cwconv_dgrad_f32(ctypes.byref(d), p, p, None, None), b"sp_cwconv_dgrad", b"dx is NULL")
    for bad, word in ((dict(x=None), b"x is NULL"), (dict(nbr=None), b"nbr is NULL"), (dict(workspace=None), b"workspace is NULL")):
        _refused(lib, wgrad(new(**bad)), b"sp_cwconv_wgrad", word)
    _refused(lib, lib.vdetr_sp_cwconv_wgrad_f32(ctypes.byref(d), None, p, p, None), b"sp_cwconv_wgrad", b"dy is NULL")
    _refused(lib, lib.vdetr_sp_cwconv_wgrad_f32(ctypes.byref(d), p, None, None, None), b"sp_cwconv_wgrad", b"dw is NULL")
    _refused(lib, lib.vdetr_sp_cwconv_fwd_f32(None, None), b"sp_cwconv_fwd", b"null descriptor")
    _refused(lib, lib.vdetr_sp_cwconv_dgrad_f32(None, p, p, p, None), b"sp_cwconv_dgrad", b"null descriptor")
    _refused(lib, lib.vdetr_sp_cwconv_wgrad_f32(None, p, p, p, None), b"sp_cwconv_wgrad", b"null descriptor")


def test_empty_tables_are_no_ops(env):
    _lib, lib, spare = env
    p = spare.ctypes.data
    d = _filled(_lib.SpCwConvDesc(), spare, K=27, nout=0, nin=90, C=8, nbr=None, y=None)
    assert lib.vdetr_sp_cwconv_fwd_f32(ctypes.byref(d), None) == 0
    d = _filled(_lib.SpCwConvDesc(), spare, K=27, nout=100, nin=0, C=8)
    assert lib.vdetr_sp_cwconv_dgrad_f32(ctypes.byref(d), None, None, None, None) == 0
    d = _filled(_lib.SpCwConvDesc(), spare, K=27, nout=0, nin=0, C=8)
    assert lib.vdetr_sp_cwconv_fwd_f32(ctypes.byref(d), None) == 0
    assert lib.vdetr_sp_cwconv_dgrad_f32(ctypes.byref(d), p, p, p, None) == 0
    # the checks come before the no-op
    _refused(lib, lib.vdetr_sp_cwconv_fwd_f32(ctypes.byref(_filled(_lib.SpCwConvDesc(), spare, K=27, nout=0, nin=0, C=6)), None), b"C=6")


def test_workspace_grows_with_nout_and_covers_the_chunks(env):
    _, lib, _ = env
    for K, C in ((1, 4), (27, 64), (125, 1024)):
        prev = 0
        for nout in list(range(0, 2100)) + [4830, 32768, 32769, 35018, 100000, 2 ** 24, 2 ** 31 - 2, 2 ** 31 - 1]:
            rows = lib.vdetr_sp_cwconv_chunk_rows(nout)
            assert rows > 0
            chunks = -(-nout // rows)
            got = lib.vdetr_sp_cwconv_workspace_bytes(K, nout, C)
            assert got >= chunks * (K + 1) * C * 4, (K, nout, C)
            assert got >= prev, (K, nout, C)
            prev = got
    assert lib.vdetr_sp_cwconv_chunk_rows(-7) > 0
    for K, nout, C in ((0, 10, 8), (128, 10, 8), (27, -1, 8), (27, 10, 6), (27, 10, 0), (27, 10, 1028), (-3, -3, -3)):
        assert lib.vdetr_sp_cwconv_workspace_bytes(K, nout, C) == 0
