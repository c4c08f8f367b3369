"""The C ABI of the region-keys launch (csrc/sparse_voxel.hip: vdetr_sp_region_keys_i64): exported and bound, the descriptor's
layout, every argument check an error code whose message names the field before anything is launched, empty tables no-ops.
No GPU needed."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def env():
    from vdetr_amd import _lib
    spare = np.zeros(64, np.uint8)  # an address for the pointer checks; a failed check launches nothing, so nothing follows it
    return _lib, _lib.lib(), spare


def _desc(_lib, spare, **fields):
    d = _lib.SpRegionKeysDesc()
    for name, kind in d._fields_:
        if kind is ctypes.c_void_p:
            setattr(d, name, spare.ctypes.data)
    for name, value in fields.items():
        setattr(d, name, value)
    return d


def _refused(lib, status, *words):
    msg = lib.vdetr_last_error()
    assert status == 1 and all(w in msg for w in (b"sp_region_keys",) + words), (status, msg, words)


def test_entry_point_is_exported_and_bound(env):
    _lib, lib, _ = env
    assert "vdetr_sp_region_keys_i64" in _lib.exported_symbols() and hasattr(lib, "vdetr_sp_region_keys_i64")
    assert lib.vdetr_abi_version() == 3  # additive
    with open(_header()) as fh:
        assert "int vdetr_sp_region_keys_i64(const vdetr_sp_region_keys_desc* d, vdetr_stream_t stream);" in fh.read()


def _header():
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vdetr_hip.h")


def test_descriptor_layout(env):
    _lib, _, _ = env
    D = _lib.SpRegionKeysDesc
    assert [n for n, _ in D._fields_] == ["N", "K", "keys", "offsets", "cand"]
    assert ctypes.sizeof(D) == 32
    assert [getattr(D, n).offset for n in ("N", "K", "keys", "offsets", "cand")] == [0, 4, 8, 16, 24]
    assert D.N.size == D.K.size == 4 and D.keys.size == D.offsets.size == D.cand.size == 8


def test_argument_checks(env):
    _lib, lib, spare = env
    call = lambda **f: lib.vdetr_sp_region_keys_i64(ctypes.byref(_desc(_lib, spare, **f)), None)  # noqa: E731
    _refused(lib, lib.vdetr_sp_region_keys_i64(None, None), b"null descriptor")
    _refused(lib, call(N=-1, K=27), b"N=-1")
    _refused(lib, call(N=10, K=-3), b"K=-3")
    _refused(lib, call(N=-1, K=0), b"N=-1")  # the checks come before the no-op
    for bad, word in ((dict(keys=None), b"keys is NULL"), (dict(offsets=None), b"offsets is NULL"), (dict(cand=None), b"cand is NULL")):
        _refused(lib, call(N=10, K=27, **bad), word)
    # K * N >= 2^31: refused; 32-bit products that wrap are refused as well
    for N, K in ((2 ** 31 - 1, 2), (2 ** 16, 2 ** 15), (2 ** 30, 2), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 16, 2 ** 16), (2 ** 31 - 1, 1025)):
        _refused(lib, call(N=N, K=K), b"31 bits")


def test_empty_tables_are_no_ops(env):
    _lib, lib, spare = env
    for N, K in ((0, 27), (100, 0), (0, 0), (0, 2 ** 31 - 1), (2 ** 31 - 1, 0)):
        d = _desc(_lib, spare, N=N, K=K, keys=None, offsets=None, cand=None)
        assert lib.vdetr_sp_region_keys_i64(ctypes.byref(d), None) == 0, (N, K)
