"""The C ABI of the sparse pooling and InstanceNorm launches (vdetr_sp_pool_{fwd,bwd}_f32, vdetr_sp_inorm_{fwd,bwd}_f32): exported,
bound, descriptors laid out as the header says, argument errors as status codes before anything is launched, the empty cases as
no-ops.  No GPU needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMS = ("vdetr_sp_pool_fwd_f32", "vdetr_sp_pool_bwd_f32", "vdetr_sp_inorm_fwd_f32", "vdetr_sp_inorm_bwd_f32",
        "vdetr_sp_inorm_workspace_bytes")


def test_entry_points_are_exported_and_bound():
    from vdetr_amd import _lib
    handle = _lib.lib()
    for sym in SYMS:
        assert sym in _lib.exported_symbols(), sym
        assert hasattr(handle, sym), sym
    assert handle.vdetr_abi_version() == 3  # additive: the version and every existing descriptor stay


@pytest.mark.parametrize("cls_name,c_name,fields,size", [
    ("SpPoolDesc", "vdetr_sp_pool_desc", ["K", "nout", "nin", "C", "mode", "x", "nbr", "y", "inv_count", "arg"], 5 * 4 + 4 + 5 * 8),
    ("SpInormDesc", "vdetr_sp_inorm_desc", ["N", "C", "nseg", "eps", "x", "seg", "gamma", "beta", "y", "save_mean", "save_invstd",
                                            "workspace"], 4 * 4 + 8 * 8)])
def test_descriptors_match_the_header(tmp_path, cls_name, c_name, fields, size):
    """sizeof / offsetof of every field, as gcc compiles include/vdetr_hip.h"""
    from vdetr_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    cls = getattr(_lib, cls_name)
    assert [f[0] for f in cls._fields_] == fields
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vdetr_hip.h"', 'int main(void) {',
             f'  printf("%zu\\n", sizeof({c_name}));']
    want = [(f"sizeof({c_name})", ctypes.sizeof(cls))]
    for field in cls._fields_:
        lines.append(f'  printf("%zu\\n", offsetof({c_name}, {field[0]}));')
        want.append((f"offsetof({c_name}, {field[0]})", getattr(cls, field[0]).offset))
    lines += ['  return 0;', '}']
    c_file = tmp_path / "layout.c"
    c_file.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(c_file), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert len(got) == len(want)
    bad = [(what, int(g), w) for (what, w), g in zip(want, got) if int(g) != w]
    assert not bad, bad
    assert ctypes.sizeof(cls) == size


def _spare():
    buf = np.zeros(256, np.uint8)
    return buf, (buf.ctypes.data + 15) & ~15


def _pool(_lib, p, mode=0):
    d = _lib.SpPoolDesc()
    d.K, d.nout, d.nin, d.C, d.mode = 27, 10, 12, 16, mode
    d.x = d.nbr = d.y = p
    d.inv_count = p if mode == 1 else None
    d.arg = p if mode == 2 else None
    return d


def test_pool_entry_points_reject_bad_arguments():
    """every argument error is status 1 with a message that names the entry point and the offending value; nothing is launched"""
    from vdetr_amd import _lib
    lib = _lib.lib()
    keep, p = _spare()

    def fwd(d):
        return lib.vdetr_sp_pool_fwd_f32(ctypes.byref(d), None), b"sp_pool_fwd"

    def bwd(d, inv=True, dy=True, dx=True):
        return lib.vdetr_sp_pool_bwd_f32(ctypes.byref(d), p if inv else None, p if dy else None, p if dx else None, None), b"sp_pool_bwd"

    def refused(call, text, mode=0, **fields):
        d = _pool(_lib, p, mode)
        for name, value in fields.items():
            setattr(d, name, value)
        status, op = call(d)
        err = lib.vdetr_last_error()
        assert status == 1 and op in err and text in err, (fields, status, err)

    assert lib.vdetr_sp_pool_fwd_f32(None, None) == 1
    assert b"sp_pool_fwd" in lib.vdetr_last_error() and b"null descriptor" in lib.vdetr_last_error()
    assert lib.vdetr_sp_pool_bwd_f32(None, None, None, None, None) == 1
    assert b"sp_pool_bwd" in lib.vdetr_last_error() and b"null descriptor" in lib.vdetr_last_error()
    for call in (fwd, bwd):
        refused(call, b"C=18", C=18)
        refused(call, b"C=0", C=0)
        refused(call, b"K=0", K=0)
        refused(call, b"K=128", K=128)
        refused(call, b"K=-2", K=-2)
    for call in (fwd, bwd):
        d = _pool(_lib, p)
        d.mode = 3
        status, op = call(d)
        assert status == 1 and op in lib.vdetr_last_error() and b"mode=3" in lib.vdetr_last_error()
        d.mode = -1
        status, op = call(d)
        assert status == 1 and b"mode=-1" in lib.vdetr_last_error()
        refused(call, b"nout=-1", nout=-1)
        refused(call, b"nin=-4", nin=-4)
    refused(fwd, b"x is NULL", x=None)
    refused(fwd, b"nbr is NULL", nbr=None)
    refused(fwd, b"y is NULL", y=None)
    refused(fwd, b"inv_count is NULL", mode=1, inv_count=None)
    refused(fwd, b"arg is NULL", mode=2, arg=None)
    refused(lambda d: bwd(d, inv=False), b"inv is NULL")
    refused(lambda d: bwd(d, dy=False), b"dy is NULL")
    refused(lambda d: bwd(d, dx=False), b"dx is NULL")
    refused(bwd, b"inv_count is NULL", mode=1, inv_count=None)
    refused(bwd, b"arg is NULL", mode=2, arg=None)
    del keep


def test_pool_empty_tables_are_no_ops():
    from vdetr_amd import _lib
    lib = _lib.lib()
    keep, p = _spare()
    for mode in range(3):
        d = _pool(_lib, p, mode)
        d.nout = 0
        d.x = d.nbr = d.y = d.inv_count = d.arg = None
        assert lib.vdetr_sp_pool_fwd_f32(ctypes.byref(d), None) == 0
        d = _pool(_lib, p, mode)
        d.nin = 0
        assert lib.vdetr_sp_pool_bwd_f32(ctypes.byref(d), None, None, None, None) == 0
    del keep


def _inorm(_lib, p):
    d = _lib.SpInormDesc()
    d.N, d.C, d.nseg, d.eps = 100, 16, 2, 1e-6
    for name in ("x", "seg", "gamma", "beta", "y", "save_mean", "save_invstd", "workspace"):
        setattr(d, name, p)
    return d


def test_inorm_entry_points_reject_bad_arguments():
    from vdetr_amd import _lib
    lib = _lib.lib()
    keep, p = _spare()

    def fwd(d):
        return lib.vdetr_sp_inorm_fwd_f32(ctypes.byref(d), None), b"sp_inorm_fwd"

    def bwd(d, dy=True):
        return lib.vdetr_sp_inorm_bwd_f32(ctypes.byref(d), p if dy else None, p, p, p, None), b"sp_inorm_bwd"

    def refused(call, text, **fields):
        d = _inorm(_lib, p)
        for name, value in fields.items():
            setattr(d, name, value)
        status, op = call(d)
        err = lib.vdetr_last_error()
        assert status == 1 and op in err and text in err, (fields, status, err)

    assert lib.vdetr_sp_inorm_fwd_f32(None, None) == 1
    assert b"sp_inorm_fwd" in lib.vdetr_last_error() and b"null descriptor" in lib.vdetr_last_error()
    assert lib.vdetr_sp_inorm_bwd_f32(None, None, None, None, None, None) == 1
    assert b"sp_inorm_bwd" in lib.vdetr_last_error() and b"null descriptor" in lib.vdetr_last_error()
    for call in (fwd, bwd):
        refused(call, b"C=18", C=18)
        refused(call, b"C=0", C=0)
        refused(call, b"C=1028", C=1028)
        refused(call, b"N=-1", N=-1)
        refused(call, b"nseg=-1", nseg=-1)
        refused(call, b"x is NULL", x=None)
        refused(call, b"seg is NULL", seg=None)
        refused(call, b"save_mean is NULL", save_mean=None)
        refused(call, b"save_invstd is NULL", save_invstd=None)
        refused(call, b"workspace is NULL", workspace=None)
    refused(fwd, b"y is NULL", y=None)
    refused(lambda d: bwd(d, dy=False), b"dy is NULL")
    del keep


def test_inorm_empty_table_is_a_no_op_and_workspace_size():
    from vdetr_amd import _lib
    lib = _lib.lib()
    keep, p = _spare()
    d = _inorm(_lib, p)
    d.N = 0
    d.x = d.y = d.seg = d.save_mean = d.save_invstd = d.workspace = None
    assert lib.vdetr_sp_inorm_fwd_f32(ctypes.byref(d), None) == 0
    assert lib.vdetr_sp_inorm_bwd_f32(ctypes.byref(d), None, None, None, None, None) == 0
    d = _inorm(_lib, p)
    d.nseg = 0
    assert lib.vdetr_sp_inorm_fwd_f32(ctypes.byref(d), None) == 0
    # (count, mean, M2) partials: at most ceil(N / rows) + nseg chunks of >= 16 rows, about 64 per table
    for N, C, nseg in ((1, 4, 1), (567, 64, 2), (36000, 64, 8), (5000, 256, 3)):
        nbytes = lib.vdetr_sp_inorm_workspace_bytes(N, C, nseg)
        assert nbytes % (3 * C * 4) == 0
        chunks = nbytes // (3 * C * 4)
        assert nseg + 1 <= chunks <= 64 + nseg + 1 or N < 16 * 64 and chunks <= -(-N // 16) + nseg + 1, (N, C, nseg, chunks)
    del keep
