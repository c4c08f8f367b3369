"""The C ABI of the eval-mode sparse-convolution epilogue (vdetr_sp_gather_sum_bn_act_f32): exported, bound, its descriptor laid
out as the header says, argument errors as status codes before anything is launched.  No GPU needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYM = "vdetr_sp_gather_sum_bn_act_f32"


def test_entry_point_is_exported_and_bound():
    from vdetr_amd import _lib
    handle = _lib.lib()
    assert SYM in _lib.exported_symbols()
    assert hasattr(handle, SYM)
    assert handle.vdetr_abi_version() == 3  # additive: the version and every existing descriptor stay


def test_descriptor_matches_the_header(tmp_path):
    """sizeof / offsetof of every field of vdetr_sp_gsum_bn_desc, as gcc compiles include/vdetr_hip.h"""
    from vdetr_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    cls, c_name = _lib.SpGsumBnDesc, "vdetr_sp_gsum_bn_desc"
    assert [f[0] for f in cls._fields_] == ["K", "nrows", "C", "src_stride", "act", "eps", "src", "slot", "conv_bias", "gamma", "beta",
                                            "running_mean", "running_var", "residual", "post_add", "out"]
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
    assert ctypes.sizeof(cls) == 6 * 4 + 10 * 8


def _good(_lib, p):
    d = _lib.SpGsumBnDesc()
    d.K, d.nrows, d.C, d.src_stride, d.act, d.eps = 27, 10, 16, 16, 1, 1e-5
    for name in ("src", "slot", "gamma", "beta", "running_mean", "running_var", "out"):
        setattr(d, name, p)
    return d


def test_entry_point_rejects_bad_arguments():
    """every argument error is status 1 with a message that names the entry point and the offending value; nothing is launched
    (no device is needed to get here)"""
    from vdetr_amd import _lib
    lib = _lib.lib()
    fn = getattr(lib, SYM)
    spare = np.zeros(256, np.uint8)
    p = (spare.ctypes.data + 15) & ~15

    def refused(text, **fields):
        d = _good(_lib, p)
        for name, value in fields.items():
            setattr(d, name, value)
        assert fn(ctypes.byref(d), None) == 1, fields
        err = lib.vdetr_last_error()
        assert b"sp_gather_sum_bn_act" in err and text in err, (fields, err)

    assert fn(None, None) == 1
    assert b"sp_gather_sum_bn_act" in lib.vdetr_last_error() and b"null descriptor" in lib.vdetr_last_error()
    refused(b"C=18", C=18, src_stride=20)
    refused(b"C=0", C=0)
    refused(b"src_stride=18", src_stride=18)
    refused(b"src_stride=12", src_stride=12)            # a multiple of 4, but shorter than the row
    refused(b"K=0", K=0)
    refused(b"K=-3", K=-3)
    refused(b"nrows=-1", nrows=-1)
    refused(b"act=3", act=3)
    refused(b"act=-1", act=-1)
    refused(b"running_mean", running_mean=None)
    refused(b"running_var", running_var=None)
    refused(b"slot", slot=None)
    refused(b"out", out=None)
    refused(b"running_mean", running_mean=None, nrows=0)  # checked before the empty table returns


def test_empty_table_is_a_no_op():
    from vdetr_amd import _lib
    lib = _lib.lib()
    spare = np.zeros(256, np.uint8)
    d = _good(_lib, (spare.ctypes.data + 15) & ~15)
    d.nrows = 0
    d.slot = d.out = d.src = None
    assert getattr(lib, SYM)(ctypes.byref(d), None) == 0
