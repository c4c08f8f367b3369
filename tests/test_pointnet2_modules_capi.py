"""The C ABI of the fused PointNet++ layers (vdetr_group_mlp_pack_f32, vdetr_sa_mlp_max_infer_f32, vdetr_fp_mlp_infer_f32):
exported, bound, their descriptors laid out as the header says, argument errors as status codes.  No GPU needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ("vdetr_group_mlp_pack_f32", "vdetr_sa_mlp_max_infer_f32", "vdetr_fp_mlp_infer_f32")


def test_entry_points_are_exported_and_bound():
    from vdetr_amd import _lib
    handle = _lib.lib()
    for sym in NEW:
        assert sym in _lib.exported_symbols(), sym
        assert hasattr(handle, sym), sym
    assert handle.vdetr_abi_version() == 3  # additive: the version and every existing descriptor stay


def test_descriptors_match_the_header(tmp_path):
    """sizeof / offsetof of every field of the three descriptors, as gcc compiles include/vdetr_hip.h"""
    from vdetr_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    pairs = [(_lib.GroupMlpDesc, "vdetr_group_mlp_desc"), (_lib.SaMlpDesc, "vdetr_sa_mlp_desc"), (_lib.FpMlpDesc, "vdetr_fp_mlp_desc")]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vdetr_hip.h"', 'int main(void) {']
    want = []
    for cls, c_name in pairs:
        lines.append(f'  printf("%zu\\n", sizeof({c_name}));')
        want.append((f"sizeof({c_name})", ctypes.sizeof(cls)))
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
    assert ctypes.sizeof(_lib.GroupMlpDesc) == 24 + 9 * 8
    assert ctypes.sizeof(_lib.SaMlpDesc) == 32 + 5 * 8 + 96 and ctypes.sizeof(_lib.FpMlpDesc) == 24 + 5 * 8 + 96


def test_entry_points_reject_bad_arguments():
    """argument errors are status codes with a message, checked before anything is launched"""
    from vdetr_amd import _lib
    lib = _lib.lib()
    spare = np.zeros(256, np.uint8)
    p = (spare.ctypes.data + 15) & ~15
    assert lib.vdetr_sa_mlp_max_infer_f32(None, None) == 1
    assert b"sa_mlp_max_infer" in lib.vdetr_last_error()
    d = _lib.SaMlpDesc()
    d.B, d.N, d.M, d.S, d.C, d.use_xyz = 1, 100, 10, 6, 0, 1
    assert lib.vdetr_sa_mlp_max_infer_f32(ctypes.byref(d), None) == 1
    assert b"S=6" in lib.vdetr_last_error()
    d.S = 16
    d.mlp.nlayers, d.mlp.cin = 4, 3
    assert lib.vdetr_sa_mlp_max_infer_f32(ctypes.byref(d), None) == 1
    assert b"nlayers=4" in lib.vdetr_last_error()
    d.mlp.nlayers, d.mlp.cin = 1, 4
    assert lib.vdetr_sa_mlp_max_infer_f32(ctypes.byref(d), None) == 1
    assert b"cin=4" in lib.vdetr_last_error()
    d.mlp.cin = 3
    d.mlp.width[0] = 40
    d.mlp.wt[0] = d.mlp.scale[0] = d.mlp.shift[0] = p
    assert lib.vdetr_sa_mlp_max_infer_f32(ctypes.byref(d), None) == 1
    assert b"width[0]=40" in lib.vdetr_last_error()
    d.mlp.width[0] = 48
    assert lib.vdetr_sa_mlp_max_infer_f32(ctypes.byref(d), None) == 1  # xyz, new_xyz, idx, out are NULL
    assert b"null operand" in lib.vdetr_last_error()
    d.C = 4  # features missing
    assert lib.vdetr_sa_mlp_max_infer_f32(ctypes.byref(d), None) == 1
    assert b"features" in lib.vdetr_last_error()
    f = _lib.FpMlpDesc()
    f.B, f.n, f.m, f.C1, f.C2 = 1, 70, 3, 0, 0
    assert lib.vdetr_fp_mlp_infer_f32(ctypes.byref(f), None) == 1
    assert b"fp_mlp_infer" in lib.vdetr_last_error() and b"C2=0" in lib.vdetr_last_error()
    f.C2 = 600
    f.mlp.nlayers, f.mlp.cin = 1, 600
    assert lib.vdetr_fp_mlp_infer_f32(ctypes.byref(f), None) == 1
    assert b"cin=600" in lib.vdetr_last_error()
    assert lib.vdetr_group_mlp_pack_f32(None, None, None, None, None, None, 1e-5, 3, 16, None, None, None, None) == 1
    assert b"group_mlp_pack" in lib.vdetr_last_error()
    assert lib.vdetr_group_mlp_pack_f32(p, None, p, None, None, None, 1e-5, 3, 16, p, p, p, None) == 1
    assert b"go together" in lib.vdetr_last_error()
