"""The C ABI of the inference forms (vdetr_heads_infer_f32, vdetr_pos_mlp_infer_f32, vdetr_rb_qkv_pos_infer_f32): exported, bound,
their descriptors laid out as the header says, argument errors as status codes.  No GPU needed."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NEW = ("vdetr_heads_infer_f32", "vdetr_pos_mlp_infer_f32", "vdetr_rb_qkv_pos_infer_f32")


def test_inference_entry_points_are_exported_and_bound():
    from vdetr_amd import _lib
    handle = _lib.lib()
    for sym in NEW:
        assert sym in _lib.exported_symbols(), sym
        assert hasattr(handle, sym), sym
    assert handle.vdetr_abi_version() == 3  # additive: the version and every existing descriptor stay


def test_inference_descriptors_match_the_header(tmp_path):
    """sizeof / offsetof of every field of the descriptors the new entry points take, as gcc compiles include/vdetr_hip.h"""
    from vdetr_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    pairs = [(_lib.HeadsInferDesc, "vdetr_heads_infer_desc"), (_lib.PosMlpDesc, "vdetr_posmlp_desc"),
             (_lib.RbQkvDesc, "vdetr_rb_qkv_desc")]
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
    assert ctypes.sizeof(_lib.HeadsInferDesc) == 24 + 14 * 8


def test_inference_entry_points_reject_bad_arguments():
    """argument errors are status codes with a message, checked before anything is launched"""
    from vdetr_amd import _lib
    lib = _lib.lib()
    assert lib.vdetr_heads_infer_f32(None, None) == 1
    assert b"heads_infer" in lib.vdetr_last_error()
    d = _lib.HeadsInferDesc()
    d.B, d.N, d.G, d.rows, d.tile = 1, 1024, 5, 19, 24
    assert lib.vdetr_heads_infer_f32(ctypes.byref(d), None) == 1
    assert b"tile=24" in lib.vdetr_last_error()
    d.tile, d.G = 0, 9
    assert lib.vdetr_heads_infer_f32(ctypes.byref(d), None) == 1
    assert b"G=9" in lib.vdetr_last_error()
    d.G, d.N, d.tile = 5, 1000, 32
    assert lib.vdetr_heads_infer_f32(ctypes.byref(d), None) == 1
    assert b"multiple of 32" in lib.vdetr_last_error()
    d.N = 1024
    assert lib.vdetr_heads_infer_f32(ctypes.byref(d), None) == 1  # every pointer NULL
    assert b"null" in lib.vdetr_last_error()
    m = _lib.PosMlpDesc()
    m.B, m.N, m.cin = 1, 1024, 6
    assert lib.vdetr_pos_mlp_infer_f32(ctypes.byref(m), None) == 1
    assert b"pos_mlp_infer: null" in lib.vdetr_last_error()
    m.cin = 9
    assert lib.vdetr_pos_mlp_infer_f32(ctypes.byref(m), None) == 1
    assert b"cin=9" in lib.vdetr_last_error()
    q = _lib.RbQkvDesc()
    q.rows, q.B = 1024, 1
    assert lib.vdetr_rb_qkv_pos_infer_f32(ctypes.byref(q), ctypes.byref(m), None) == 1
    assert b"rb_qkv_pos_infer" in lib.vdetr_last_error()


def test_inference_switches_are_module_attributes():
    """the A/B switch is heads.INFER (monkeypatched by tests, set by tools/infer_bench.py); inference = eval AND autograd off"""
    import torch
    from vdetr_amd import heads as HD
    m = torch.nn.Linear(2, 2)
    assert HD.INFER is True and HD.INFER_TILE == 0
    m.eval()
    with torch.no_grad():
        assert HD.inference(m)
    with torch.inference_mode():
        assert HD.inference(m)
    assert not HD.inference(m)  # eval mode with autograd on keeps today's path
    m.train()
    with torch.no_grad():
        assert not HD.inference(m)
