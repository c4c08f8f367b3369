"""CPU: the cuboid entry points of include/vdetr_hip.h are exported, their descriptor's ctypes mirror has the header's layout,
and argument errors come back as status codes with a message."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("vdetr_cuboid_workspace_bytes", "vdetr_cuboid_crop_f32", "vdetr_cuboid_compose_i32")


def test_symbols_are_declared_bound_and_exported():
    from vdetr_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vdetr_hip.h")).read(), flags=re.S)
    handle = _lib.lib()
    for sym in SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", text), sym
        assert sym in _lib.exported_symbols() and hasattr(handle, sym), sym
    assert handle.vdetr_abi_version() == 3                              # additive: the ABI version stays


def test_constants_agree_with_the_header():
    from vdetr_amd import _lib
    text = open(os.path.join(ROOT, "include", "vdetr_hip.h")).read()
    for name in ("VDETR_CUBOID_TILE", "VDETR_CUBOID_MAX_TRIALS", "VDETR_CUBOID_TRIAL", "VDETR_CUBOID_RESULT"):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == getattr(_lib, name), name


def test_descriptor_mirror_has_the_headers_layout(tmp_path):
    from vdetr_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    cls = _lib.CuboidDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vdetr_hip.h"', 'int main(void) {',
             '  printf("%zu\\n", sizeof(vdetr_cuboid_desc));']
    want = [ctypes.sizeof(cls)]
    for name, _ in cls._fields_:
        lines.append(f'  printf("%zu\\n", offsetof(vdetr_cuboid_desc, {name}));')
        want.append(getattr(cls, name).offset)
    lines += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert ctypes.sizeof(cls) == 8 * 4 + 13 * 8 and cls.points.offset == 32


def test_argument_errors_are_status_codes():
    from vdetr_amd import _lib
    lib = _lib.lib()
    off = np.array([0, 300, 813], np.int32)
    host = off.ctypes.data_as(ctypes.c_void_p)
    tiles = 2 + 3
    # 9 floats per tile | 6 doubles per scene and attempt | 7 words per tile and attempt | 1 word per tile, each rounded to 256 B
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    assert lib.vdetr_cuboid_workspace_bytes(host, 2, 100) == up(tiles * 36) + up(2 * 100 * 48) + up(tiles * 100 * 28) + up(tiles * 4) + 256
    assert lib.vdetr_cuboid_workspace_bytes(host, 0, 100) == 0 and lib.vdetr_cuboid_workspace_bytes(None, 2, 100) == 0
    d = _lib.CuboidDesc()
    d.B, d.W, d.G, d.T, d.min_points, d.num_points = 2, 3, 4, 100, 10, 16
    assert lib.vdetr_cuboid_crop_f32(ctypes.byref(d), host, None, 0, None) == 1
    assert b"null pointer" in lib.vdetr_last_error()
    d.T = 0
    assert lib.vdetr_cuboid_crop_f32(ctypes.byref(d), host, None, 0, None) == 1
    assert b"attempts" in lib.vdetr_last_error()
    d.T, d.min_points = 100, 0
    assert lib.vdetr_cuboid_crop_f32(ctypes.byref(d), host, None, 0, None) == 1
    assert b"min_points" in lib.vdetr_last_error()
    d.min_points = 10
    empty = np.array([0, 300, 300], np.int32)
    assert lib.vdetr_cuboid_crop_f32(ctypes.byref(d), empty.ctypes.data_as(ctypes.c_void_p), None, 0, None) == 1
    assert b"no points" in lib.vdetr_last_error()
    d.num_points = 0
    assert lib.vdetr_cuboid_compose_i32(ctypes.byref(d), host, None) == 1
    assert b"num_points" in lib.vdetr_last_error()
    d.B = 0
    assert lib.vdetr_cuboid_crop_f32(ctypes.byref(d), host, None, 0, None) == 0          # no scenes: no-op


def test_crop_and_sample_refuses_cpu_tensors():
    import torch
    from vdetr_amd.scene_prep import crop_and_sample
    with pytest.raises(RuntimeError, match="CPU not supported"):
        crop_and_sample(torch.zeros(10, 3), np.array([0, 10]), torch.zeros(1, 2, 6), torch.zeros(1, dtype=torch.int64),
                        torch.zeros(1, 2, dtype=torch.int64), [np.random.RandomState(0)], 8, min_points=2)
