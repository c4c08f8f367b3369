"""CPU: the vertex-normals entry points of include/vdetr_hip.h are exported, their descriptor's ctypes mirror has the header's
layout, the workspace formula holds, argument errors come back as status codes with a message, and the public functions
refuse CPU tensors, bad host faces and clouds that are not six columns wide."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("vdetr_vertex_normals_workspace_bytes", "vdetr_vertex_normals_f32")


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
    for name in ("VDETR_NORMALS_TILE", "VDETR_NORMALS_SCAN_TILE", "VDETR_NORMALS_SHORT"):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == getattr(_lib, name), name


def test_descriptor_mirror_has_the_headers_layout(tmp_path):
    from vdetr_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    cls = _lib.NormalsDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vdetr_hip.h"', 'int main(void) {',
             '  printf("%zu\\n", sizeof(vdetr_normals_desc));']
    want = [ctypes.sizeof(cls)]
    for name, _ in cls._fields_:
        lines.append(f'  printf("%zu\\n", offsetof(vdetr_normals_desc, {name}));')
        want.append(getattr(cls, name).offset)
    lines += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert ctypes.sizeof(cls) == 4 * 4 + 5 * 8 and cls.vertices.offset == 16


def host(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_workspace_formula():
    from vdetr_amd import _lib
    lib = _lib.lib()
    voff, foff = np.array([0, 300, 1813], np.int32), np.array([0, 0, 1000], np.int32)
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    # N = 1813 vertices, F = 1000 faces, T = 2 scan tiles of 1024: w [F,3] f32, counts / starts / cursors [N], tile sums [T], lists [3F]
    want = up(1000 * 3 * 4) + 3 * up(1813 * 4) + up(2 * 4) + up(3 * 1000 * 4) + 256
    assert want == 12032 + 3 * 7424 + 256 + 12032 + 256
    assert lib.vdetr_vertex_normals_workspace_bytes(host(voff), host(foff), 2) == want
    assert lib.vdetr_vertex_normals_workspace_bytes(host(voff), host(foff), 0) == 0
    assert lib.vdetr_vertex_normals_workspace_bytes(None, host(foff), 2) == 0 and lib.vdetr_vertex_normals_workspace_bytes(host(voff), None, 2) == 0


def test_argument_errors_are_status_codes():
    from vdetr_amd import _lib
    lib = _lib.lib()
    voff, foff = np.array([0, 300, 1813], np.int32), np.array([0, 0, 1000], np.int32)
    d = _lib.NormalsDesc()
    d.B, d.vert_stride, d.out_stride = 2, 3, 3
    call = lambda v, f, desc=d: lib.vdetr_vertex_normals_f32(ctypes.byref(desc) if desc is not None else None, v, f, None, 0, None)  # noqa: E731
    assert call(host(voff), host(foff)) == 1
    assert b"null pointer" in lib.vdetr_last_error()
    assert call(None, host(foff)) == 1
    assert b"null descriptor or offsets" in lib.vdetr_last_error()
    assert call(host(voff), None) == 1
    assert b"null descriptor or offsets" in lib.vdetr_last_error()
    assert call(host(voff), host(foff), None) == 1
    assert b"null descriptor or offsets" in lib.vdetr_last_error()
    empty = np.array([0, 300, 300], np.int32)
    assert call(host(empty), host(foff)) == 1
    assert b"scene 1 has no vertices" in lib.vdetr_last_error()
    back = np.array([0, 10, 5], np.int32)
    assert call(host(voff), host(back)) == 1
    assert b"face offsets decrease at scene 1" in lib.vdetr_last_error()
    late = np.array([4, 300, 1813], np.int32)
    assert call(host(late), host(foff)) == 1
    assert b"not at 0" in lib.vdetr_last_error()
    many = np.array([0, 0, 715827883], np.int32)                       # 3F = 2^31 + 1
    assert call(host(voff), host(many)) == 1
    assert b"below 2^31" in lib.vdetr_last_error()
    assert lib.vdetr_vertex_normals_workspace_bytes(host(voff), host(many), 2) == 0
    d.vert_stride = 2
    assert call(host(voff), host(foff)) == 1
    assert b"xyz needs 3" in lib.vdetr_last_error()
    d.vert_stride, d.out_stride = 3, 1
    assert call(host(voff), host(foff)) == 1
    assert b"xyz needs 3" in lib.vdetr_last_error()
    d.out_stride, d.B = 3, 5000
    assert call(host(voff), host(foff)) == 1
    assert b"scenes" in lib.vdetr_last_error()
    d.B = 0
    assert call(host(voff), host(foff)) == 0                            # no scenes: no-op


def test_the_public_functions_refuse_cpu_tensors():
    import torch
    from vdetr_amd.scene_prep import vertex_normals, with_normals
    xyz, faces = torch.zeros(10, 3), np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        vertex_normals(xyz, np.array([0, 10]), faces, np.array([0, 2]))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        vertex_normals(xyz, np.array([0, 4, 10]), torch.from_numpy(faces).long(), np.array([0, 1, 2]))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        with_normals(torch.zeros(10, 6), torch.zeros(10, 3))


def test_host_faces_are_range_checked():
    import torch
    from vdetr_amd.scene_prep import vertex_normals
    xyz = torch.zeros(10, 3)
    for bad in ([[0, 1, -1]], [[0, 10, 2]], [[0, 1, 2], [3, 4, 5], [0, 1, 6]]):   # the last: 6 is outside the second scene of 6
        with pytest.raises(ValueError, match="outside their scene"):
            vertex_normals(xyz, np.array([0, 4, 10]) if len(bad) == 3 else np.array([0, 10]), np.array(bad, np.int64),
                           np.array([0, 1, 3]) if len(bad) == 3 else np.array([0, 1]))
    with pytest.raises(ValueError, match="int32 / int64"):
        vertex_normals(xyz, np.array([0, 10]), np.zeros((2, 3), np.float32), np.array([0, 2]))
    with pytest.raises(ValueError, match="no vertices"):
        vertex_normals(xyz, np.array([0, 10, 10]), np.zeros((2, 3), np.int32), np.array([0, 1, 2]))
    with pytest.raises(ValueError, match="may not decrease"):
        vertex_normals(xyz, np.array([0, 4, 10]), np.zeros((2, 3), np.int32), np.array([0, 3, 2]))


def test_with_normals_takes_six_columns_only():
    import torch
    from vdetr_amd.scene_prep import with_normals
    for width in (3, 9):
        with pytest.raises(ValueError, match=r"must be \[N, 6\]"):
            with_normals(torch.zeros(10, width), torch.zeros(10, 3))
    with pytest.raises(ValueError, match="normals must be"):
        with_normals(torch.zeros(10, 6), torch.zeros(9, 3))
