"""CPU: the scan-export entry points of include/vdetr_hip.h are exported, their descriptor's ctypes mirror has the header's
layout, the workspace formula holds, argument errors come back as status codes with a message before anything is launched, and
``export_scans`` refuses CPU tensors, bad shapes, bad offsets and tables that do not fit."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_scan_export_restatement import LABEL_MAP

SYMBOLS = ("vdetr_scan_export_workspace_bytes", "vdetr_scan_export_f32")


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
    for name in ("VDETR_EXPORT_TILE", "VDETR_EXPORT_MAX_INSTANCES"):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == getattr(_lib, name), name
    assert _lib.VDETR_EXPORT_MAX_INSTANCES >= 512
    assert _lib.VDETR_EXPORT_MAX_INSTANCES * 6 * 4 <= 64 * 1024         # the [K, 6] table of 32-bit keys fits a workgroup's LDS
    assert _lib.VDETR_EXPORT_TILE % 64 == 0 and _lib.VDETR_EXPORT_TILE <= 1024


def test_descriptor_mirror_has_the_headers_layout(tmp_path):
    from vdetr_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    cls = _lib.ScanExportDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vdetr_hip.h"', 'int main(void) {',
             '  printf("%zu\\n", sizeof(vdetr_scan_export_desc));']
    want = [ctypes.sizeof(cls)]
    for name, _ in cls._fields_:
        lines.append(f'  printf("%zu\\n", offsetof(vdetr_scan_export_desc, {name}));')
        want.append(getattr(cls, name).offset)
    lines += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert ctypes.sizeof(cls) == 8 * 4 + 22 * 8 and cls.vertices.offset == 32


def host(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_workspace_formula():
    from vdetr_amd import _lib
    lib = _lib.lib()
    off = np.array([0, 300, 1813], np.int32)
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    # 1 + 3 tiles of 512 rows, 40 object slots: partials [4, 40, 6] u32, two [4] i32 arrays
    want = up(4 * 40 * 6 * 4) + 2 * up(4 * 4) + 256
    assert want == 3840 + 512 + 256
    assert lib.vdetr_scan_export_workspace_bytes(host(off), 2, 40) == want
    assert lib.vdetr_scan_export_workspace_bytes(host(off), 2, 0) == 2 * 256 + 256
    assert lib.vdetr_scan_export_workspace_bytes(host(off), 0, 40) == 0 and lib.vdetr_scan_export_workspace_bytes(None, 2, 40) == 0
    assert lib.vdetr_scan_export_workspace_bytes(host(off), 2, _lib.VDETR_EXPORT_MAX_INSTANCES + 1) == 0
    assert lib.vdetr_scan_export_workspace_bytes(host(np.array([0, 300, 300], np.int32)), 2, 40) == 0


def test_argument_errors_are_status_codes():
    """every one of these returns before a launch: the descriptor's pointers are null"""
    from vdetr_amd import _lib
    lib = _lib.lib()
    off, counts = np.array([0, 300, 1813], np.int32), np.array([3, 40], np.int32)
    d = _lib.ScanExportDesc()
    d.B, d.W, d.vert_stride, d.Kmax = 2, 6, 7, 40
    call = lambda o=off, c=counts, desc=d: lib.vdetr_scan_export_f32(ctypes.byref(desc) if desc is not None else None,  # noqa: E731
                                                                    host(o) if o is not None else None,
                                                                    host(c) if c is not None else None, None, 0, None)
    assert call() == 1
    assert b"null pointer" in lib.vdetr_last_error()
    for kw in (dict(o=None), dict(c=None), dict(desc=None)):
        assert call(**kw) == 1
        assert b"null descriptor, offsets or instance counts" in lib.vdetr_last_error()
    assert call(c=np.array([3, 41], np.int32)) == 1
    assert b"scene 1 has 41 objects, 40 slots" in lib.vdetr_last_error()
    assert call(c=np.array([-1, 4], np.int32)) == 1
    assert b"scene 0 has -1 objects" in lib.vdetr_last_error()
    assert call(o=np.array([0, 300, 300], np.int32)) == 1
    assert b"scene 1 has no points" in lib.vdetr_last_error()
    assert call(o=np.array([4, 300, 1813], np.int32)) == 1
    assert b"not at 0" in lib.vdetr_last_error()
    d.Kmax = _lib.VDETR_EXPORT_MAX_INSTANCES + 1
    assert call() == 1
    assert b"object slots" in lib.vdetr_last_error()
    d.Kmax, d.W = 40, 2
    assert call() == 1
    assert b"3 <= W <= stride" in lib.vdetr_last_error()
    d.W, d.vert_stride = 8, 7
    assert call() == 1
    assert b"3 <= W <= stride" in lib.vdetr_last_error()
    d.W, d.num_segments = 6, -1
    assert call() == 1
    assert b"negative table length" in lib.vdetr_last_error()
    d.num_segments, d.B = 0, 5000
    assert call() == 1
    assert b"scenes" in lib.vdetr_last_error()
    d.B = 0
    assert call() == 0                                                  # no scenes: no-op


def tables_for(n, K=1):
    from vdetr_amd.scan_export import scan_tables
    groups = [{"objectId": k, "label": "chair", "segments": [k]} for k in range(K)]
    return scan_tables(np.arange(n) % max(K, 1), groups, LABEL_MAP)


def cfg():
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    return ScannetDatasetConfig()


def test_export_scans_refuses_cpu_tensors():
    import torch
    from vdetr_amd.scan_export import export_scans
    with pytest.raises(RuntimeError, match="CPU not supported"):
        export_scans(torch.zeros(10, 6), np.array([0, 10]), [tables_for(10)], cfg())
    with pytest.raises(RuntimeError, match="CPU not supported"):
        export_scans(torch.zeros(10, 7)[:, :6], np.array([0, 4, 10]), [tables_for(4), tables_for(6, 2)], cfg(), donotcare_ids=(1, 2))


def test_shape_and_offset_errors_raise_value_errors():
    import torch
    from vdetr_amd import _lib
    from vdetr_amd.scan_export import export_scans
    v = torch.zeros(10, 6)
    with pytest.raises(ValueError, match="6 or more columns"):
        export_scans(torch.zeros(10, 3), np.array([0, 10]), [tables_for(10)], cfg())
    with pytest.raises(ValueError, match="unit column stride"):
        export_scans(torch.zeros(6, 10).t(), np.array([0, 10]), [tables_for(10)], cfg())
    with pytest.raises(RuntimeError, match="float tensor"):
        export_scans(v.double(), np.array([0, 10]), [tables_for(10)], cfg())
    for bad in ([0, 9], [1, 10], [0, 12]):
        with pytest.raises(ValueError, match="vert_offsets run from"):
            export_scans(v, np.array(bad), [tables_for(bad[1] - bad[0])], cfg())
    with pytest.raises(ValueError, match="scene 1 has no vertices"):
        export_scans(v, np.array([0, 10, 10]), [tables_for(10), tables_for(1)], cfg())
    with pytest.raises(ValueError, match="2 scan tables for 1 scenes"):
        export_scans(v, np.array([0, 10]), [tables_for(10), tables_for(10)], cfg())
    with pytest.raises(ValueError, match="tables made for 7 vertices, the scene has 10"):
        export_scans(v, np.array([0, 10]), [tables_for(7)], cfg())
    with pytest.raises(KeyError):
        export_scans(v, np.array([0, 10]), [tables_for(10)], cfg(), obj_class_ids=(3, 4, 13))       # 13 has no class index
    with pytest.raises(ValueError, match="donotcare_ids"):
        export_scans(v, np.array([0, 10]), [tables_for(10)], cfg(), donotcare_ids=(-1,))
    # one object too many, in tables made by hand (scan_tables itself refuses to make them): refused on the host
    K = _lib.VDETR_EXPORT_MAX_INSTANCES
    t = tables_for(K, K)
    t.num_instances, t.object_label = K + 1, np.zeros(K + 1, np.int32)
    with pytest.raises(ValueError, match="VDETR_EXPORT_MAX_INSTANCES"):
        export_scans(torch.zeros(K, 6), np.array([0, K]), [t], cfg())
