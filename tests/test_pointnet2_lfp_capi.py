"""The C ABI of the fused post MLP of PointnetLFPModuleMSG (vdetr_pw_mlp_infer_f32): exported, bound, its descriptor laid out as
the header says, argument errors as status codes checked before anything is launched.  No GPU needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYM = "vdetr_pw_mlp_infer_f32"


def test_entry_point_is_exported_and_bound():
    from vdetr_amd import _lib
    handle = _lib.lib()
    assert SYM in _lib.exported_symbols() and hasattr(handle, SYM)
    assert handle.vdetr_abi_version() == 3  # additive: the version and every existing descriptor stay


def test_descriptor_matches_the_header(tmp_path):
    """sizeof / offsetof of every field of vdetr_pw_mlp_desc, as gcc compiles include/vdetr_hip.h"""
    from vdetr_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    cls, c_name = _lib.PwMlpDesc, "vdetr_pw_mlp_desc"
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
    assert ctypes.sizeof(cls) == 32 + 6 * 8 + ctypes.sizeof(_lib.GroupMlpDesc) == 176


def test_entry_point_rejects_bad_arguments():
    from vdetr_amd import _lib
    lib = _lib.lib()
    fn = lib.vdetr_pw_mlp_infer_f32
    spare = np.zeros(256, np.uint8)
    p = (spare.ctypes.data + 15) & ~15

    def rejected(d, *words):
        assert fn(ctypes.byref(d) if d is not None else None, None) == 1
        msg = lib.vdetr_last_error()
        assert b"pw_mlp_infer" in msg, msg
        for word in words:
            assert word in msg, msg

    rejected(None, b"null descriptor")
    d = _lib.PwMlpDesc()
    d.B, d.n, d.Ck, d.C2 = 2, 9, 16, 4
    d.mlp.nlayers, d.mlp.cin, d.mlp.width[0] = 1, 20, 48
    d.mlp.wt[0] = d.mlp.scale[0] = d.mlp.shift[0] = p
    d.features2 = p
    d.out_channels = 96
    for k in (0, 5):
        d.K = k
        rejected(d, b"K=%d" % k)
    d.K = 2
    d.mlp.cin = 21
    rejected(d, b"cin=21", b"Ck=16", b"C2=4")
    d.mlp.cin = 20
    d.features2 = None  # C2 > 0 without the tensor
    rejected(d, b"features2")
    d.features2 = p
    d.C2, d.mlp.cin = 0, 16  # ... and the tensor without C2
    rejected(d, b"features2")
    d.C2, d.mlp.cin = 4, 20
    d.out_channel0 = 1  # 1 + 2 x 48 > 96
    rejected(d, b"out_channel0=1", b"out_channels=96")
    d.out_channel0, d.out_channels = 0, 95
    rejected(d, b"out_channels=95")
    d.out_channels = 96
    d.mlp.width[0] = 40
    rejected(d, b"width[0]=40")
    d.mlp.width[0] = 48
    d.mlp.nlayers = 4
    rejected(d, b"nlayers=4")
    d.mlp.nlayers = 1
    d.B = 0
    rejected(d, b"B=0")
    d.B = 2
    rejected(d, b"null operand")  # pooled and out are NULL: the last check, nothing was launched
    d.out = p
    d.pooled[0] = p
    rejected(d, b"null operand")  # pooled[1] of K = 2
    d.B, d.n, d.K = 1 << 15, 1 << 15, 4
    d.out_channels = 192
    rejected(d, b"2^31")
