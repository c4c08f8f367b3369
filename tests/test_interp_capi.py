"""The C ABI of the trilinear interpolation (csrc/sparse_interp.hip: vdetr_sp_interp_map_f32, vdetr_sp_interp_fwd_f32,
vdetr_sp_interp_seg_i32, vdetr_sp_interp_bwd_f32 and the tile query): exported, bound, descriptors laid out as the header says,
argument errors as status codes before anything is launched; and what the host entry points and the MinkowskiEngine-named API
refuse.  No GPU needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

SYMS = ("vdetr_sp_interp_tile", "vdetr_sp_interp_map_f32", "vdetr_sp_interp_fwd_f32", "vdetr_sp_interp_seg_i32", "vdetr_sp_interp_bwd_f32")


def test_entry_points_are_exported_and_bound():
    from vdetr_amd import _lib
    handle = _lib.lib()
    for sym in SYMS:
        assert sym in _lib.exported_symbols(), sym
        assert hasattr(handle, sym), sym
    assert handle.vdetr_abi_version() == 3  # additive: the version and every existing descriptor stay
    tile = handle.vdetr_sp_interp_tile()
    assert tile >= 64 and tile % 64 == 0


@pytest.mark.parametrize("cls_name,c_name,fields,size", [
    ("SpInterpMapDesc", "vdetr_sp_interp_map_desc", ["M", "N", "stride", "keys", "tfield", "nbr", "w"], 3 * 4 + 4 + 4 * 8),
    ("SpInterpDesc", "vdetr_sp_interp_desc", ["M", "N", "C", "x", "nbr", "w", "order", "seg", "y"], 3 * 4 + 4 + 6 * 8)])
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


def _filled(cls, p, **ints):
    d = cls()
    for name, ctype in cls._fields_:
        setattr(d, name, ints[name] if name in ints else p)
    return d


CASES = {
    "sp_interp_map": ("SpInterpMapDesc", "vdetr_sp_interp_map_f32", dict(M=4, N=10, stride=2)),
    "sp_interp_fwd": ("SpInterpDesc", "vdetr_sp_interp_fwd_f32", dict(M=4, N=10, C=3)),
    "sp_interp_bwd": ("SpInterpDesc", "vdetr_sp_interp_bwd_f32", dict(M=4, N=10, C=3)),
}

REFUSED = {
    "sp_interp_map": [(b"N=-1", dict(N=-1)), (b"M=-1", dict(M=-1)), (b"s=0", dict(stride=0)), (b"s=-2", dict(stride=-2)),
                      (b"s=32769", dict(stride=32769)), (b"2^31 pairs", dict(N=2 ** 28)), (b"keys is NULL", dict(keys=None)),
                      (b"tfield is NULL", dict(tfield=None)), (b"nbr is NULL", dict(nbr=None)), (b"w is NULL", dict(w=None)),
                      (b"16-byte aligned", dict(tfield="odd")), (b"16-byte aligned", dict(nbr="odd")), (b"16-byte aligned", dict(w="odd"))],
    "sp_interp_fwd": [(b"C=0", dict(C=0)), (b"C=-4", dict(C=-4)), (b"M=-1", dict(M=-1)), (b"N=-1", dict(N=-1)), (b"2^31 pairs", dict(N=2 ** 28)),
                      (b"x is NULL", dict(x=None)), (b"nbr is NULL", dict(nbr=None)), (b"w is NULL", dict(w=None)), (b"y is NULL", dict(y=None)),
                      (b"16-byte aligned", dict(nbr="odd")), (b"16-byte aligned", dict(w="odd"))],
    "sp_interp_bwd": [(b"C=0", dict(C=0)), (b"M=-1", dict(M=-1)), (b"N=-1", dict(N=-1)), (b"x is NULL", dict(x=None)),
                      (b"w is NULL", dict(w=None)), (b"order is NULL", dict(order=None)), (b"seg is NULL", dict(seg=None)),
                      (b"y is NULL", dict(y=None))],
}


@pytest.mark.parametrize("op", sorted(CASES))
def test_entry_points_reject_bad_arguments(op):
    """every argument error is status 1 with a message that names the entry point and the offending value; nothing is launched"""
    from vdetr_amd import _lib
    lib = _lib.lib()
    keep, p = _spare()
    cls_name, fn_name, ints = CASES[op]
    fn = getattr(lib, fn_name)
    assert fn(None, None) == 1
    assert op.encode() in lib.vdetr_last_error() and b"null descriptor" in lib.vdetr_last_error()
    for text, fields in REFUSED[op]:
        d = _filled(getattr(_lib, cls_name), p, **ints)
        for name, value in fields.items():
            setattr(d, name, p + 4 if value == "odd" else value)
        status = fn(ctypes.byref(d), None)
        err = lib.vdetr_last_error()
        assert status == 1 and op.encode() in err and text in err, (fields, status, err)
    del keep


def test_segment_entry_rejects_bad_arguments():
    from vdetr_amd import _lib
    lib = _lib.lib()
    keep, p = _spare()
    for text, args in ((b"M=-1", (p, p, -1, 4, p, p)), (b"N=-1", (p, p, 4, -1, p, p)), (b"2^31 pairs", (p, p, 4, 2 ** 28, p, p)),
                       (b"seg is NULL", (p, p, 4, 4, p, None)), (b"NULL operand", (None, p, 4, 4, p, p)),
                       (b"NULL operand", (p, None, 4, 4, p, p)), (b"NULL operand", (p, p, 4, 4, None, p))):
        assert lib.vdetr_sp_interp_seg_i32(*args, None) == 1
        err = lib.vdetr_last_error()
        assert b"sp_interp_seg" in err and text in err, (args, err)
    del keep


def test_empty_cases_are_no_ops():
    from vdetr_amd import _lib
    lib = _lib.lib()
    for op, fields in (("sp_interp_map", dict(N=0)), ("sp_interp_map", dict(N=0, M=0)), ("sp_interp_fwd", dict(N=0)),
                       ("sp_interp_fwd", dict(N=0, M=0)), ("sp_interp_bwd", dict(M=0)), ("sp_interp_bwd", dict(M=0, N=0))):
        cls_name, fn_name, ints = CASES[op]
        d = _filled(getattr(_lib, cls_name), None, **dict(ints, **fields))
        assert getattr(lib, fn_name)(ctypes.byref(d), None) == 0, (op, fields)


def test_host_entry_points_refuse_cpu_tensors_dtypes_and_shapes():
    from vdetr_amd import sparse_ops as S
    keys = torch.arange(4, dtype=torch.int64)
    tfield = torch.zeros(5, 4)
    with pytest.raises(RuntimeError, match="keys: CPU not supported"):
        S.interp_map(keys, 1, tfield)
    for bad in (keys.int(), keys.float(), keys.view(2, 2)):
        with pytest.raises(RuntimeError, match="keys must be a one-dimensional int64 key tensor"):
            S.interp_map(bad, 1, tfield)
    for bad in (0, -1, 32769, 1.0, 2.5, True, None):
        with pytest.raises(ValueError, match="tensor_stride"):
            S.interp_map(keys, bad, tfield)
    for bad in (tfield.double(), tfield.int(), tfield.half()):
        with pytest.raises(RuntimeError, match="tfield must be a float tensor"):
            S.interp_map(keys, 1, bad)
    for bad in (torch.zeros(5, 3), torch.zeros(5), torch.zeros(4, 5), torch.zeros(5, 4, 1)):
        with pytest.raises(RuntimeError, match="tfield must be .N, 4."):
            S.interp_map(keys, 1, bad)
    imap = S.InterpMap(torch.full((5, 8), -1, dtype=torch.int32), torch.zeros(5, 8), 4)
    assert (imap.M, imap.N) == (4, 5)
    with pytest.raises(RuntimeError, match="feats: CPU not supported"):
        S.interpolate(torch.zeros(4, 3), imap)
    with pytest.raises(RuntimeError, match="feats has 3 rows, the map 4 sites"):
        S.interpolate(torch.zeros(3, 3), imap)
    with pytest.raises(RuntimeError, match="feats must be a float tensor"):
        S.interpolate(torch.zeros(4, 3, dtype=torch.float64), imap)
    for bad in (torch.zeros(4), torch.zeros(4, 0), torch.zeros(4, 3, 1)):
        with pytest.raises(RuntimeError, match="feats must be a feature table"):
            S.interpolate(bad, imap)
    with pytest.raises(RuntimeError, match="imap must be the InterpMap"):
        S.interpolate(torch.zeros(4, 3), (imap.nbr, imap.w))


def test_module_api_refusals_and_names():
    from vdetr_amd import minkowski as ME
    coords = torch.tensor([[0, 1, 2, 3], [0, 0, 0, 0]], dtype=torch.int32)
    x = ME.SparseTensor(torch.arange(4.0).view(2, 2), coordinates=coords)
    for flags in ((False, False), (True, False), (False, True), (True, True)):
        mod = ME.MinkowskiInterpolation(*flags)
        assert (mod.return_kernel_map, mod.return_weights) == flags and not list(mod.parameters())
    interp = ME.MinkowskiInterpolation()
    with pytest.raises(ValueError, match="a SparseTensor is expected"):
        interp(x.F, torch.zeros(2, 4))
    for bad in (torch.zeros(2, 3), torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(8), [[0, 0, 0, 0]]):
        with pytest.raises(ValueError, match="tfield must be a .N, 4. float32 tensor"):
            interp(x, bad)
    with pytest.raises(RuntimeError, match="keys: CPU not supported"):  # the native map has no CPU form
        interp(x, torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        x.features_at_coordinates(torch.zeros(2, 4))
    for name in ("slice", "cat_slice", "interpolate"):
        with pytest.raises(ValueError, match="a TensorField is expected"):
            getattr(x, name)(torch.zeros(2, 4))
    assert "SPLAT_LINEAR_INTERPOLATION" in ME.TensorField.__doc__ and "NO_QUANTIZATION" in ME.TensorField.__doc__
