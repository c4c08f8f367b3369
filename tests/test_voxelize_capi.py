"""The C ABI of the voxeliser (csrc/sparse_voxel.hip: vdetr_sp_voxel_keys_f32, vdetr_sp_voxel_sites_i64, vdetr_sp_voxel_reduce_f32,
vdetr_sp_voxel_reduce_grad_f32, vdetr_sp_voxel_labels_i32 and their queries): exported, bound, descriptors laid out as the header
says, argument errors as status codes before anything is launched; and what the host entry points and the MinkowskiEngine-named API
refuse.  No GPU needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

SYMS = ("vdetr_sp_voxel_tile", "vdetr_sp_voxel_keys_f32", "vdetr_sp_voxel_sites_workspace_bytes", "vdetr_sp_voxel_sites_i64",
        "vdetr_sp_voxel_reduce_f32", "vdetr_sp_voxel_reduce_grad_f32", "vdetr_sp_voxel_labels_i32")


def test_entry_points_are_exported_and_bound():
    from vdetr_amd import _lib
    handle = _lib.lib()
    for sym in SYMS:
        assert sym in _lib.exported_symbols(), sym
        assert hasattr(handle, sym), sym
    assert handle.vdetr_abi_version() == 3  # additive: the version and every existing descriptor stay
    tile = handle.vdetr_sp_voxel_tile()
    assert tile >= 64 and tile % 64 == 0


@pytest.mark.parametrize("cls_name,c_name,fields,size", [
    ("SpVoxelKeysDesc", "vdetr_sp_voxel_keys_desc", ["N", "B", "stride", "voxel_size", "points", "offsets", "coords", "keys"], 3 * 4 + 4 + 8 + 4 * 8),
    ("SpVoxelSitesDesc", "vdetr_sp_voxel_sites_desc",
     ["N", "sorted", "order", "sites", "first", "inverse", "order32", "seg", "count", "workspace"], 4 + 4 + 9 * 8),
    ("SpVoxelReduceDesc", "vdetr_sp_voxel_reduce_desc", ["M", "N", "C", "mode", "x", "order", "seg", "y", "arg"], 4 * 4 + 5 * 8)])
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
    lines += ['  printf("%d %d %d %d\\n", VDETR_VOXEL_SUM, VDETR_VOXEL_AVG, VDETR_VOXEL_MAX, VDETR_VOXEL_FIRST);', '  return 0;', '}']
    c_file = tmp_path / "layout.c"
    c_file.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(c_file), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    modes = [int(v) for v in got[-4:]]
    got = got[:-4]
    assert len(got) == len(want)
    bad = [(what, int(g), w) for (what, w), g in zip(want, got) if int(g) != w]
    assert not bad, bad
    assert ctypes.sizeof(cls) == size
    assert modes == [_lib.VDETR_VOXEL_SUM, _lib.VDETR_VOXEL_AVG, _lib.VDETR_VOXEL_MAX, _lib.VDETR_VOXEL_FIRST]


def _spare():
    buf = np.zeros(256, np.uint8)
    return buf, (buf.ctypes.data + 15) & ~15


def _filled(cls, p, **ints):
    d = cls()
    for name, ctype in cls._fields_:
        setattr(d, name, ints[name] if name in ints else p)
    return d


CASES = {
    "sp_voxel_keys": ("SpVoxelKeysDesc", "vdetr_sp_voxel_keys_f32", dict(N=10, B=2, stride=3, voxel_size=0.01, coords=None)),
    "sp_voxel_sites": ("SpVoxelSitesDesc", "vdetr_sp_voxel_sites_i64", dict(N=10)),
    "sp_voxel_reduce": ("SpVoxelReduceDesc", "vdetr_sp_voxel_reduce_f32", dict(M=4, N=10, C=3, mode=2)),
}

REFUSED = {
    "sp_voxel_keys": [(b"N=-1", dict(N=-1)), (b"keys is NULL", dict(keys=None)), (b"points is NULL", dict(points=None)),
                      (b"offsets is NULL", dict(offsets=None)), (b"B=0", dict(B=0)), (b"B=32769", dict(B=32769)),
                      (b"row stride 2", dict(stride=2)), (b"voxel_size=0", dict(voxel_size=0.0)), (b"voxel_size=-0.01", dict(voxel_size=-0.01)),
                      (b"voxel_size=inf", dict(voxel_size=float("inf"))), (b"voxel_size=nan", dict(voxel_size=float("nan")))],
    "sp_voxel_sites": [(b"N=-1", dict(N=-1))] + [(name.encode() + b" is NULL", {name: None}) for name in
                                                 ("sorted", "order", "sites", "first", "inverse", "order32", "seg", "count", "workspace")],
    "sp_voxel_reduce": [(b"mode=4", dict(mode=4)), (b"mode=-1", dict(mode=-1)), (b"C=0", dict(C=0)), (b"M=-1", dict(M=-1)),
                        (b"N=3 points for M=4", dict(N=3)), (b"x is NULL", dict(x=None)), (b"order is NULL", dict(order=None)),
                        (b"seg is NULL", dict(seg=None)), (b"y is NULL", dict(y=None)), (b"arg is NULL in max mode", dict(arg=None))],
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
            setattr(d, name, value)
        status = fn(ctypes.byref(d), None)
        err = lib.vdetr_last_error()
        assert status == 1 and op.encode() in err and text in err, (fields, status, err)
    # both inputs at once, and the gradient / label entries
    d = _filled(_lib.SpVoxelKeysDesc, p, **dict(CASES["sp_voxel_keys"][2], coords=p))
    assert lib.vdetr_sp_voxel_keys_f32(ctypes.byref(d), None) == 1 and b"both points and coords" in lib.vdetr_last_error()
    d = _filled(_lib.SpVoxelReduceDesc, p, **CASES["sp_voxel_reduce"][2])
    assert lib.vdetr_sp_voxel_reduce_grad_f32(ctypes.byref(d), p, p, None, None) == 1 and b"dx is NULL" in lib.vdetr_last_error()
    assert lib.vdetr_sp_voxel_reduce_grad_f32(ctypes.byref(d), p, None, p, None) == 1 and b"inverse is NULL" in lib.vdetr_last_error()
    assert lib.vdetr_sp_voxel_reduce_grad_f32(None, p, p, p, None) == 1 and b"null descriptor" in lib.vdetr_last_error()
    assert lib.vdetr_sp_voxel_labels_i32(p, p, p, 5, 4, -100, p, None) == 1 and b"M=5 sites of N=4" in lib.vdetr_last_error()
    assert lib.vdetr_sp_voxel_labels_i32(None, p, p, 4, 5, -100, p, None) == 1 and b"NULL operand" in lib.vdetr_last_error()
    del keep


def test_empty_cases_are_no_ops_and_workspace_sizes():
    from vdetr_amd import _lib
    lib = _lib.lib()
    for op, fields in (("sp_voxel_keys", dict(N=0)), ("sp_voxel_sites", dict(N=0)), ("sp_voxel_reduce", dict(M=0)),
                       ("sp_voxel_reduce", dict(M=0, N=0))):
        cls_name, fn_name, ints = CASES[op]
        d = _filled(getattr(_lib, cls_name), None, **dict(ints, **fields))
        assert getattr(lib, fn_name)(ctypes.byref(d), None) == 0, (op, fields)
    assert lib.vdetr_sp_voxel_labels_i32(None, None, None, 0, 0, -100, None, None) == 0
    tile = lib.vdetr_sp_voxel_tile()
    for n in (0, 1, tile, tile + 1, 400000):
        need = 4 * -(-n // tile)  # a count per tile
        assert need <= lib.vdetr_sp_voxel_sites_workspace_bytes(n) <= need + 2 * 256, n
    assert lib.vdetr_sp_voxel_sites_workspace_bytes(-1) == 0


def test_host_entry_points_refuse_cpu_tensors_dtypes_and_shapes():
    from vdetr_amd import sparse_ops as S
    pts = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="points: CPU not supported"):
        S.voxel_map(pts, [0, 5], 0.01)
    with pytest.raises(RuntimeError, match="coords: CPU not supported"):
        S.voxel_map_coords(torch.zeros(5, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="features: CPU not supported"):
        S.voxel_reduce(pts, None, "sum")
    with pytest.raises(RuntimeError, match="site_features: CPU not supported"):
        S.voxel_slice(pts, None)
    with pytest.raises(RuntimeError, match="labels: CPU not supported"):
        S.voxel_labels(torch.zeros(5, dtype=torch.int64), None)
    assert S.VOXEL_MODES == {"sum": 0, "average": 1, "max": 2, "first": 3}
    # dtypes and shapes (the checks that do not need the tensor on a device come first)
    with pytest.raises(RuntimeError, match="points must be a float tensor"):
        S.voxel_map(pts.double(), [0, 5], 0.01)
    for bad in (torch.zeros(5, 2), torch.zeros(5), torch.zeros(3, 5).t()):
        with pytest.raises(RuntimeError, match="points must be .N, 3 or more columns. with unit column stride"):
            S.voxel_map(bad, [0, 5], 0.01)
    for bad in (0.0, -0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            S.voxel_map(pts, [0, 5], bad)
    with pytest.raises(RuntimeError, match="coords must be .N, 4."):
        S.voxel_map_coords(torch.zeros(5, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="coords must be an integer tensor"):
        S.voxel_map_coords(torch.zeros(5, 4))
    with pytest.raises(RuntimeError, match="labels must be a one-dimensional int32 or int64 tensor"):
        S.voxel_labels(torch.zeros(5), None)


def test_quantization_modes_that_are_not_built():
    from vdetr_amd import minkowski as ME
    modes = ME.SparseTensorQuantizationMode
    assert {m.name for m in modes} == {"RANDOM_SUBSAMPLE", "UNWEIGHTED_AVERAGE", "UNWEIGHTED_SUM", "MAX_POOL", "NO_QUANTIZATION",
                                       "SPLAT_LINEAR_INTERPOLATION"}
    for mode in (modes.NO_QUANTIZATION, modes.SPLAT_LINEAR_INTERPOLATION):
        for call in (lambda: ME.SparseTensor(torch.zeros(2, 3), coordinates=torch.zeros(2, 4, dtype=torch.int32), quantization_mode=mode),
                     lambda: ME.TensorField(torch.zeros(2, 3), torch.zeros(2, 4, dtype=torch.int32), quantization_mode=mode)):
            with pytest.raises(NotImplementedError, match="RANDOM_SUBSAMPLE, UNWEIGHTED_AVERAGE, UNWEIGHTED_SUM and MAX_POOL"):
                call()
    with pytest.raises(ValueError, match="quantization_mode 'median'"):
        ME._quantization_mode("median")
    assert ME._quantization_mode("unweighted_average") is modes.UNWEIGHTED_AVERAGE
    # the default mode on CPU tensors is the composition it always was, now with the inverse map kept
    coords = torch.tensor([[0, 1, 2, 3], [0, 0, 0, 0], [0, 1, 2, 3]], dtype=torch.int32)
    feats = torch.arange(6.0).view(3, 2)
    x = ME.SparseTensor(feats, coordinates=coords)
    assert x.quantization_mode is modes.RANDOM_SUBSAMPLE and x.unique_index.tolist() == [1, 0] and x.inverse_mapping.tolist() == [1, 0, 1]
    assert torch.equal(x.F, feats[[1, 0]])
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ME.SparseTensor(feats, coordinates=coords, quantization_mode=modes.UNWEIGHTED_SUM)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ME.sparse_quantize(coords[:, 1:])
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ME.TensorField(feats, coords)
