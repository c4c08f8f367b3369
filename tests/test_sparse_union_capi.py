"""The C ABI of the union / pruning launches (vdetr_sp_union_map_i64, vdetr_sp_prune_map_i64, vdetr_sp_union_add_f32,
vdetr_sp_take_rows_f32 and their size functions): exported, bound, descriptors laid out as the header says, argument errors as
status codes before anything is launched, the empty cases as no-ops.  No GPU needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMS = ("vdetr_sp_union_tile", "vdetr_sp_union_map_workspace_bytes", "vdetr_sp_union_map_i64", "vdetr_sp_prune_map_workspace_bytes",
        "vdetr_sp_prune_map_i64", "vdetr_sp_union_add_f32", "vdetr_sp_take_rows_f32")


def test_entry_points_are_exported_and_bound():
    from vdetr_amd import _lib
    handle = _lib.lib()
    for sym in SYMS:
        assert sym in _lib.exported_symbols(), sym
        assert hasattr(handle, sym), sym
    assert handle.vdetr_abi_version() == 3  # additive: the version and every existing descriptor stay
    tile = handle.vdetr_sp_union_tile()
    assert tile >= 64 and tile % 64 == 0


@pytest.mark.parametrize("cls_name,c_name,fields,size", [
    ("SpUnionMapDesc", "vdetr_sp_union_map_desc", ["na", "nb", "a", "b", "u", "row_a", "row_b", "src_a", "src_b", "count", "workspace"],
     2 * 4 + 9 * 8),
    ("SpPruneMapDesc", "vdetr_sp_prune_map_desc", ["N", "mask", "keys", "kept", "pos", "keys_out", "count", "workspace"], 4 + 4 + 7 * 8),
    ("SpUnionAddDesc", "vdetr_sp_union_add_desc", ["nu", "na", "nb", "C", "sign", "a", "b", "src_a", "src_b", "y"], 5 * 4 + 4 + 5 * 8),
    ("SpTakeRowsDesc", "vdetr_sp_take_rows_desc", ["nrows", "nsrc", "C", "sign", "x", "idx", "y"], 4 * 4 + 3 * 8)])
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
    "sp_union_map": ("SpUnionMapDesc", "vdetr_sp_union_map_i64", dict(na=10, nb=12)),
    "sp_prune_map": ("SpPruneMapDesc", "vdetr_sp_prune_map_i64", dict(N=10)),
    "sp_union_add": ("SpUnionAddDesc", "vdetr_sp_union_add_f32", dict(nu=14, na=10, nb=12, C=16, sign=1)),
    "sp_take_rows": ("SpTakeRowsDesc", "vdetr_sp_take_rows_f32", dict(nrows=14, nsrc=10, C=16, sign=-1)),
}

REFUSED = {
    "sp_union_map": [(b"na=-1", dict(na=-1)), (b"nb=-3", dict(nb=-3)), (b"na=2147483647 + nb=12", dict(na=2 ** 31 - 1)),
                     (b"a is NULL", dict(a=None)), (b"b is NULL", dict(b=None)), (b"u is NULL", dict(u=None)),
                     (b"row_a is NULL", dict(row_a=None)), (b"row_b is NULL", dict(row_b=None)), (b"src_a is NULL", dict(src_a=None)),
                     (b"src_b is NULL", dict(src_b=None)), (b"count is NULL", dict(count=None)), (b"workspace is NULL", dict(workspace=None))],
    "sp_prune_map": [(b"N=-1", dict(N=-1)), (b"mask is NULL", dict(mask=None)), (b"keys is NULL", dict(keys=None)),
                     (b"kept is NULL", dict(kept=None)), (b"pos is NULL", dict(pos=None)), (b"keys_out is NULL", dict(keys_out=None)),
                     (b"count is NULL", dict(count=None)), (b"workspace is NULL", dict(workspace=None))],
    "sp_union_add": [(b"C=6", dict(C=6)), (b"C=0", dict(C=0)), (b"C=-4", dict(C=-4)), (b"sign=0", dict(sign=0)), (b"sign=2", dict(sign=2)),
                     (b"nu=-1", dict(nu=-1)), (b"na=-2", dict(na=-2)), (b"nb=-5", dict(nb=-5)), (b"src_a is NULL", dict(src_a=None)),
                     (b"src_b is NULL", dict(src_b=None)), (b"y is NULL", dict(y=None)), (b"a is NULL with na=10", dict(a=None)),
                     (b"b is NULL with nb=12", dict(b=None))],
    "sp_take_rows": [(b"C=6", dict(C=6)), (b"C=0", dict(C=0)), (b"sign=0", dict(sign=0)), (b"sign=-2", dict(sign=-2)),
                     (b"nrows=-1", dict(nrows=-1)), (b"nsrc=-7", dict(nsrc=-7)), (b"idx is NULL", dict(idx=None)), (b"y is NULL", dict(y=None)),
                     (b"x is NULL with nsrc=10", dict(x=None))],
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
    del keep


def test_empty_cases_are_no_ops():
    """no rows to write: status 0 without a launch, whatever the pointers (NULL included)"""
    from vdetr_amd import _lib
    lib = _lib.lib()
    empties = {"sp_union_map": [dict(na=0, nb=0)], "sp_prune_map": [dict(N=0)],
               "sp_union_add": [dict(nu=0), dict(nu=0, na=0), dict(nu=0, nb=0), dict(nu=0, na=0, nb=0)],
               "sp_take_rows": [dict(nrows=0), dict(nrows=0, nsrc=0)]}
    for op, cases in empties.items():
        cls_name, fn_name, ints = CASES[op]
        for fields in cases:
            d = _filled(getattr(_lib, cls_name), None, **dict(ints, **fields))
            assert getattr(lib, fn_name)(ctypes.byref(d), None) == 0, (op, fields)


def test_workspace_sizes():
    from vdetr_amd import _lib
    lib = _lib.lib()
    tile = lib.vdetr_sp_union_tile()
    for na, nb in ((0, 0), (1, 0), (0, 1), (tile, tile + 1), (35018, 280144)):
        need = 4 * (na + nb) + 4 * (-(-na // tile) + -(-nb // tile))  # a word per key, a count per tile
        got = lib.vdetr_sp_union_map_workspace_bytes(na, nb)
        assert need <= got <= need + 3 * 256, (na, nb, got)
    for n in (0, 1, tile, tile + 1, 280144):
        need = 4 * -(-n // tile)
        assert need <= lib.vdetr_sp_prune_map_workspace_bytes(n) <= need + 2 * 256, n
    assert lib.vdetr_sp_union_map_workspace_bytes(-1, 4) == 0 and lib.vdetr_sp_prune_map_workspace_bytes(-1) == 0
