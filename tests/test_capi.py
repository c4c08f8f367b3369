"""The C-ABI library loads on a CPU-only machine and exports every symbol include/vdetr_hip.h declares."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT


def header_symbols():
    text = open(os.path.join(ROOT, "include", "vdetr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vdetr_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    from vdetr_amd import _lib
    assert header_symbols() == _lib.exported_symbols()


def test_library_exports_every_symbol():
    from vdetr_amd import _lib
    handle = _lib.lib()
    for sym in header_symbols():
        assert hasattr(handle, sym), sym
    assert handle.vdetr_abi_version() == 3


def test_descriptor_layout():
    from vdetr_amd import _lib
    # 6x4 | ptr | 3x4 + pad | 3 ptr | ptr | 2x4 | 2x8 | ptr | 2x4 | ptr | 4x4 | ptr   (ABI 3: the launch-shape fields)
    assert ctypes.sizeof(_lib.AttnDesc) == 168
    assert _lib.AttnDesc.table_grid.offset == 128 and _lib.AttnDesc.kv_halves.offset == 144 and _lib.AttnDesc.kv_img.offset == 152 and _lib.AttnDesc.fwd_sched.offset == 160
    assert _lib.AttnDesc.table.offset == 24 and _lib.AttnDesc.vertices.offset == 48
    assert _lib.AttnDesc.seed.offset == 88 and _lib.AttnDesc.rng_state.offset == 104


def test_argument_errors_do_not_exit():
    """status codes + vdetr_last_error instead of the reference's exit(-1) (cuda_utils.h:32-41)."""
    from vdetr_amd import _lib
    lib = _lib.lib()
    assert lib.vdetr_gather_points_f32(None, None, None, -1, 1, 1, 1, None) == 1
    assert b"negative" in lib.vdetr_last_error()
    assert lib.vdetr_furthest_point_sampling_f32(None, 1, 0, 4, None, None, 0, None) == 1
    assert lib.vdetr_furthest_point_sampling_f32(None, 1, 10, 0, None, None, 0, None) == 0  # m <= 0: no-op
    # the sorted cloud in 64-slot segments of tree-leaf buckets: at most 2 ceil(n / 64) + 64 of them
    assert 40000 * 20 + 256 <= lib.vdetr_fps_workspace_bytes(1, 40000) <= (2 * 625 + 64) * 64 * 20 + 256
    d = _lib.AttnDesc()
    d.kind, d.B, d.H, d.nQ, d.nK = 0, 1, 3, 4, 4
    assert lib.vdetr_attn_fwd_f32(ctypes.byref(d), None, None, None, None, None, None, None, 0, None) == 1
    assert b"4 heads" in lib.vdetr_last_error()


def test_round2_entry_points_reject_bad_arguments():
    """the sparse-convolution / Morton entry points added in round 2: argument errors are status codes with a message"""
    from vdetr_amd import _lib
    lib = _lib.lib()
    assert lib.vdetr_sp_pair_plan_workspace_ints(27, 1000) == 27 * 4
    assert lib.vdetr_sp_pair_plan_i32(None, 0, 10, 10, None, None, None, None, None, None, None) == 1
    assert b"sp_pair_plan" in lib.vdetr_last_error()
    assert lib.vdetr_sp_wgrad_reduce_f32(None, None, 27, 6, None, None) == 1      # elems not a multiple of 4
    assert b"sp_wgrad_reduce" in lib.vdetr_last_error()
    assert lib.vdetr_morton_sort_max() == 16384
    assert lib.vdetr_morton_order_f32(None, 1, 16, None, None, None) == 1
    assert b"morton_order" in lib.vdetr_last_error()
    assert lib.vdetr_sp_pairs_gemm_f32(None, None, None, None, 5, 24, 64, 0, None, None) == 1
    assert b"sp_pairs_gemm" in lib.vdetr_last_error()
    assert lib.vdetr_sp_pairs_gemm_f32(None, None, None, None, 0, 16, 16, 0, None, None) == 0   # no tiles: no-op


def test_round3_attention_backward_entry_points_reject_bad_arguments():
    """vdetr_attn_bwd_kv_f32 / vdetr_attn_bwd_table_f32 / the workgroup-shape setter (round 3): status codes + message."""
    from vdetr_amd import _lib
    lib = _lib.lib()
    d = _lib.AttnDesc()
    d.kind, d.B, d.H, d.nQ, d.nK, d.scale = _lib.VDETR_ATTN_SHARED_KV, 1, 4, 64, 100, 0.125
    # packed operand images: 3 kinds x 4 sub-operands x (hi, lo) x 64 lanes x 16 B per 32-row tile; rows = 4 heads x nQ
    assert lib.vdetr_attn_bwd_kv_workspace_bytes(ctypes.byref(d)) == (64 * 4 // 32) * 3 * 4 * 2 * 64 * 16 + 256
    assert lib.vdetr_attn_bwd_kv_f32(ctypes.byref(d), None, None, None, None, None, None, None, None, None, None, 0, None) == 1
    assert b"attn_bwd_kv" in lib.vdetr_last_error()
    d.kind = _lib.VDETR_ATTN_PER_HEAD
    d.H = 3  # per-head K/V: one problem per (scene, head), rows = queries
    assert lib.vdetr_attn_bwd_kv_workspace_bytes(ctypes.byref(d)) == 3 * (64 // 32) * 3 * 4 * 2 * 64 * 16 + 256
    d.kind, d.H = _lib.VDETR_ATTN_SHARED_KV, 4
    assert lib.vdetr_attn_bwd_table_f32(ctypes.byref(d), None, None, None, 0, None) == 1   # no dS, no table, no bwd_aux
    assert b"attn_bwd_table" in lib.vdetr_last_error()
    assert lib.vdetr_ab_switches() == 0  # the shipped build reads no environment switch


def test_round5_operand_image_entry_points():
    """vdetr_attn_kv_image_bytes / vdetr_attn_pack_kv_f32 and their part-count forms (round 5: the forward's K / V operand images;
    parts 3 = f32 accuracy, 1 = operands rounded to bf16): sizes by the layout (attn_fwd_pipe.hip: a 16-key tile is 6 + 4 pieces
    of 64 lanes x 16 B with three parts, 2 + 2 with one), argument errors as status codes."""
    from vdetr_amd import _lib
    lib = _lib.lib()
    tiles = (4096 + 15) // 16
    assert lib.vdetr_attn_kv_image_bytes(1, 4096) == lib.vdetr_attn_kv_image_parts_bytes(1, 4096, 3) == tiles * 10 * 64 * 16
    assert lib.vdetr_attn_kv_image_parts_bytes(1, 4096, 1) == tiles * 4 * 64 * 16
    assert lib.vdetr_attn_kv_image_parts_bytes(2, 301, 1) == 2 * 19 * 4 * 64 * 16          # ragged key count: whole tiles
    assert lib.vdetr_attn_kv_image_parts_bytes(1, 4096, 2) == 0 and lib.vdetr_attn_kv_image_parts_bytes(0, 4096, 1) == 0
    assert lib.vdetr_attn_pack_kv_f32(None, None, 1, 4096, 64, 64, 1, 0, None, None) == 1
    assert b"attn_pack_kv" in lib.vdetr_last_error()
    assert lib.vdetr_attn_pack_kv_parts_f32(None, None, 1, 4096, 64, 64, 1, 0, 1, None, None) == 1
    assert b"attn_pack_kv" in lib.vdetr_last_error()
    buf = (ctypes.c_char * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    ptr = ctypes.c_void_p((ptr.value + 15) & ~15)
    assert lib.vdetr_attn_pack_kv_parts_f32(ptr, ptr, 1, 4096, 64, 64, 1, 0, 2, ptr, None) == 1   # no such part count
    assert b"parts=2" in lib.vdetr_last_error()
    assert lib.vdetr_attn_pack_kv_parts_f32(ptr, ptr, 1, 4096, 62, 64, 1, 0, 1, ptr, None) == 1   # rows shorter than 64 floats
    assert b"attn_pack_kv" in lib.vdetr_last_error()


def test_scene_preparation_entry_points_keep_their_messages():
    """The eight launch entry points of scene_prep.hip, cuboid.hip, color_aug.hip and normals.hip: an empty scene and a missing
    workspace (the six that take one) are refused on the host, before any launch, with exactly these texts.  They were recorded
    from the library as it was before the four files came to share csrc/scene_tiles.h."""
    import numpy as np
    from vdetr_amd import _lib
    lib = _lib.lib()
    spare = np.zeros(64, np.uint8)                                       # an address for the pointer checks; nothing follows it

    def filled(d, **fields):
        for name, kind in d._fields_:
            if kind is ctypes.c_void_p:
                setattr(d, name, spare.ctypes.data)
        for name, value in fields.items():
            setattr(d, name, value)
        return ctypes.byref(d)

    prep = filled(_lib.ScenePrepDesc(), B=2, C=3, G=4, max_obj=64)
    crop = filled(_lib.CuboidDesc(), B=2, W=3, G=4, T=100, min_points=10, num_points=16)
    color = filled(_lib.ColorAugDesc(), B=2, W=6, noise_rows=813, out=spare.ctypes.data + 32)
    mesh = filled(_lib.NormalsDesc(), B=2, vert_stride=3, out_stride=3)
    faces = np.array([0, 10, 20], np.int32).ctypes.data_as(ctypes.c_void_p)
    calls = {"scene_prep_points": lambda off: lib.vdetr_scene_prep_points_f32(prep, off, None, 0, None),
             "scene_prep_targets": lambda off: lib.vdetr_scene_prep_targets_f32(prep, off, None, 0, None),
             "cuboid_crop": lambda off: lib.vdetr_cuboid_crop_f32(crop, off, None, 0, None),
             "cuboid_compose": lambda off: lib.vdetr_cuboid_compose_i32(crop, off, None),
             "color_augment": lambda off: lib.vdetr_color_augment_f32(color, off, None, 0, None),
             "append_height": lambda off: lib.vdetr_append_height_f32(color, off, None, 0, None),
             "sunrgbd_color": lambda off: lib.vdetr_sunrgbd_color_f32(color, off, None),
             "vertex_normals": lambda off: lib.vdetr_vertex_normals_f32(mesh, off, faces, None, 0, None)}
    empty = np.array([0, 300, 300], np.int32)
    no_rows = {"scene_prep_points": b"scene_prep: scene 1 has no points (offsets 300 .. 300)",
               "scene_prep_targets": b"scene_prep: scene 1 has no points (offsets 300 .. 300)",
               "cuboid_crop": b"cuboid: scene 1 has no points (offsets 300 .. 300)",
               "cuboid_compose": b"cuboid: scene 1 has no points (offsets 300 .. 300)",
               "color_augment": b"color_augment: scene 1 has no points (offsets 300 .. 300)",
               "append_height": b"append_height: scene 1 has no points (offsets 300 .. 300)",
               "sunrgbd_color": b"sunrgbd_color: scene 1 has no points (offsets 300 .. 300)",
               "vertex_normals": b"vertex_normals: scene 1 has no vertices (offsets 300 .. 300)"}
    assert sorted(no_rows) == sorted(calls)
    for name, text in no_rows.items():
        assert calls[name](empty.ctypes.data_as(ctypes.c_void_p)) == 1, name
        assert lib.vdetr_last_error() == text, name
    good = np.array([0, 300, 813], np.int32)
    no_workspace = {"scene_prep_points": b"scene_prep: workspace 0 B < required 376 B",
                    "scene_prep_targets": b"scene_prep: workspace 0 B < required 376 B",
                    "cuboid_crop": b"cuboid_crop: workspace 0 B < required 24576 B",
                    "color_augment": b"color_augment: workspace 0 B < required 768 B",
                    "append_height": b"append_height: workspace 0 B < required 6656 B",
                    "vertex_normals": b"vertex_normals: workspace 0 B < required 11008 B"}
    for name, text in no_workspace.items():                              # cuboid_compose and sunrgbd_color take no workspace
        assert calls[name](good.ctypes.data_as(ctypes.c_void_p)) == 3, name
        assert lib.vdetr_last_error() == text, name


def test_ops_refuse_cpu_tensors():
    """No CPU fallback: the reference asserts "CPU not supported" (sampling.cpp:36,62,84)."""
    from vdetr_amd import pointnet2_utils as PU
    from vdetr_amd import attention as A
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.furthest_point_sample(torch.rand(1, 16, 3), 4)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.gather_operation(torch.rand(1, 4, 16), torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        A.fused_attention(torch.rand(1, 4, 256), torch.rand(1, 8, 64), torch.rand(1, 8, 64), num_heads=4, scale=0.125,
                          shared_kv=True)


def test_build_rejects_the_packed_multiply_form_of_design_4_4b():
    """build.py disassembles the library and refuses `v_pk_mul/fma_f32` with a high-broadcast second source."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("vdetr_build", os.path.join(root, "v-detr_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b._hi_broadcast(" v[0:1], v[2:3], v[4:5] op_sel:[0,1]")                      # the failing kernel's form
    assert b._hi_broadcast(" v[0:1], v[2:3], v[4:5], v[0:1] op_sel:[1,1,0] op_sel_hi:[0,1,1]")
    assert not b._hi_broadcast(" v[0:1], v[2:3], v[4:5] op_sel:[0,1] op_sel_hi:[1,0]")  # crossed: fine
    assert not b._hi_broadcast(" v[0:1], v[2:3], v[4:5] op_sel_hi:[1,0]")               # low-broadcast: fine
    assert not b._hi_broadcast(" v[0:1], v[2:3], v[4:5] op_sel:[1,0]")                  # first source: covered by parity tests
    assert not b._hi_broadcast(" v[0:1], v[2:3], v[4:5]")
    assert b.check_code_objects(b.build()) >= 15  # every .hip of the library is a code object, none has the form


def test_every_ctypes_mirror_has_the_headers_layout(tmp_path):
    """include/vdetr_hip.h compiled by gcc: sizeof and the offset of every field of every struct that v-detr_amd/_lib.py mirrors
    (the class's docstring names it) — a descriptor that drifts from its mirror is a launch reading garbage, on the GPU only."""
    import re
    import shutil
    import subprocess
    import sys
    from vdetr_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = open(_lib.__file__).read()
    pairs = re.findall(r'class (\w+)\(ctypes\.Structure\):\n\s+"""Mirror of ``(\w+)``', src)
    assert len(pairs) >= 28
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vdetr_hip.h"', 'int main(void) {']
    want = []
    for cls_name, c_name in pairs:
        cls = getattr(_lib, cls_name)
        lines.append(f'  printf("%zu\\n", sizeof({c_name}));')
        want.append((f"sizeof({c_name})", ctypes.sizeof(cls)))
        for field in cls._fields_:
            name = field[0]
            lines.append(f'  printf("%zu\\n", offsetof({c_name}, {name}));')
            want.append((f"offsetof({c_name}, {name})", getattr(cls, name).offset))
    lines += ['  return 0;', '}']
    c_file = tmp_path / "layout.c"
    c_file.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([gcc, "-std=c11", "-I", os.path.join(root, "include"), str(c_file), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert len(got) == len(want)
    bad = [(what, int(g), w) for (what, w), g in zip(want, got) if int(g) != w]
    assert not bad, bad


def _attn_desc(_lib, spare, kind=0, B=1, H=4, nQ=1024, nK=4096, T=10, **flags):
    """a descriptor for the size functions and the host checks: they read fields only, so `spare` stands in for every pointer"""
    d = _lib.AttnDesc()
    d.kind, d.B, d.H, d.nQ, d.nK, d.scale = kind, B, H, nQ, nK, 0.125
    if T:
        d.table, d.table_size, d.vertices, d.xyz = spare, T, spare, spare
    for name, value in flags.items():
        setattr(d, name, spare if value is True else value)
    return d


def test_workspace_sizes_keep_their_byte_counts():
    """What the *_workspace_bytes functions of nms.hip, fps.hip, attn_bwd.hip, attn_bwd_kv.hip and attn_fwd.hip answer.  Every
    figure was recorded from the library as it was before these files came to write their layouts once, on a Carver
    (csrc/workspace.h): callers have sized buffers by them, so they stay what they were, to the byte.  Without a device the
    library counts 256 compute units."""
    import numpy as np
    from vdetr_amd import _lib
    lib = _lib.lib()
    spare = np.zeros(64, np.uint8).ctypes.data
    per_head = _lib.VDETR_ATTN_PER_HEAD
    small = dict(B=2, nQ=12, nK=272)                                     # key split 2, ragged last tile
    fwd = {"T 10": (dict(), 6882048),                                    # counter, four key splits' partials, K/V image
           "T 10, fwd_sched": (dict(fwd_sched=True), 6881792),
           "T 10, kv_img": (dict(kv_img=True), 4260352),
           "T 10, fwd_sched and kv_img": (dict(fwd_sched=True, kv_img=True), 4260096),
           "T 10, fwd_kernel 1": (dict(fwd_kernel=1), 4260096),
           "T 10, fwd_kernel 3": (dict(fwd_kernel=3), 6882048),
           "T 6": (dict(T=6), 4260096),
           "T 10, mask": (dict(mask=True, mask_kind=_lib.VDETR_MASK_BOOL), 4260096),
           "small, T 10": (dict(small), 398848),
           "small, T 10, kv_img": (dict(small, kv_img=True), 50432),
           "small, T 10, fwd_kernel 2": (dict(small, fwd_kernel=2), 50432),
           "small, no table": (dict(small, T=0), 50176),
           "64 keys, T 10": (dict(nK=64), 41472),                        # no key split: counter and image
           "64 keys, T 10, kv_img": (dict(nK=64, kv_img=True), 256),     # the counter alone
           "per-head": (dict(kind=per_head, nQ=1024, nK=1024, T=0), 0)}
    for name, (fields, want) in fwd.items():
        assert lib.vdetr_attn_fwd_workspace_bytes(ctypes.byref(_attn_desc(_lib, spare, **fields))) == want, name
    bwd = {"no table": (dict(T=0), 0), "T 10, 1024 queries": (dict(), 32768256), "T 10, 8 queries": (dict(nQ=8), 1024256),
           "T 6": (dict(T=6), 7078144)}
    for name, (fields, want) in bwd.items():
        assert lib.vdetr_attn_bwd_workspace_bytes(ctypes.byref(_attn_desc(_lib, spare, **fields))) == want, name
    bwd_kv = {"shared, H 4": (dict(T=0), 3145984), "per-head, B 2, H 4, nQ 100": (dict(kind=per_head, B=2, nQ=100, T=0), 786688),
              "shared, H 8": (dict(H=8, T=0), 0)}
    for name, (fields, want) in bwd_kv.items():
        assert lib.vdetr_attn_bwd_kv_workspace_bytes(ctypes.byref(_attn_desc(_lib, spare, **fields))) == want, name
    fps = {(1, 40000): 1682176, (2, 300): 189696, (1, 300000): 6000896, (0, 5): 0}
    for (b, n), want in fps.items():
        assert lib.vdetr_fps_workspace_bytes(b, n) == want, (b, n)
    fps_varlen = {(300, 130): 184576, (40000,): 1682176, (20000,) * 4: 3533056}
    for counts, want in fps_varlen.items():
        arr = np.array(counts, np.int32)
        assert lib.vdetr_fps_varlen_workspace_bytes(arr.ctypes.data, len(counts)) == want, counts
    nms = {(1, 256): (15616, 34048), (2, 70): (6912, 16896), (4, 4096): (8847616, 10027264), (0, 5): (0, 0)}
    for (B, K), (want, want_rot) in nms.items():
        assert lib.vdetr_nms3d_workspace_bytes(B, K) == want, (B, K)
        assert lib.vdetr_nms3d_rot_workspace_bytes(B, K) == want_rot, (B, K)


def test_workspace_entry_points_keep_their_messages():
    """A missing workspace (NULL, 0) is refused on the host, before any launch, with status 3 and exactly these texts: they were
    recorded from the library as it was before nms.hip, fps.hip, attn_bwd.hip, attn_bwd_kv.hip and attn_fwd.hip came to share
    require_workspace (csrc/workspace.h).  All eight entry points reach the check without a device.  Two more rows: the bf16
    forward refuses a caller's K/V image (an image of f32 parts is not what it reads), and vdetr_attn_pack_kv_f32, now the
    three-part form of vdetr_attn_pack_kv_parts_f32, still refuses short rows."""
    import numpy as np
    from vdetr_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(4096, np.uint8)                                       # addresses for the pointer checks; nothing follows them
    base = (buf.ctypes.data + 255) & ~255
    p = [base + 256 * i for i in range(11)]

    def desc(**fields):
        return ctypes.byref(_attn_desc(_lib, p[0], B=2, nQ=12, nK=272, **fields))

    counts = np.array([300, 130], np.int32)
    scenes = ctypes.cast((ctypes.c_void_p * 2)(p[1], p[2]), ctypes.c_void_p)
    nms_args = (p[0], p[1], p[2], p[3], p[4], 2, 70, 0.25, 0, p[5], None, 0, None)
    no_workspace = [
        (lambda: lib.vdetr_nms3d_f32(*nms_args), b"nms3d: workspace 0 B < required 6912 B"),
        (lambda: lib.vdetr_nms3d_rot_f32(*nms_args), b"nms3d_rot: workspace 0 B < required 16896 B"),
        (lambda: lib.vdetr_furthest_point_sampling_f32(p[0], 2, 300, 16, p[1], None, 0, None),
         b"furthest_point_sampling: workspace 0 B < required 189696 B"),
        (lambda: lib.vdetr_furthest_point_sampling_varlen_f32(scenes, counts.ctypes.data, 2, 16, p[3], None, 0, None),
         b"furthest_point_sampling_varlen: workspace 0 B < required 184576 B"),
        (lambda: lib.vdetr_attn_fwd_f32(desc(), p[1], p[2], p[3], p[4], p[5], None, None, 0, None),
         b"attn_fwd: workspace 0 B < required 398848 B"),
        (lambda: lib.vdetr_attn_fwd_bf16(desc(), p[1], p[2], p[3], p[4], p[5], None, None, 0, None),
         b"attn_fwd_bf16: workspace 0 B < required 398848 B"),
        (lambda: lib.vdetr_attn_bwd_kv_f32(desc(), *p[1:10], None, 0, None), b"attn_bwd_kv: workspace 0 B < required 98560 B"),
        (lambda: lib.vdetr_attn_bwd_scores_f32(desc(), p[1], p[2], p[3], p[4], p[5], p[6], p[7], None, 0, None),
         b"attn_bwd_scores: workspace 0 B < required 3072256 B")]
    for call, text in no_workspace:
        assert call() == 3, text
        assert lib.vdetr_last_error() == text
    assert lib.vdetr_attn_fwd_bf16(desc(kv_img=True), p[1], p[2], p[3], p[4], p[5], None, p[6], 1 << 20, None) == 1
    assert lib.vdetr_last_error().startswith(b"attn_fwd_bf16:") and b"kv_img" in lib.vdetr_last_error()
    assert lib.vdetr_attn_pack_kv_f32(p[1], p[2], 1, 4096, 62, 64, 1, 0, p[3], None) == 1
    assert lib.vdetr_last_error() == b"attn_pack_kv: rows of >= 64 floats, strides multiples of 4, 16-B aligned"
