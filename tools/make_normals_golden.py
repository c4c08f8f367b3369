#!/usr/bin/env python3
"""Generates tests/golden/normals.npz from the reference's own loader (build container only, like
tools/make_color_aug_golden.py, whose import recipe it reuses).

A one-scan directory is written, ``ScannetDetectionDataset`` is constructed on it with ``use_color=True, use_normals=True`` and
the case's settings, ``datasets.scannet.read_plymesh`` is replaced by a function that returns the case's ``(vertices7, faces)``
(no ``.ply`` is ever read), and ``__getitem__`` is called under ``np.random.seed(s)``.  It wraps; it does not restate: the file
holds the inputs, the settings, the seed, the returned ``point_clouds`` and the generator's state after the call.  The plain
cases run with ``augment=False``, so that columns 6:9 of the result are the normals of every vertex; ``chain`` runs the whole
training loader.

The cases are the ones DESIGN.md 6.6 lists; tests/test_normals_restatement.py (``cases_present``) asserts what each has to
hold, here and again on every test run, among them that summing the fan's hub in reversed face order changes its bits.

    python tools/make_normals_golden.py
"""
import os
import sys
import tempfile
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_scene_prep_golden as SPG  # noqa: E402
from oracle import make_golden as MG  # noqa: E402
import color_aug_restatement as CA  # noqa: E402
import normals_restatement as NR  # noqa: E402
from test_normals_restatement import CASES, FAN_FACES, SETTINGS, cases_present, settings_of  # noqa: E402


def run_reference(S, vert, ply_vertices, faces, box, seed, s):
    rot, trans, scale = s["ratios"]
    split = "train" if s["augment"] else "val"
    with tempfile.TemporaryDirectory() as tmp:
        data, meta = os.path.join(tmp, "data"), os.path.join(tmp, "meta")
        os.makedirs(data)
        os.makedirs(meta)
        name = "scene0000_00"
        np.save(os.path.join(data, name + "_vert.npy"), vert)
        np.save(os.path.join(data, name + "_bbox.npy"), box)
        np.save(os.path.join(data, name + "_ins_label.npy"), np.zeros(len(vert), np.int64))
        np.save(os.path.join(data, name + "_sem_label.npy"), np.zeros(len(vert), np.int64))
        with open(os.path.join(meta, f"scannetv2_{split}.txt"), "w") as fh:
            fh.write(name + "\n")
        args = Namespace(dataset_root_dir=data, meta_data_dir=meta, num_points=int(s["num_points"]), use_color=True,
                         color_mean=float(s["color_mean"]), rot_ratio=rot, scale_ratio=scale, trans_ratio=trans, use_superpoint=False,
                         filt_empty=False, use_normals=True, color_drop=float(s["color_drop"]), color_contrastp=float(s["color_contrastp"]),
                         color_jitterp=float(s["color_jitterp"]), hue_sat=str(s["hue_sat"]), coloraug_sunrgbd=bool(s["coloraug_sunrgbd"]))
        ds = S.ScannetDetectionDataset(S.ScannetDatasetConfig(), split_set=split, use_height=bool(s["use_height"]), augment=bool(s["augment"]),
                                       use_random_cuboid=bool(s["use_random_cuboid"]), random_cuboid_min_points=int(s["min_points"]),
                                       args=args)
        real = S.read_plymesh
        S.read_plymesh = lambda path: (ply_vertices.copy(), faces.copy())
        try:
            np.random.seed(seed)
            with np.errstate(all="ignore"):
                ret = ds[0]
        finally:
            S.read_plymesh = real
        return ret["point_clouds"].numpy(), np.random.get_state()


def record(arrays, name, S, xyz, faces, ids, want=lambda t: True, seeds=range(400), rng=None, **settings):
    s = dict(SETTINGS, **settings)
    n = len(xyz)
    vert, box = SPG.scan(rng, n, 3, ids, colours=True)
    vert[:, :3] = xyz                                                  # the prepared scan holds the mesh's vertices
    ply = np.concatenate([vert, np.full((n, 1), 255, np.float32)], 1)  # x y z r g b a, float32 as read_plymesh returns them
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    colour_settings = {k: v for k, v in s.items() if k != "augment"}
    for seed in seeds:
        if not s["augment"] or want(CA.color_augment_scene(vert, np.random.RandomState(seed), **colour_settings)[1]):
            break
    else:
        raise AssertionError(f"{name}: no seed gives the case")
    out, state = run_reference(S, vert, ply, faces, box, seed, s)
    rs = np.random.RandomState(seed)
    mine = NR.loader_scene(vert, ply, faces, box, rs, s)
    assert mine.tobytes() == out.tobytes(), name
    a = {"vert": vert, "ply_vertices": ply, "faces": faces, "boxes7": box, "seed": np.array(seed), "out_points": out,
         "state_keys": state[1], "state_pos": np.array(state[2])}
    for k, v in s.items():
        a[f"set_{k}"] = np.array(v)
    cases_present(name, a, s)
    for k, v in a.items():
        arrays[f"{name}:{k}"] = v
    print(f"{name}: seed {seed}, {n} vertices, {len(faces)} faces -> {out.shape}")


def height_field(rng, nx, ny):
    """a triangulated nx x ny height field with noise in a 8 x 6 x 3 m room: nx * ny vertices, 2 (nx - 1)(ny - 1) faces"""
    gx, gy = np.meshgrid(np.linspace(-4, 4, nx), np.linspace(-3, 3, ny), indexing="ij")
    xyz = np.stack([gx + rng.normal(0, 0.01, gx.shape), gy + rng.normal(0, 0.01, gx.shape), rng.uniform(0, 3, gx.shape)], -1)
    at = np.arange(nx * ny).reshape(nx, ny)
    a, b, c, d = at[:-1, :-1], at[1:, :-1], at[:-1, 1:], at[1:, 1:]
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([b, d, c], -1).reshape(-1, 3)])
    return xyz.reshape(-1, 3).astype(np.float32), faces


def fan(rng, faces_at_hub):
    """a hub that ``faces_at_hub`` triangles share; the rim's radii are spread over three orders of magnitude, the areas over six,
    large and small mixed along the face order"""
    m = faces_at_hub + 1
    radius = 10.0 ** rng.uniform(-3, 0, m)
    angle = np.sort(rng.uniform(0, 2 * np.pi, m))
    rim = np.stack([radius * np.cos(angle), radius * np.sin(angle), radius * rng.uniform(-1, 1, m)], 1)
    xyz = np.concatenate([np.zeros((1, 3)), rim]).astype(np.float32)
    faces = np.stack([np.zeros(m - 1, np.int64), np.arange(1, m), np.arange(2, m + 1)], 1)
    return xyz, faces


def tiny(rng):
    """triangles at the origin with edges from 1e-10 down to 1e-19: the squares of the cross product run through the subnormal
    range into zero, and a product of two edges of 1e-19 is itself subnormal"""
    xyz, faces = [], []
    for edge in (1e-10, 3e-11, 1e-11, 3e-12, 1e-12, 1e-15, 1e-19, 2e-19):
        base = len(xyz)
        xyz += [rng.normal(size=3) * edge for _ in range(4)]
        faces += [(base, base + 1, base + 2), (base + 1, base + 3, base + 2)]
    return np.array(xyz).astype(np.float32), np.array(faces)


def main():
    MG.import_reference()
    import datasets.scannet as S  # noqa  (reference)
    ids = S.ScannetDatasetConfig().nyu40ids
    rng = np.random.default_rng(77)
    arrays = {}
    kw = dict(rng=rng)
    every = dict(color_drop=0.2, color_contrastp=0.2, color_jitterp=0.95, hue_sat="0.5_0.2_0.9")

    record(arrays, "single", S, rng.uniform(-1, 1, (3, 3)).astype(np.float32), [(0, 1, 2)], ids, **kw)
    xyz, faces = height_field(rng, 3, 3)
    record(arrays, "isolated", S, np.concatenate([xyz, rng.uniform(-1, 1, (4, 3)).astype(np.float32)]), faces, ids, **kw)
    xyz, faces = height_field(rng, 3, 4)
    xyz[9:12] = np.float32([1.0, 0.5, 0.25]) + np.outer([0.0, 1.0, 2.5], [0.5, 0.25, 0.125]).astype(np.float32)   # three collinear vertices, exactly so
    faces = np.concatenate([faces, [(0, 0, 5), (4, 7, 7), (6, 6, 6), (9, 10, 11), (5, 4, 4)]])
    record(arrays, "degenerate", S, xyz, faces, ids, **kw)
    record(arrays, "tiny", S, *tiny(rng), ids, **kw)
    record(arrays, "fan", S, *fan(rng, FAN_FACES + 20), ids, **kw)
    record(arrays, "grid", S, *height_field(rng, 33, 31), ids, **kw)
    record(arrays, "chain", S, *height_field(rng, 60, 50), ids, lambda t: t["contrast"] and t["jitter"] and t["hue"] and t["dropped"] > 0,
           augment=True, use_random_cuboid=True, min_points=1000, num_points=1024, use_height=True, coloraug_sunrgbd=True, **every, **kw)
    arrays["cases"] = np.array(CASES)
    MG.save("normals", **arrays)
    from test_normals_restatement import golden
    for name in CASES:
        cases_present(name, golden()[name], settings_of(golden()[name]))


if __name__ == "__main__":
    main()
