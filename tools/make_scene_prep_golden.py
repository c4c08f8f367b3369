#!/usr/bin/env python3
"""Generates tests/golden/scene_prep.npz from the reference's own loader (build container only, like oracle/make_golden.py,
whose import recipe it reuses).

Which of the two ways: the FIRST.  A tiny synthetic scan directory (the four ``.npy`` files per scan and the split list) is
written to a temporary directory, ``ScannetDetectionDataset`` is constructed on it with ``use_random_cuboid=False`` and its
``__getitem__`` is called scene after scene under ``np.random.seed(s)``; nothing of scannet.py:510-626 is restated here.  Two
things are added around the calls:
  * ``np.random.random`` is wrapped while the reference runs, so that the raw draws are seen; the recorded parameters are those
    draws put through the expressions of scannet.py:516-540, and the generator's state after the batch is recorded too;
  * ``__getitem__`` samples only after RandomCuboid (whose attempt loop is out of scope), so for the ``choices``
    case the indices are drawn here as pc_util.random_sampling draws them (``np.random.choice`` with replacement) and the
    reference is given the gathered scan: every step it takes is per point, so that is ``pc[choices]`` taken first.
The file holds inputs, drawn parameters and outputs only.

    python tools/make_scene_prep_golden.py
"""
import os
import sys
import tempfile
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as MG  # noqa: E402

OUT_KEYS = ("gt_box_corners", "gt_box_centers", "gt_box_centers_normalized", "gt_angle_class_label", "gt_angle_residual_label",
            "gt_box_sem_cls_label", "gt_box_present", "gt_box_sizes", "gt_box_sizes_normalized", "gt_box_sizes_residual_label",
            "gt_box_angles", "point_cloud_dims_min", "point_cloud_dims_max")
G = 64


def scan(rng, n, nbox, ids, colours=False, axis_point=False):
    """a cloud in a 8 x 6 x 3 m room around the origin and nbox boxes in it, as the prepared ScanNet files hold them"""
    xyz = rng.uniform([-4, -3, 0], [4, 3, 3], (n, 3))
    if axis_point:
        xyz[0] = (0.0, 0.0, 1.25)                                      # on the z axis: x = y = 0 after any rotation
    cols = [xyz] + ([rng.integers(0, 256, (n, 3)).astype(np.float64)] if colours else [])
    vert = np.concatenate(cols, 1).astype(np.float32)
    box = np.concatenate([rng.uniform([-4, -3, 0], [4, 3, 3], (nbox, 3)), rng.uniform(0.2, 2.0, (nbox, 3)),
                          rng.choice(ids, (nbox, 1)).astype(np.float64)], 1).astype(np.float32).astype(np.float64)
    return vert, box


def run_reference(S, scans, augment, seed, use_color=False, color_mean=-1.0, rot=5.0, trans=0.0, scale=0.0):
    """-> (list of the reference's ret dicts, raw np.random.random draws per scene, generator state after the batch)"""
    with tempfile.TemporaryDirectory() as tmp:
        data, meta = os.path.join(tmp, "data"), os.path.join(tmp, "meta")
        os.makedirs(data)
        os.makedirs(meta)
        names = [f"scene{i:04d}_00" for i in range(len(scans))]
        for name, (vert, box) in zip(names, scans):
            n = len(vert)
            np.save(os.path.join(data, name + "_vert.npy"), vert)
            np.save(os.path.join(data, name + "_bbox.npy"), box)
            np.save(os.path.join(data, name + "_ins_label.npy"), np.zeros(n, np.int64))
            np.save(os.path.join(data, name + "_sem_label.npy"), np.zeros(n, np.int64))
        split = "train" if augment else "val"
        with open(os.path.join(meta, f"scannetv2_{split}.txt"), "w") as fh:
            fh.write("\n".join(names) + "\n")
        args = Namespace(dataset_root_dir=data, meta_data_dir=meta, num_points=40000, use_color=use_color, color_mean=color_mean,
                         rot_ratio=rot, scale_ratio=scale, trans_ratio=trans, use_superpoint=False, filt_empty=False,
                         use_normals=False, color_drop=0.0, color_contrastp=0.0, color_jitterp=0.0, hue_sat="0_0_0",
                         coloraug_sunrgbd=False)
        ds = S.ScannetDetectionDataset(S.ScannetDatasetConfig(), split_set=split, augment=augment, use_random_cuboid=False, args=args)
        assert ds.scan_names == names
        real, draws = np.random.random, []

        def seen(*a, **kw):
            v = real(*a, **kw)
            draws[-1].append(np.array(v, np.float64))
            return v

        np.random.seed(seed)
        np.random.random = seen
        try:
            rets = []
            for i in range(len(names)):
                draws.append([])
                rets.append(ds[i])
        finally:
            np.random.random = real
        state = np.random.get_state()
    return rets, draws, state


def params_from_draws(draws, rot, trans, scale):
    """the expressions of scannet.py:516-540 on the raw draws (none for the evaluation split)"""
    B = len(draws)
    p = dict(flip_x=np.zeros(B, bool), flip_y=np.zeros(B, bool), rot_angle=np.zeros(B), trans=np.zeros((B, 3)), scale=np.ones(B))
    for b, d in enumerate(draws):
        if not d:
            continue
        d = list(d)
        p["flip_x"][b] = d.pop(0) > 0.5
        p["flip_y"][b] = d.pop(0) > 0.5
        p["rot_angle"][b] = ((d.pop(0) * np.pi / 18) - np.pi / 36) * rot / 5.0
        if trans > 0.0:
            p["trans"][b] = (d.pop(0) - 0.5) * trans / 0.5
        if scale > 0.0:
            p["scale"][b] = 1 + (d.pop(0) - 0.5) * scale / 0.5
        assert not d
    return p


def record(arrays, name, S, scans, inputs, augment, seed, choices=None, **kw):
    """inputs: the scans as prepare_scenes is given them (before any gather)"""
    rets, draws, state = run_reference(S, scans, augment, seed, **kw)
    ratios = [kw.get("rot", 5.0), kw.get("trans", 0.0), kw.get("scale", 0.0)]
    cfg = S.ScannetDatasetConfig()
    B = len(scans)
    a = {"points": np.concatenate([v for v, _ in inputs]), "offsets": np.cumsum([0] + [len(v) for v, _ in inputs]).astype(np.int32),
         "boxes": np.zeros((B, G, 6), np.float32), "box_counts": np.array([len(b) for _, b in inputs], np.int64),
         "box_nyu40": np.zeros((B, G), np.int64), "box_classes": np.zeros((B, G), np.int64), "augment": np.array(augment),
         "seed": np.array(seed), "ratios": np.array(ratios), "state_keys": state[1], "state_pos": np.array(state[2]),
         "use_color": np.array(kw.get("use_color", False)), "color_mean": np.array(kw.get("color_mean", -1.0))}
    for b, (_, box) in enumerate(inputs):
        a["boxes"][b, :len(box)] = box[:, :6]
        a["box_nyu40"][b, :len(box)] = box[:, 6]
        a["box_classes"][b, :len(box)] = [cfg.nyu40id2class[int(x)] for x in box[:, 6]]
    if not kw.get("use_color", False):
        a["points"] = np.ascontiguousarray(a["points"][:, :3])
    if choices is not None:
        a["choices"] = choices
    a.update(params_from_draws(draws, *ratios))
    a["out_points"] = np.concatenate([r["point_clouds"].numpy() for r in rets])
    a["out_offsets"] = np.cumsum([0] + [len(r["point_clouds"]) for r in rets]).astype(np.int32)
    for k in OUT_KEYS:
        a[k] = np.stack([np.asarray(r[k]) for r in rets])
    for k, v in a.items():
        arrays[f"{name}:{k}"] = v
    print(name, "draws per scene", [len(d) for d in draws], "angles", a["rot_angle"], "flips", a["flip_x"], a["flip_y"])


def main():
    MG.import_reference()
    import datasets.scannet as S  # noqa  (reference)
    ids = S.ScannetDatasetConfig().nyu40ids
    rng = np.random.default_rng(64)
    arrays = {"mean_size_arr": S.ScannetDatasetConfig().mean_size_arr}
    base = [scan(rng, 1, 0, ids), scan(rng, 257, 64, ids, axis_point=True), scan(rng, 5000, 5, ids)]
    with np.errstate(all="ignore"):                                    # the one-point scene has no extent
        record(arrays, "aug", S, base, base, True, 11, trans=0.4, scale=0.4)
        record(arrays, "aug_noratio", S, base, base, True, 11)
        record(arrays, "eval", S, base, base, False, 11)
        raw = [scan(rng, 100, 3, ids), scan(rng, 300, 7, ids)]
        np.random.seed(5)
        choices = np.stack([np.random.choice(len(v), 256, replace=len(v) < 256) for v, _ in raw])
        assert len(np.unique(choices[0])) < 100 < 256
        gathered = [(v[c], b) for (v, b), c in zip(raw, choices)]
        record(arrays, "choices", S, gathered, raw, True, 12, choices=choices, trans=0.4, scale=0.4)
        col = [scan(rng, 70, 4, ids, colours=True), scan(rng, 300, 9, ids, colours=True)]
        record(arrays, "color_mean", S, col, col, True, 13, use_color=True, color_mean=-1.0, trans=0.4, scale=0.4)
        record(arrays, "color_unit", S, col, col, True, 13, use_color=True, color_mean=0.5, trans=0.4, scale=0.4)
    arrays["cases"] = np.array(["aug", "aug_noratio", "eval", "choices", "color_mean", "color_unit"])
    MG.save("scene_prep", **arrays)


if __name__ == "__main__":
    main()
