#!/usr/bin/env python3
"""Generates tests/golden/color_aug.npz from the reference's own loader (build container only, like
tools/make_cuboid_golden.py, whose import recipe and synthetic scans it reuses).

A one-scan directory is written, ``ScannetDetectionDataset`` is constructed on it with ``use_color=True`` and the case's
settings, and ``__getitem__`` is called under ``np.random.seed(s)``.  It wraps; it does not restate: the file holds the
inputs, the settings, the seed, the returned ``point_clouds`` and the generator's state after the call.  The colour cases run
with ``use_random_cuboid=False``, so that the final cloud carries every input row's colour; ``chain`` runs the crop too.

Seeds and inputs are searched so that the file holds the cases DESIGN.md 6.5 lists.  Which gate fired is read off the
reference's own stream: ``scene_prep.draw_color_augment`` replays it from the seed, and tests/color_aug_restatement.py must
then end in the recorded state with the recorded cloud, which is asserted here and again by
tests/test_color_aug_restatement.py (``cases_present``).

    python tools/make_color_aug_golden.py
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
from test_color_aug_restatement import CASES, cases_present, settings_of  # noqa: E402


def run_reference(S, vert, box, seed, s):
    rot, trans, scale = s["ratios"]
    with tempfile.TemporaryDirectory() as tmp:
        data, meta = os.path.join(tmp, "data"), os.path.join(tmp, "meta")
        os.makedirs(data)
        os.makedirs(meta)
        name = "scene0000_00"
        np.save(os.path.join(data, name + "_vert.npy"), vert)
        np.save(os.path.join(data, name + "_bbox.npy"), box)
        np.save(os.path.join(data, name + "_ins_label.npy"), np.zeros(len(vert), np.int64))
        np.save(os.path.join(data, name + "_sem_label.npy"), np.zeros(len(vert), np.int64))
        with open(os.path.join(meta, "scannetv2_train.txt"), "w") as fh:
            fh.write(name + "\n")
        args = Namespace(dataset_root_dir=data, meta_data_dir=meta, num_points=int(s["num_points"]), use_color=True,
                         color_mean=float(s["color_mean"]), rot_ratio=rot, scale_ratio=scale, trans_ratio=trans, use_superpoint=False,
                         filt_empty=False, use_normals=False, color_drop=float(s["color_drop"]), color_contrastp=float(s["color_contrastp"]),
                         color_jitterp=float(s["color_jitterp"]), hue_sat=str(s["hue_sat"]), coloraug_sunrgbd=bool(s["coloraug_sunrgbd"]))
        ds = S.ScannetDetectionDataset(S.ScannetDatasetConfig(), split_set="train", use_height=bool(s["use_height"]), augment=True,
                                       use_random_cuboid=bool(s["use_random_cuboid"]), random_cuboid_min_points=int(s["min_points"]),
                                       args=args)
        np.random.seed(seed)
        with np.errstate(all="ignore"):
            ret = ds[0]
        return ret["point_clouds"].numpy(), np.random.get_state()


def record(arrays, name, S, vert, box, want, seeds=range(400), **settings):
    s = dict(CA.SETTINGS, **settings)
    for seed in seeds:
        out, state = run_reference(S, vert, box, seed, s)
        mine, seen = CA.loader_scene(vert, box, np.random.RandomState(seed), s)
        if want(seen):
            break
    else:
        raise AssertionError(f"{name}: no seed gives the case")
    assert mine.tobytes() == out.tobytes(), name
    a = {"vert": vert, "boxes7": box, "seed": np.array(seed), "out_points": out, "state_keys": state[1], "state_pos": np.array(state[2])}
    for k, v in s.items():
        a[f"set_{k}"] = np.array(v)
    for k, v in a.items():
        arrays[f"{name}:{k}"] = v
    print(f"{name}: seed {seed}, {len(vert)} rows -> {out.shape}, saw {seen}")


def colours(rng, n):
    """integer colours 0 .. 255 with the ends present, one grey row and one row per hue sextant"""
    rgb = rng.integers(0, 256, (n, 3)).astype(np.float32)
    fixed = [(0, 0, 0), (255, 255, 255), (128, 128, 128), (250, 40, 10), (200, 240, 10), (10, 240, 90), (10, 200, 240), (60, 10, 240), (240, 10, 200)]
    rgb[:min(n, len(fixed))] = fixed[:n]
    return rgb


def scan(rng, n, nbox, ids):
    v, b = SPG.scan(rng, n, nbox, ids, colours=True)
    v[:, 3:6] = colours(rng, n)
    return v, b


def main():
    MG.import_reference()
    import datasets.scannet as S  # noqa  (reference)
    ids = S.ScannetDatasetConfig().nyu40ids
    rng = np.random.default_rng(66)
    arrays = {}
    every = dict(color_drop=0.2, color_contrastp=0.2, color_jitterp=0.95, hue_sat="0.5_0.2_0.9")

    record(arrays, "drop", S, *scan(rng, 255, 3, ids), lambda t: t["dropped"] > 0, color_drop=0.2)
    record(arrays, "contrast", S, *scan(rng, 256, 3, ids), lambda t: t["contrast"], color_contrastp=0.2, color_mean=0.5)
    record(arrays, "contrast_off", S, *scan(rng, 70, 2, ids), lambda t: not t["contrast"], color_contrastp=0.2)
    record(arrays, "jitter", S, *scan(rng, 257, 3, ids), lambda t: t["jitter"] and t["clipped_low"] and t["clipped_high"], color_jitterp=0.95)
    record(arrays, "jitter_off", S, *scan(rng, 70, 2, ids), lambda t: not t["jitter"], color_jitterp=0.95)
    record(arrays, "hue", S, *scan(rng, 300, 3, ids), lambda t: t["hue"] and t["sextants"] == [0, 1, 2, 3, 4, 5] and t["grey"] and t["wrapped"],
           hue_sat="0.5_0.2_0.9", color_mean=0.5)
    record(arrays, "hue_off", S, *scan(rng, 70, 2, ids), lambda t: not t["hue"], hue_sat="0.5_0.2_0.1")
    record(arrays, "all", S, *scan(rng, 2500, 5, ids),
           lambda t: t["dropped"] and t["contrast"] and t["jitter"] and t["hue"] and len(t["sextants"]) == 6 and t["grey"], **every)
    v, b = scan(rng, 64, 2, ids)
    v[:, 5] = 0                                                        # a channel that is constant after the drop: 255 / 0
    record(arrays, "nan", S, v, b, lambda t: t["contrast"] and t["nan_channels"] == 1 and t["jitter"] and t["dropped"], color_drop=0.2,
           color_contrastp=1.0, color_jitterp=0.95)
    record(arrays, "sunrgbd", S, *scan(rng, 257, 3, ids), lambda t: True, coloraug_sunrgbd=True, color_mean=0.5)
    record(arrays, "all_sunrgbd", S, *scan(rng, 300, 3, ids), lambda t: t["contrast"] and t["jitter"] and t["hue"], coloraug_sunrgbd=True,
           **every)
    for n in (1, 2, 101, 257):
        record(arrays, f"height{n}", S, *scan(rng, n, 2, ids), lambda t: True, use_height=True, color_mean=0.5)
    record(arrays, "chain", S, *scan(rng, 3000, 5, ids), lambda t: t["contrast"] and t["jitter"] and t["hue"], use_random_cuboid=True,
           min_points=1000, num_points=1024, use_height=True, coloraug_sunrgbd=True, **every)
    arrays["cases"] = np.array(CASES)
    MG.save("color_aug", **arrays)
    from test_color_aug_restatement import golden
    for name in CASES:
        cases_present(name, golden()[name], settings_of(golden()[name]))


if __name__ == "__main__":
    main()
