#!/usr/bin/env python3
"""Generates tests/golden/cuboid.npz from the reference's own loader (build container only, like
tools/make_scene_prep_golden.py, whose synthetic scans and import recipe it reuses).

A one-scan directory is written, ``ScannetDetectionDataset`` is constructed on it with ``use_random_cuboid=True`` and a small
``random_cuboid_min_points``, and ``__getitem__`` is called under ``np.random.seed(s)``.  Nothing of the crop or the sampling is
restated here; the reference's own calls are watched:
  * ``random_cuboid_augmentor`` is wrapped: its arguments and what it returns are recorded (the cropped cloud, the kept boxes;
    the fallback hands back the very array it was given).  While it runs, the ``np`` its module sees is a forwarding proxy
    that notes every ``np.random.rand``, every ``np.random.choice`` and every ``np.sum`` of a bool vector, so each attempt's
    fate can be read off: rand without choice = the aspect test failed; the sum is the attempt's point count;
  * ``pc_util.random_sampling`` is wrapped: its ``choices`` and the generator's state right after it are recorded.
The literal ``instance_bboxes.sum() > 0`` of the array the augmentor was given is recorded next to them.

Seeds are searched so that the file holds the cases DESIGN.md 6.4 lists; each is asserted here and again by
tests/test_cuboid_restatement.py from the recorded fields.  Inputs, recorded results and settings only.

    python tools/make_cuboid_golden.py
"""
import os
import sys
import tempfile
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_scene_prep_golden as SPG  # noqa: E402
from oracle import make_golden as MG  # noqa: E402

RATIOS = (5.0, 0.4, 0.4)   # rot, trans, scale
T = 100


class Watch:
    """stands in for ``np`` in utils/random_cuboid.py while the augmentor runs: forwards everything, notes three calls"""

    class _Random:
        def __init__(self, events):
            self._events = events

        def rand(self, *a):
            self._events.append(("rand", -1))
            return np.random.rand(*a)

        def choice(self, *a, **kw):
            self._events.append(("choice", -1))
            return np.random.choice(*a, **kw)

        def __getattr__(self, name):
            return getattr(np.random, name)

    def __init__(self):
        self.events = []
        self.random = Watch._Random(self.events)

    def sum(self, a, *args, **kw):
        r = np.sum(a, *args, **kw)
        if getattr(a, "dtype", None) == np.bool_ and a.ndim == 1 and not args and not kw:
            self.events.append(("count", int(r)))
        return r

    def __getattr__(self, name):
        return getattr(np, name)


def attempts_of(events):
    """-> (valid [t] int8, count [t] int32 with -1 where the attempt never counted) of the attempts gone through"""
    valid, count = [], []
    for what, value in events:
        if what == "rand":
            valid.append(0)
            count.append(-1)
        elif what == "choice":
            valid[-1] = 1
        else:
            count[-1] = value
    return np.array(valid, np.int8), np.array(count, np.int32)


def run_reference(S, RC, vert, box, seed, min_points, num_points):
    rot, trans, scale = RATIOS
    seen = {}
    with tempfile.TemporaryDirectory() as tmp:
        data, meta = os.path.join(tmp, "data"), os.path.join(tmp, "meta")
        os.makedirs(data)
        os.makedirs(meta)
        name = "scene0000_00"
        np.save(os.path.join(data, name + "_vert.npy"), vert)
        np.save(os.path.join(data, name + "_bbox.npy"), box)
        np.save(os.path.join(data, name + "_ins_label.npy"), np.arange(len(vert), dtype=np.int64))
        np.save(os.path.join(data, name + "_sem_label.npy"), np.zeros(len(vert), np.int64))
        with open(os.path.join(meta, "scannetv2_train.txt"), "w") as fh:
            fh.write(name + "\n")
        args = Namespace(dataset_root_dir=data, meta_data_dir=meta, num_points=num_points, use_color=False, color_mean=-1.0, rot_ratio=rot,
                         scale_ratio=scale, trans_ratio=trans, use_superpoint=False, filt_empty=False, use_normals=False, color_drop=0.0,
                         color_contrastp=0.0, color_jitterp=0.0, hue_sat="0_0_0", coloraug_sunrgbd=False)
        ds = S.ScannetDetectionDataset(S.ScannetDatasetConfig(), split_set="train", augment=True, use_random_cuboid=True,
                                       random_cuboid_min_points=min_points, args=args)
        augmentor, sampling, watch = ds.random_cuboid_augmentor, S.pc_util.random_sampling, Watch()

        def crop(cloud, boxes, labels):
            seen["cloud_in"], seen["boxes_in"] = cloud.copy(), boxes.copy()
            real_np, RC.np = RC.np, watch
            try:
                out = augmentor(cloud, boxes, labels)
            finally:
                RC.np = real_np
            seen["fallback"] = out[0] is cloud
            seen["cloud"], seen["boxes"], seen["rows"] = out[0].copy(), out[1].copy(), out[2][0].copy()   # the instance labels are the row numbers
            return out

        def sample(*a, **kw):
            out = sampling(*a, **kw)
            seen["choices"], seen["state_sampled"] = out[1].copy(), np.random.get_state()
            return out

        ds.random_cuboid_augmentor, S.pc_util.random_sampling = crop, sample
        try:
            np.random.seed(seed)
            ret = ds[0]
            seen["state"] = np.random.get_state()
        finally:
            S.pc_util.random_sampling = sampling
    seen["valid"], seen["count"] = attempts_of(watch.events)
    seen["trial"] = -1 if seen["fallback"] else len(seen["valid"]) - 1
    return ret, seen


def fates(seen, min_points):
    """what became of each attempt before the accepted one, from the recorded calls alone"""
    n = len(seen["valid"]) if seen["trial"] < 0 else seen["trial"]
    valid, count = seen["valid"][:n], seen["count"][:n]
    return {"aspect": int((valid == 0).sum()), "count": int(((valid == 1) & (count < min_points)).sum()),
            "box": int(((valid == 1) & (count >= min_points)).sum())}


def record(arrays, name, S, RC, vert, box, min_points, num_points, want, seeds=range(400)):
    for seed in seeds:
        ret, seen = run_reference(S, RC, vert, box, seed, min_points, num_points)
        if want(seen, fates(seen, min_points)):
            break
    else:
        raise AssertionError(f"{name}: no seed gives the case")
    assert np.array_equal(seen["cloud_in"], vert[:, :3]) and np.array_equal(seen["boxes_in"], box)
    assert np.array_equal(vert[seen["rows"], :3], seen["cloud"])
    a = {"points": np.ascontiguousarray(vert[:, :3]), "boxes7": box, "seed": np.array(seed), "min_points": np.array(min_points),
         "num_points": np.array(num_points), "ratios": np.array(RATIOS), "trial": np.array(seen["trial"]),
         "attempt_valid": seen["valid"], "attempt_count": seen["count"], "crop_points": seen["cloud"], "crop_rows": seen["rows"],
         "crop_boxes7": seen["boxes"], "choices": seen["choices"].astype(np.int64), "literal_filter": np.array(bool(box.sum() > 0)),
         "state_sampled_keys": seen["state_sampled"][1], "state_sampled_pos": np.array(seen["state_sampled"][2]),
         "state_keys": seen["state"][1], "state_pos": np.array(seen["state"][2]), "out_points": ret["point_clouds"].numpy()}
    for k in SPG.OUT_KEYS:
        a[k] = np.asarray(ret[k])
    for k, v in a.items():
        arrays[f"{name}:{k}"] = v
    print(f"{name}: seed {seed}, trial {seen['trial']}, before it {fates(seen, min_points)}, kept {len(seen['cloud'])} of {len(vert)} rows, "
          f"{len(seen['boxes'])} of {len(box)} boxes")
    return seen


def main():
    MG.import_reference()
    import datasets.scannet as S  # noqa  (reference)
    import utils.random_cuboid as RC  # noqa  (reference)
    ids = S.ScannetDatasetConfig().nyu40ids
    rng = np.random.default_rng(65)
    arrays = {}
    accepted = lambda s, f: s["trial"] >= 0  # noqa: E731

    v, b = SPG.scan(rng, 5000, 5, ids)
    s = record(arrays, "late", S, RC, v, b, 2000, 1024, lambda s, f: s["trial"] > 0 and f["aspect"] and f["count"] and len(s["boxes"]) < 5)
    assert len(s["cloud"]) > 1024 and len(v) // 256 >= 19              # sampled without replacement; about 20 tiles
    v, b = SPG.scan(rng, 1000, 1, ids)
    record(arrays, "nobox", S, RC, v, b, 200, 512, lambda s, f: s["trial"] > 0 and f["box"])
    v, b = SPG.scan(rng, 300, 3, ids)
    s = record(arrays, "fallback", S, RC, v, b, 301, 512, lambda s, f: True)
    assert s["trial"] == -1 and len(s["valid"]) == T and len(s["cloud"]) == 300 and len(s["boxes"]) == 3
    v, b = SPG.scan(rng, 400, 0, ids)
    s = record(arrays, "empty", S, RC, v, b, 100, 512, accepted)
    assert b.shape == (0, 7) and s["boxes"].shape == (0, 7)
    v, b = SPG.scan(rng, 500, 6, ids)
    b[:, :6] = rng.uniform([-4, -3, 0, 0.2, 0.2, 0.2], [4, 3, 3, 2, 2, 2], (6, 6))                # genuine float64 values
    assert (b[:, :6].astype(np.float32).astype(np.float64) != b[:, :6]).all()
    record(arrays, "f64", S, RC, v, b, 150, 256, lambda s, f: s["trial"] >= 0 and 0 < len(s["boxes"]) < 6 and len(s["cloud"]) > 256)
    for n in (255, 256, 257):
        v, b = SPG.scan(rng, n, 4, ids)
        s = record(arrays, f"n{n}", S, RC, v, b, 60, 512, lambda s, f: s["trial"] >= 0 and 0 < len(s["boxes"]) < 4)
        assert len(s["cloud"]) < 512                                   # sampled with replacement
    arrays["cases"] = np.array(["late", "nobox", "fallback", "empty", "f64", "n255", "n256", "n257"])
    MG.save("cuboid", **arrays)


if __name__ == "__main__":
    main()
