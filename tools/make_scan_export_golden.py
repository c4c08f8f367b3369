#!/usr/bin/env python3
"""Generates tests/golden/scan_export.npz from the reference's own exporter (build container only, like
tools/make_normals_golden.py).

It wraps; it does not restate.  The reference imports a module ``scannet_utils`` that it does not ship: a stub goes into
``sys.modules`` whose ``read_mesh_vertices_rgb`` returns the case's float32 [n,6] array (as upstream's does from the ``.ply``) and
whose ``read_label_mapping`` returns the case's dict.  The case's aggregation and segmentation go into a temporary directory
as the JSON files the reference parses, the matrix as the ``axisAlignment`` line of the meta file; then
``load_scannet_data.export`` and ``batch_load_scannet_data.export_one_scan`` run there (the latter opens
``meta_data/scannet_train.txt`` relative to the working directory when it is imported, and reads ``DONOTCARE_CLASS_IDS`` from its
globals).  The file holds the inputs, the settings and every returned / saved array.

The fixture rule: a case is only kept if the reference's float32 vertices equal the stated left-to-right float64 evaluation
AND its fused variant (tests/scan_export_restatement.py ``align`` / ``align_fused``) -- BLAS is free to add in another order, and
on such inputs the reference itself is unambiguous -- and if it holds what tests/test_scan_export_restatement.py
(``cases_present``) says the case is for; otherwise the next seed is drawn.

    python tools/make_scan_export_golden.py
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import make_golden as MG  # noqa: E402
from test_scan_export_restatement import CASES, cases_present, inputs_of, make_scan, pack_inputs  # noqa: E402
import scan_export_restatement as SR  # noqa: E402

SCAN = "scene0000_00"
_modules = {}


def reference_modules(tmp):
    """the reference's two modules, imported once with the working directory where their import-time file lies"""
    if not _modules:
        sys.dont_write_bytecode = True
        stub = types.ModuleType("scannet_utils")
        stub.read_mesh_vertices_rgb = stub.read_label_mapping = None
        sys.modules["scannet_utils"] = stub
        sys.path.insert(0, os.path.join(MG.REF, "scannet"))
        import batch_load_scannet_data as BL  # noqa  (reference)
        import load_scannet_data as LS  # noqa  (reference)
        _modules.update(stub=stub, LS=LS, BL=BL)
    return _modules["stub"], _modules["LS"], _modules["BL"]


def run_reference(scan, donotcare):
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "meta_data"))
        with open(os.path.join(tmp, "meta_data", "scannet_train.txt"), "w") as fh:
            fh.write(SCAN + "\n")
        os.chdir(tmp)
        try:
            stub, LS, BL = reference_modules(tmp)
            folder = os.path.join(BL.SCANNET_DIR, SCAN)
            os.makedirs(folder)
            with open(os.path.join(folder, SCAN + ".aggregation.json"), "w") as fh:
                json.dump({"segGroups": scan["groups"]}, fh)
            with open(os.path.join(folder, SCAN + "_vh_clean_2.0.010000.segs.json"), "w") as fh:
                json.dump({"segIndices": [int(s) for s in scan["seg_indices"]]}, fh)
            with open(os.path.join(folder, SCAN + ".txt"), "w") as fh:
                fh.write("axisAlignment = " + " ".join(repr(float(v)) for v in scan["axis_align"]) + "\nnumDepthFrames = 1\n")
            stub.read_mesh_vertices_rgb = lambda path: scan["mesh"].copy()
            stub.read_label_mapping = lambda path, label_from, label_to: dict(scan["label_map"])
            files = [os.path.join(folder, SCAN + end) for end in ("_vh_clean_2.ply", ".aggregation.json", "_vh_clean_2.0.010000.segs.json", ".txt")]
            mesh, labels, instances, boxes, object_label = LS.export(*files, BL.LABEL_MAP_FILE)
            BL.DONOTCARE_CLASS_IDS = np.array(donotcare)
            BL.export_one_scan(SCAN, "out")
            saved = {k: np.load(f"out_{k}.npy") for k in ("vert", "sem_label", "ins_label", "bbox")}
        finally:
            os.chdir(cwd)
    ids = sorted(object_label)
    return dict(saved, ex_vertices=mesh, ex_labels=labels, ex_instances=instances, ex_bboxes=boxes, ex_object_ids=np.array(ids, np.int64),
                ex_object_labels=np.array([int(object_label[k]) for k in ids], np.int64))


def record(arrays, name, build, donotcare=(), seeds=range(400)):
    at = CASES.index(name)
    for seed in seeds:
        scan = build(np.random.default_rng([at, seed]))
        case = dict(pack_inputs(scan, donotcare), **run_reference(scan, donotcare))
        try:
            cases_present(name, case)
        except AssertionError:
            continue
        break
    else:
        raise AssertionError(f"{name}: no seed gives the case")
    for k, v in case.items():
        arrays[f"{name}:{k}"] = v
    print(f"{name}: seed {seed}, {len(scan['mesh'])} vertices, {len(scan['groups'])} groups -> {case['ex_bboxes'].shape[0]} objects, "
          f"{case['bbox'].shape[0]} kept, {len(case['vert'])} rows")


def everywhere(rng, n, tile):
    """objectId 0, written last, also owns the first and the last vertex's segment: it has vertices in every tile"""
    s = make_scan(rng, n, 6)
    own = next(g for g in s["groups"] if g["objectId"] == 0)
    s["groups"].remove(own)
    own["segments"] = own["segments"] + [x for x in (s["seg_indices"][0], s["seg_indices"][-1]) if x not in own["segments"]]
    s["groups"].append(own)
    return s


def shared_seg(rng):
    """ten segments of four vertices; see the group list: a label's first object without segments of its own (the alias gives it
    the next chair's), segment 12 under two labels, segment 15 under two objects of one label, objectId 1 named twice"""
    s = make_scan(rng, 40, 0)
    s["seg_indices"] = np.repeat(np.arange(11, 21), 4).tolist()
    group = lambda i, label, segs: {"objectId": i, "label": label, "segments": segs}  # noqa: E731
    s["groups"] = [group(0, "chair", []), group(1, "chair", [11, 12]), group(2, "table", [12, 13]), group(3, "office chair", [14, 15]),
                   group(4, "office chair", [15, 16]), group(1, "desk", [17])]
    return s


def empty_object(rng):
    """all 18 kept classes, six others, and an object whose only segments a later object takes: its row stays zero"""
    kept = ["cabinet", "bed", "chair", "couch", "table", "door", "window", "bookshelf", "picture", "counter", "desk", "curtain",
            "refrigerator", "shower curtain", "toilet", "sink", "bathtub", "trash can"]
    other = ["wall", "floor", "blinds", "box", "lamp", "mirror"]
    names = [x for pair in zip(kept[:6], other) for x in pair] + kept[6:] + ["armchair", "door"]
    s = make_scan(rng, 700, len(names))
    for g in s["groups"]:
        g["label"] = names[g["objectId"]]
    lost = next(g for g in s["groups"] if g["objectId"] == len(names) - 2)
    taker = next(g for g in s["groups"] if g["objectId"] == len(names) - 1)
    s["groups"].remove(lost)
    s["groups"].remove(taker)
    taker["segments"] = taker["segments"] + lost["segments"]
    s["groups"] = [lost] + s["groups"] + [taker]
    return s


def negative(rng):
    s = make_scan(rng, 90, 3, translation=(1e3, -1e3, 1e3), centres=[(-3, -2, -1.5), (0, 0, 0), (3, 2, 1.5)])
    return s


def with_labels(rng, n, K, names, **kw):
    s = make_scan(rng, n, K, **kw)
    for g in s["groups"]:
        g["label"] = names[g["objectId"] % len(names)]
    return s


def identity(rng):
    s = make_scan(rng, 300, 4)
    s["axis_align"] = np.eye(4).reshape(16).tolist()
    return s


def main():
    from vdetr_amd import _lib
    tile = _lib.VDETR_EXPORT_TILE
    arrays = {}
    record(arrays, "single", lambda rng: make_scan(rng, 1, 1))
    record(arrays, "edge_m1", lambda rng: everywhere(rng, tile - 1, tile))
    record(arrays, "edge", lambda rng: everywhere(rng, tile, tile))
    record(arrays, "edge_p1", lambda rng: everywhere(rng, tile + 1, tile))
    record(arrays, "negative", negative)
    record(arrays, "shared_seg", shared_seg)
    record(arrays, "empty_object", empty_object)
    record(arrays, "unannotated", lambda rng: make_scan(rng, 600, 5, cover=0.33))
    record(arrays, "donotcare", lambda rng: with_labels(rng, 500, 8, ["wall", "chair", "floor", "table", "desk", "lamp", "floor", "bed"], cover=0.8),
           donotcare=(1, 2))
    record(arrays, "identity", identity)
    arrays["cases"] = np.array(CASES)
    MG.save("scan_export", **arrays)
    from test_scan_export_restatement import golden
    for name in CASES:                                                 # the file as the tests will read it
        c = golden()[name]
        cases_present(name, c)
        got = SR.export(*inputs_of(c))
        assert all(a.tobytes() == c[k].tobytes() for a, k in zip(got[:4], ("ex_vertices", "ex_labels", "ex_instances", "ex_bboxes"))), name

if __name__ == "__main__":
    main()
