"""numpy restatement of the reference's scan export on parsed arrays (scannet/load_scannet_data.py:26-129 ``read_aggregation``,
``read_segmentation``, ``export``; scannet/batch_load_scannet_data.py:25-50 ``export_one_scan``), vectorised over the vertices,
for generated inputs.  tests/test_scan_export_restatement.py holds it against the fixture that the reference itself produced
(tests/golden/scan_export.npz).  It works per vertex, where v-detr_amd/scan_export.py:scan_tables works per segment: the two
share nothing but the walk over the groups.

The alignment is stated, not delegated to BLAS: ``((x*m[r][0] + y*m[r][1]) + z*m[r][2]) + m[r][3]`` in float64, one rounding to
float32.  ``np.dot`` may add in another order or fuse; the fixture only holds inputs on which its float32 result equals this
evaluation and the fused one (``align_fused``), so the reference itself is unambiguous there.
"""
from fractions import Fraction

import numpy as np

OBJ_CLASS_IDS = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)


def align(xyz, matrix):
    """float32 [n,3] -> float32 [n,3]: every product and sum one float64 operation, left to right"""
    m = np.asarray(matrix, np.float64).reshape(4, 4)
    x, y, z = (np.asarray(xyz[:, c], np.float64) for c in range(3))
    return np.stack([(((x * m[r, 0]) + (y * m[r, 1])) + (z * m[r, 2])) + m[r, 3] for r in range(3)], 1).astype(np.float32)


def align_fused(xyz, matrix):
    """the same with fused multiply-adds, fma(z, m2, fma(y, m1, x * m0)) + m3, exact rationals rounded once per step (slow: the
    fixture's few thousand vertices only)"""
    m = np.asarray(matrix, np.float64).reshape(4, 4)
    out = np.empty((len(xyz), 3), np.float64)
    for i, p in enumerate(np.asarray(xyz, np.float64)[:, :3]):
        for r in range(3):
            t = p[0] * m[r, 0]
            t = float(Fraction(p[1]) * Fraction(m[r, 1]) + Fraction(t))
            t = float(Fraction(p[2]) * Fraction(m[r, 2]) + Fraction(t))
            out[i, r] = t + m[r, 3]
    return out.astype(np.float32)


def walk_groups(seg_groups):
    """read_aggregation on the parsed ``segGroups``: {object id: segments}, {label: segments}; the label's list is its first
    object's own list, which later objects of the label extend (:37-41)"""
    object_segs, label_segs = {}, {}
    for g in seg_groups:
        segs = list(g["segments"])
        object_segs[int(g["objectId"]) + 1] = segs
        if g["label"] in label_segs:
            label_segs[g["label"]].extend(segs)
        else:
            label_segs[g["label"]] = segs
    return object_segs, label_segs


def export(mesh_vertices, seg_indices, seg_groups, label_map, axis_align):
    """-> mesh_vertices float32 [n,W], label_ids uint32 [n], instance_ids uint32 [n], instance_bboxes float64 [K,7],
    object_label {object id: label id}; ``axis_align``: 16 numbers"""
    mesh = np.array(mesh_vertices, np.float32)
    mesh[:, :3] = align(mesh, axis_align)
    seg = np.asarray(seg_indices, np.int64)
    n = len(seg)
    carried = set(np.unique(seg).tolist())
    object_segs, label_segs = walk_groups(seg_groups)
    label_ids = np.zeros(n, np.uint32)
    for label, segs in label_segs.items():
        label_id = label_map[label]
        for s in segs:
            if s not in carried:
                raise KeyError(s)
        label_ids[np.isin(seg, segs)] = label_id
    instance_ids = np.zeros(n, np.uint32)
    num_instances = len(object_segs)
    object_label = {}
    for object_id, segs in object_segs.items():
        for s in segs:
            if s not in carried:
                raise KeyError(s)
        instance_ids[np.isin(seg, segs)] = object_id
        if segs:
            object_label[object_id] = label_ids[np.argmax(seg == segs[0])]
    boxes = np.zeros((num_instances, 7))
    order = np.argsort(instance_ids, kind="stable")
    ids, starts = np.unique(instance_ids[order], return_index=True)
    if n:
        lo, hi = np.minimum.reduceat(mesh[order, :3], starts), np.maximum.reduceat(mesh[order, :3], starts)
    for i, object_id in enumerate(ids.tolist()):
        if object_id == 0:
            continue
        if not 1 <= object_id <= num_instances:
            raise IndexError(object_id)
        boxes[object_id - 1, :3] = (lo[i] + hi[i]) / np.float32(2)          # float32 arithmetic, widened by the table
        boxes[object_id - 1, 3:6] = hi[i] - lo[i]
        boxes[object_id - 1, 6] = object_label[object_id]
    for object_id in object_segs:
        if object_id not in object_label:
            raise KeyError(object_id)
        if not 1 <= object_id <= num_instances:
            raise IndexError(object_id)
    return mesh, label_ids, instance_ids, boxes, object_label


def export_one_scan(mesh_vertices, seg_indices, seg_groups, label_map, axis_align, donotcare_ids=(), obj_class_ids=OBJ_CLASS_IDS):
    """-> the four saved arrays: _vert float32 [n',W], _sem_label uint32 [n'], _ins_label uint32 [n'], _bbox float64 [G,7]"""
    mesh, sem, ins, boxes, _ = export(mesh_vertices, seg_indices, seg_groups, label_map, axis_align)
    mask = ~np.isin(sem, np.asarray(donotcare_ids))
    return mesh[mask], sem[mask], ins[mask], boxes[np.isin(boxes[:, -1], np.asarray(obj_class_ids))]


def batch_tensors(scans, nyu40id2class, Kmax=None):
    """what ``export_scans`` returns for a batch, from ``export`` / ``export_one_scan`` results: scans = [(export's five,
    export_one_scan's four)] -> dict of host arrays"""
    Kmax = max(len(full[3]) for full, _ in scans) if Kmax is None else Kmax
    B = len(scans)
    out = {"mesh_vertices": np.concatenate([one[0] for _, one in scans]),
           "offsets": np.cumsum([0] + [len(one[0]) for _, one in scans]),
           "semantic_labels": np.concatenate([one[1] for _, one in scans]).astype(np.int32),
           "instance_labels": np.concatenate([one[2] for _, one in scans]).astype(np.int32),
           "instance_bboxes": np.zeros((B, Kmax, 7), np.float32), "boxes": np.zeros((B, Kmax, 6), np.float32),
           "box_nyu40": np.zeros((B, Kmax), np.int64), "box_classes": np.zeros((B, Kmax), np.int64), "box_counts": np.zeros(B, np.int64)}
    for b, (full, one) in enumerate(scans):
        kept = one[3]
        out["instance_bboxes"][b, :len(full[3])] = full[3]
        out["boxes"][b, :len(kept)] = kept[:, :6]
        out["box_nyu40"][b, :len(kept)] = kept[:, 6]
        out["box_classes"][b, :len(kept)] = [nyu40id2class[int(v)] for v in kept[:, 6]]
        out["box_counts"][b] = len(kept)
    return out
