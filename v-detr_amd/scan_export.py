"""A raw ScanNet scan -> the arrays of its ``_vert`` / ``_sem_label`` / ``_ins_label`` / ``_bbox`` files, on the device (DESIGN.md
6.7; reference scannet/load_scannet_data.py:60-129 ``export`` and scannet/batch_load_scannet_data.py:25-50 ``export_one_scan``).

This is the step in front of ``scene_prep``: the mesh vertices, the over-segmentation (``segIndices``), the aggregation
(``segGroups``), the label map and the ``axisAlignment`` matrix become the aligned cloud, the per-vertex labels and the boxes
that ``crop_and_sample`` and ``prepare_scenes`` take.  ``scan_tables`` is the host half: it walks the groups in the reference's
order, with the reference's list aliasing, and leaves two per-segment tables, so that a segment named by several groups gets
what the reference's loops leave there.  ``export_scans`` is the device half (csrc/scan_export.hip): the float64 alignment
rounded once to float32, the label gathers, one [K, 6] min / max table per tile in LDS, the merge, the class filter and the
compaction, in two launches on the current stream without a synchronisation (three launches and one read-back of a count per
scene when ``donotcare_ids`` removes vertices).  Everything equals the reference bit for bit.  No file is opened here: the
caller parses the ``.ply`` / ``.json`` / ``.tsv`` / ``.txt`` files.  No CPU path.
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from .scene_prep import _packed_scenes, _upload_offsets

OBJ_CLASS_IDS = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)   # batch_load_scannet_data.py:22
MAX_LABEL = 2 ** 24   # labels travel as float32 in column 6 of instance_bboxes, exactly


@dataclass
class ScanTables:
    """One scan's tables, host arrays: ``seg_indices`` int32 [n]: per vertex the row of its segment in the two segment tables
    (the raw ids, ascending, are ``seg_ids`` [S]); ``seg_label`` int32 [S] the nyu40 id, 0 if no group names the segment;
    ``seg_object`` int32 [S] the 1-based object id, 0 if none; ``num_instances`` K; ``object_label`` int32 [K]
    (load_scannet_data.py:100); ``axis_align`` float64 [4,4]."""
    seg_indices: np.ndarray
    seg_ids: np.ndarray
    seg_label: np.ndarray
    seg_object: np.ndarray
    num_instances: int
    object_label: np.ndarray
    axis_align: np.ndarray


def _rows_of(seg_ids, segs):
    """rows of the raw segment ids ``segs`` in the ascending ``seg_ids``; a segment that no vertex carries is the reference's
    ``seg_to_verts[seg]`` KeyError"""
    segs = np.asarray(segs, np.int64).reshape(-1)
    rows = np.minimum(np.searchsorted(seg_ids, segs), len(seg_ids) - 1)
    missing = seg_ids[rows] != segs
    if missing.any():
        raise KeyError(int(segs[np.argmax(missing)]))
    return rows


def scan_tables(seg_indices, seg_groups, label_map, axis_align=None):
    """``seg_indices``: the ``segIndices`` list (one int per vertex); ``seg_groups``: the ``segGroups`` list of dicts with
    ``objectId``, ``label``, ``segments``; ``label_map``: {raw_category: nyu40id}; ``axis_align``: the 16 numbers of the
    ``axisAlignment`` line (row-major) or None for the identity -> ``ScanTables``.  Host only, nothing is modified.

    The groups are walked as load_scannet_data.py:26-42 and :88-100 walk them.  ``label_to_segs[label]`` IS the segment list of
    the label's first object and later objects of the label extend it, so that object's list ends with their segments too;
    labels are written in the order the labels first appear, objects in the order their ids first appear, and the last writer
    of a segment wins.  Raises as the reference fails: KeyError for a label outside ``label_map``, for a group segment that no
    vertex carries and for an object that ends without segments; ValueError for object ids that are not exactly 1 .. K and for
    more than VDETR_EXPORT_MAX_INSTANCES objects."""
    seg = np.asarray(seg_indices)
    if seg.ndim != 1 or len(seg) < 1 or seg.dtype.kind not in "iu":
        raise ValueError("seg_indices must hold one integer per vertex")
    seg_ids, inverse = np.unique(seg.astype(np.int64), return_inverse=True)
    object_segs, label_segs = {}, {}
    for group in seg_groups:
        object_id = int(group["objectId"]) + 1
        segs = [int(s) for s in group["segments"]]
        object_segs[object_id] = segs
        if group["label"] in label_segs:
            label_segs[group["label"]].extend(segs)
        else:
            label_segs[group["label"]] = segs                             # the same list: the alias of :41
    K = len(object_segs)
    if K > L.VDETR_EXPORT_MAX_INSTANCES:
        raise ValueError(f"{K} objects > VDETR_EXPORT_MAX_INSTANCES {L.VDETR_EXPORT_MAX_INSTANCES}")
    if sorted(object_segs) != list(range(1, K + 1)):
        raise ValueError(f"object ids must be exactly 1 .. {K} (objectId + 1), got {sorted(object_segs)[:8]} ...")
    seg_label = np.zeros(len(seg_ids), np.int32)
    for label, segs in label_segs.items():
        label_id = int(label_map[label])
        if not 0 <= label_id < MAX_LABEL:
            raise ValueError(f"label id {label_id} of {label!r} outside 0 .. {MAX_LABEL - 1}")
        seg_label[_rows_of(seg_ids, segs)] = label_id
    seg_object = np.zeros(len(seg_ids), np.int32)
    object_label = np.zeros(K, np.int32)
    for object_id, segs in object_segs.items():
        rows = _rows_of(seg_ids, segs)
        if len(rows) == 0:
            raise KeyError(object_id)                                     # object_id_to_label_id[obj_id] of :103
        seg_object[rows] = object_id
        object_label[object_id - 1] = seg_label[rows[0]]
    matrix = np.eye(4) if axis_align is None else np.array(axis_align, np.float64).reshape(4, 4)
    return ScanTables(np.ascontiguousarray(inverse.reshape(-1), dtype=np.int32), seg_ids, seg_label, seg_object, K, object_label, matrix)


def _id_table(ids, values, what):
    """a dense int32 look-up table over 0 .. max(ids): ``values`` at ``ids``, -1 elsewhere"""
    ids = [int(i) for i in ids]
    if any(not 0 <= i < MAX_LABEL for i in ids):
        raise ValueError(f"{what} must lie in 0 .. {MAX_LABEL - 1}")
    table = np.full(max(ids) + 1 if ids else 0, -1, np.int32)
    for i, v in zip(ids, values):
        table[i] = v
    return table


def export_scans(vertices, offsets, tables, dataset_config, *, donotcare_ids=(), obj_class_ids=OBJ_CLASS_IDS):
    """``export`` + ``export_one_scan`` for a packed batch of raw scans.  vertices [N,6+] f32 on the device (xyz first, as
    ``read_mesh_vertices_rgb`` returns them; rows may be strided, e.g. seven-column ply rows), offsets [B+1] on the host as in
    ``prepare_scenes``, tables: B ``ScanTables``; ``obj_class_ids``: OBJ_CLASS_IDS, each a key of
    ``dataset_config.nyu40id2class``; ``donotcare_ids``: DONOTCARE_CLASS_IDS.  -> dict of device tensors:

    ``mesh_vertices`` [N',W] the packed cloud, columns 0:3 aligned and the others untouched, and its ``offsets`` (host int64);
    ``semantic_labels`` / ``instance_labels`` int32 [N']; ``instance_bboxes`` [B,Kmax,7] f32, ``export``'s table before the class
    filter (Kmax: the largest object count of the batch; a row of zeros is an object without vertices or a slot past the scene's
    objects); and what ``crop_and_sample`` / ``prepare_scenes`` take: ``boxes`` [B,Kmax,6] f32, the rows of the kept classes in
    ascending object id with zero rows after them, ``box_nyu40`` / ``box_classes`` [B,Kmax] int64, ``box_counts`` [B] int64
    (``prepare_scenes`` takes at most ``max_num_obj`` slots: slice ``[:, :64]`` when a scan has more objects).

    Two launches on the current stream and no synchronisation.  A non-empty ``donotcare_ids`` removes the vertices with those
    semantic labels, order kept (batch_load_scannet_data.py:33-36; the boxes are those of all vertices, as in the reference):
    N' and the offsets change, which costs a third launch and ONE read-back of a count per scene.  No CPU path."""
    off, sizes = _packed_scenes(vertices, offsets, 6, "export_scans", name="vertices", strided=True, gpu=False)
    tables = list(tables)
    B, N = len(off) - 1, vertices.shape[0]
    if len(tables) != B:
        raise ValueError(f"{len(tables)} scan tables for {B} scenes")
    for b, (t, n) in enumerate(zip(tables, sizes)):
        if len(t.seg_indices) != n:
            raise ValueError(f"scene {b}: tables made for {len(t.seg_indices)} vertices, the scene has {n}")
        if t.num_instances > L.VDETR_EXPORT_MAX_INSTANCES or len(t.object_label) != t.num_instances:
            raise ValueError(f"scene {b}: {t.num_instances} objects (at most VDETR_EXPORT_MAX_INSTANCES {L.VDETR_EXPORT_MAX_INSTANCES}, "
                             f"{len(t.object_label)} labels)")
    nyu40id2class = dataset_config.nyu40id2class
    class_table = _id_table(obj_class_ids, [nyu40id2class[int(i)] for i in obj_class_ids], "obj_class_ids")
    drop_table = np.maximum(_id_table(donotcare_ids, [1] * len(donotcare_ids), "donotcare_ids"), 0)   # 1: dropped, 0: kept
    L.require_gpu(vertices, "vertices")                                # after the host checks, which need no device
    dev = vertices.device
    vertices = vertices.detach()
    W = vertices.shape[1]
    Kmax = max((t.num_instances for t in tables), default=0)

    f32, i32, i64 = (dict(dtype=d, device=dev) for d in (torch.float32, torch.int32, torch.int64))
    ret = {"mesh_vertices": torch.empty((N, W), **f32), "offsets": off, "semantic_labels": torch.empty(N, **i32),
           "instance_labels": torch.empty(N, **i32), "instance_bboxes": torch.empty((B, Kmax, 7), **f32),
           "boxes": torch.empty((B, Kmax, 6), **f32), "box_nyu40": torch.empty((B, Kmax), **i64),
           "box_classes": torch.empty((B, Kmax), **i64), "box_counts": torch.empty(B, **i64)}
    if B == 0:
        return ret

    # one upload per table: the scenes' segment tables end to end, every vertex's segment as a row of them
    seg_base = np.cumsum([0] + [len(t.seg_label) for t in tables])
    seg_rows = np.concatenate([t.seg_indices.astype(np.int64) + base for t, base in zip(tables, seg_base)]).astype(np.int32)
    counts = np.array([t.num_instances for t in tables], np.int32)
    labels = np.zeros((B, Kmax), np.int32)
    for b, t in enumerate(tables):
        labels[b, :t.num_instances] = t.object_label
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)  # noqa: E731
    seg_rows_dev, seg_label_dev = up(seg_rows), up(np.concatenate([t.seg_label for t in tables]).astype(np.int32))
    seg_object_dev, counts_dev, labels_dev = up(np.concatenate([t.seg_object for t in tables]).astype(np.int32)), up(counts), up(labels)
    align_dev = up(np.stack([np.asarray(t.axis_align, np.float64).reshape(16) for t in tables]))
    class_dev, drop_dev = up(class_table), up(drop_table)
    off32, off_dev, host = _upload_offsets(off, dev)

    d = L.ScanExportDesc()
    d.B, d.W, d.vert_stride, d.Kmax = B, W, vertices.stride(0), Kmax
    d.num_segments, d.class_table_len, d.drop_table_len = int(seg_base[-1]), len(class_table), len(drop_table)
    d.vertices, d.offsets, d.seg_indices = vertices.data_ptr(), off_dev.data_ptr(), seg_rows_dev.data_ptr()
    d.seg_label, d.seg_object, d.num_instances = seg_label_dev.data_ptr(), seg_object_dev.data_ptr(), counts_dev.data_ptr()
    d.object_label, d.axis_align, d.class_table, d.drop_table = (labels_dev.data_ptr(), align_dev.data_ptr(), class_dev.data_ptr(),
                                                                 drop_dev.data_ptr())
    d.out_vertices, d.semantic, d.instance = ret["mesh_vertices"].data_ptr(), ret["semantic_labels"].data_ptr(), ret["instance_labels"].data_ptr()
    d.instance_bboxes, d.boxes, d.box_nyu40 = ret["instance_bboxes"].data_ptr(), ret["boxes"].data_ptr(), ret["box_nyu40"].data_ptr()
    d.box_classes, d.box_counts = ret["box_classes"].data_ptr(), ret["box_counts"].data_ptr()
    alive = [vertices, seg_rows_dev, seg_label_dev, seg_object_dev, counts_dev, labels_dev, align_dev, class_dev, drop_dev, off_dev, off32, ret]
    kept = None
    if len(drop_table):
        kept = (torch.empty((N, W), **f32), torch.empty(N, **i32), torch.empty(N, **i32), torch.empty(B, **i32))
        d.kept_vertices, d.kept_semantic, d.kept_instance, d.kept_counts = (t.data_ptr() for t in kept)
        alive.append(kept)
    nbytes = L.lib().vdetr_scan_export_workspace_bytes(host, B, Kmax)
    ws = L.workspace(nbytes, dev)
    _launch_export(d, host, counts, ws, nbytes, alive)
    if kept is not None:
        rows = kept[3].cpu().numpy().astype(np.int64)                  # the one read-back
        total = int(rows.sum())
        ret["mesh_vertices"], ret["semantic_labels"], ret["instance_labels"] = kept[0][:total], kept[1][:total], kept[2][:total]
        ret["offsets"] = np.concatenate([[0], np.cumsum(rows)])
    return ret


def _launch_export(d, host_offsets, host_counts, ws, nbytes, alive):
    """the launches on the current stream (tools/scan_export_bench.py times exactly these and holds on to ``alive``)"""
    L.check(L.lib().vdetr_scan_export_f32(ctypes.byref(d), host_offsets, host_counts.ctypes.data_as(ctypes.c_void_p), L.ptr(ws), nbytes,
                                          L.stream_ptr()), "scan_export")
