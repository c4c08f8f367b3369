"""The evaluation loop's detections on the device (csrc/eval_store.hip).

``DetectionStore`` is the host side of ``vdetr_det_store``: the kept boxes and the present ground-truth boxes of every batch,
one row per box, in arrays whose cursors are device memory too.  ``append`` launches and returns: it reads nothing back.  The host
sizes the arrays by what it knows without reading, the upper bound ``sum of B * K`` of rows (``sum of B * G`` ground-truth boxes):
when a call's bound exceeds the capacity the arrays are re-allocated at least twice as large and the old ones copied on the device,
rows and cursors unchanged.  A fixed ``capacity`` caps the box rows instead; rows that do not fit are counted on the device and
``evaluate`` raises.

``evaluate`` is ``compute_metrics`` for all IoU thresholds with two host reads: the four counters (the number of detections sizes
the launches) and one ``[T, 4, C]`` buffer of results.  In between: ONE matching launch (``vdetr_box3d_iou_max_idx_f64``: ovmax /
jmax do not depend on the threshold), the ranking by two stable library sorts and the claim rule by a scatter-min as in
``eval_det.match_detections`` (written without boolean indexing, which would read a count back), and one
``vdetr_voc_ap_f64`` launch.  GPU only: there is no CPU path.

``evaluate_sizes`` is the same for the size split of ``--test_size``: every stored box gets its volume class on the
device (``vdetr_box3d_size_class_f32``), ONE size-restricted matching launch serves S, M and L (``vdetr_box3d_iou_max_size_f64``) and
``vdetr_voc_ap_f64`` runs once over ``3C`` (size, class) segments — again two host reads, and no read-back of the store.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L

MATCH_LAUNCHES = 0   # calls of the matching entry point (tests count them per compute_metrics)


class DetectionStore:
    def __init__(self, scores_per_box, device, capacity=None, initial_capacity=4096):
        self.S = int(scores_per_box)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"DetectionStore: CPU not supported (device {self.device})")
        self.fixed = capacity is not None
        self.box_capacity = int(capacity if self.fixed else initial_capacity)
        self.gt_capacity = self.scan_capacity = 0
        self.box_bound = self.gt_bound = self.nscans = 0     # what the host knows without reading: upper bounds / exact
        self.counters = torch.zeros(4, dtype=torch.int32, device=self.device)
        self._alloc_boxes(self.box_capacity, None)
        self._alloc_gt(64, None)
        self._alloc_scans(64, None)

    # ---- allocation: a larger array, the old rows copied on the device -------------------------------------------------------
    def _grown(self, old, rows, tail, dtype):
        new = torch.empty((rows,) + tail, dtype=dtype, device=self.device)
        if old is not None:
            new[:old.shape[0]].copy_(old)
        return new

    def _alloc_boxes(self, rows, old):
        o = old or (None,) * 4
        self.box_corners = self._grown(o[0], rows, (8, 3), torch.float32)
        self.box_scores = self._grown(o[1], rows, (self.S,), torch.float32)
        self.box_cls = self._grown(o[2], rows, (), torch.int32)
        self.box_scan = self._grown(o[3], rows, (), torch.int32)
        self.box_capacity = rows
        self._desc = None

    def _alloc_gt(self, rows, old):
        o = old or (None,) * 2
        self.gt_corners = self._grown(o[0], rows, (8, 3), torch.float32)
        self.gt_cls = self._grown(o[1], rows, (), torch.int32)
        self.gt_capacity = rows
        self._desc = None

    def _alloc_scans(self, scans, old):
        o = old or (None,) * 2
        self.box_begin = self._grown(o[0], scans + 1, (), torch.int32)
        self.gt_begin = self._grown(o[1], scans + 1, (), torch.int32)
        self.scan_capacity = scans
        self._desc = None

    def _reserve(self, boxes, gts, scans):
        if boxes > self.box_capacity and not self.fixed:
            self._alloc_boxes(max(boxes, 2 * self.box_capacity), (self.box_corners, self.box_scores, self.box_cls, self.box_scan))
        if gts > self.gt_capacity:
            self._alloc_gt(max(gts, 2 * self.gt_capacity), (self.gt_corners, self.gt_cls))
        if scans > self.scan_capacity:
            self._alloc_scans(max(scans, 2 * self.scan_capacity), (self.box_begin, self.gt_begin))

    def desc(self):
        if self._desc is None:
            d = L.DetStore()
            d.box_capacity, d.gt_capacity, d.scan_capacity, d.S = self.box_capacity, self.gt_capacity, self.scan_capacity, self.S
            for name in ("box_corners", "box_scores", "box_cls", "box_scan", "box_begin", "gt_corners", "gt_cls", "gt_begin", "counters"):
                setattr(d, name, getattr(self, name).data_ptr())
            self._desc = d
        return self._desc

    def append(self, keep, corners, scores, cls, gt_corners, gt_cls, gt_present):
        """keep [B,K] bool / u8, corners [B,K,8,3] f32, scores [B,K,S] f32, cls [B,K] integer; gt_corners [B,G,8,3] f32, gt_cls
        [B,G] integer, gt_present [B,G] bool / u8.  No host read."""
        L.require_gpu(keep, "keep")
        B, K = keep.shape
        G = gt_present.shape[1]
        assert corners.shape == (B, K, 8, 3) and scores.shape == (B, K, self.S) and cls.shape == (B, K)
        assert gt_corners.shape == (B, G, 8, 3) and gt_cls.shape == (B, G) and gt_present.shape == (B, G)
        if self.box_bound + B * K >= 2 ** 31 or self.gt_bound + B * G >= 2 ** 31:
            raise RuntimeError("DetectionStore: more than 2^31 rows")
        self._reserve(self.box_bound + B * K, self.gt_bound + B * G, self.nscans + B)
        u8 = lambda t: (t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)).contiguous()  # noqa: E731
        f32 = lambda t: t.detach().to(torch.float32).contiguous()                                         # noqa: E731
        i32 = lambda t: t.detach().to(torch.int32).contiguous()                                           # noqa: E731
        args = (u8(keep), f32(corners), f32(scores), i32(cls), f32(gt_corners), i32(gt_cls), u8(gt_present))
        L.check(L.lib().vdetr_det_append_f32(ctypes.byref(self.desc()), *(L.ptr(a) for a in args), B, K, G, self.nscans,
                                             L.stream_ptr()), "det_append")
        self.box_bound += B * K
        self.gt_bound += B * G
        self.nscans += B

    def read_counters(self):
        """-> (boxes, ground-truth boxes, scans, dropped rows): ONE host read."""
        return tuple(int(v) for v in self.counters.cpu().tolist())

    def require_complete(self, counts):
        if counts[3] > 0:
            raise RuntimeError(f"DetectionStore: {counts[3]} rows dropped: the fixed capacity of {self.box_capacity} boxes is too "
                               f"small ({counts[0]} were kept)")

    def to_host(self):
        """The store's rows as numpy arrays (tests and tools/eval_loop_bench.py read it back; no metric does):
        dict(counts, box_corners, box_scores, box_cls, box_scan, box_begin, gt_corners, gt_cls, gt_begin)."""
        counts = self.read_counters()
        self.require_complete(counts)
        n, g, s, _ = counts
        out = {"counts": counts}
        for name, rows in (("box_corners", n), ("box_scores", n), ("box_cls", n), ("box_scan", n), ("box_begin", s + 1),
                           ("gt_corners", g), ("gt_cls", g), ("gt_begin", s + 1)):
            out[name] = getattr(self, name)[:rows].cpu().numpy()
        return out


def match_store(store, nboxes, nscans, ngt, num_classes):
    """vdetr_box3d_iou_max_idx_f64 -> (ovmax [P] f64, jmax [P] i32, class [P] i32, score [P] f32) of the P detections in the
    reference's list order; num_classes = 0: one detection per box under its stored class."""
    global MATCH_LAUNCHES
    P = nboxes * max(num_classes, 1)
    dev = store.device
    ovmax = torch.empty(P, dtype=torch.float64, device=dev)
    jmax = torch.empty(P, dtype=torch.int32, device=dev)
    det_cls = torch.empty(P, dtype=torch.int32, device=dev)
    det_score = torch.empty(P, dtype=torch.float32, device=dev)
    MATCH_LAUNCHES += 1
    L.check(L.lib().vdetr_box3d_iou_max_idx_f64(ctypes.byref(store.desc()), nboxes, nscans, ngt, num_classes, L.ptr(ovmax), L.ptr(jmax),
                                                L.ptr(det_cls), L.ptr(det_score), L.stream_ptr()), "box3d_iou_max_idx")
    return ovmax, jmax, det_cls, det_score


def voc_ap(tp, seg, npos, curves=False):
    """vdetr_voc_ap_f64: tp [T,P] u8 in ranked order, seg [C+1] i32, npos [C] i32 -> out [T,4,C] f64 (AP, last recall, number of
    detections, npos) and, with ``curves``, rec / prec [T,P] f64."""
    T, P = tp.shape
    C = npos.shape[0]
    out = torch.empty((T, 4, C), dtype=torch.float64, device=tp.device)
    rec = torch.empty((T, P), dtype=torch.float64, device=tp.device) if curves else None
    prec = torch.empty((T, P), dtype=torch.float64, device=tp.device) if curves else None
    L.check(L.lib().vdetr_voc_ap_f64(L.ptr(tp), L.ptr(seg), L.ptr(npos), T, P, C, L.ptr(out), L.ptr(rec), L.ptr(prec), L.stream_ptr()),
            "voc_ap")
    return out, rec, prec


def evaluate(store, thresholds, num_classes, per_class, curves=False):
    """Every class's AP and last recall at every threshold.  ``num_classes`` = C: labels are 0 .. C-1; ``per_class``: every box is a
    detection of every class (scores [.,C]), else of its stored class.  -> dict(result [T,4,C] numpy f64 = AP, last recall, number of
    detections, npos; order [P] and tp [T,P] (ranked) device tensors; rec / prec [T,P] device tensors with ``curves``; seg [C+1]).
    Host reads: the counters, then the result buffer."""
    counts = store.read_counters()                                          # host read 1
    store.require_complete(counts)
    nboxes, ngt, nscans, _ = counts
    dev, C, T = store.device, int(num_classes), len(thresholds)
    P = nboxes * (C if per_class else 1)
    classes = torch.arange(C + 1, dtype=torch.int32, device=dev)
    gseg = torch.searchsorted(torch.sort(store.gt_cls[:ngt])[0], classes)
    npos = (gseg[1:] - gseg[:-1]).to(torch.int32)
    if P > 0:
        ovmax, jmax, det_cls, det_score = match_store(store, nboxes, nscans, ngt, C if per_class else 0)   # once for all thresholds
        # rank: class-major, then descending confidence, ties in insertion order (two stable sorts, eval_det.py:75-80)
        o1 = torch.sort(-det_score, stable=True)[1]
        cls_sorted, o2 = torch.sort(det_cls[o1], stable=True)
        order = o1[o2]
        rank = torch.empty(P, dtype=torch.int64, device=dev)
        rank[order] = torch.arange(P, device=dev)
        seg = torch.searchsorted(cls_sorted, classes).to(torch.int32)
        j = jmax.long()
        tps = []
        for thr in thresholds:   # the best-ranked detection of every box claims it: a scatter-min over all P, misses into a spare slot
            hit = ovmax > thr
            slot = torch.where(hit, j, ngt)
            claim = torch.full((ngt + 1,), P, dtype=torch.int64, device=dev)
            claim.scatter_reduce_(0, slot, torch.where(hit, rank, P), reduce="amin")
            tps.append((hit & (claim[slot] == rank))[order])
        tp = torch.stack(tps).view(torch.uint8)
    else:
        order = torch.zeros(0, dtype=torch.int64, device=dev)
        tp = torch.zeros((T, 0), dtype=torch.uint8, device=dev)
        seg = torch.zeros(C + 1, dtype=torch.int32, device=dev)
    out, rec, prec = voc_ap(tp, seg, npos, curves)
    return dict(result=out.cpu().numpy(), order=order, tp=tp, rec=rec, prec=prec, seg=seg)        # host read 2


def size_classes(corners, n):
    """vdetr_box3d_size_class_f32 of the first n rows of corners [.,8,3] f32 -> [n] u8: 0 = S, 1 = M, 2 = L, 3 = none (the
    reference's box3d_vol_batch in float32 against float32(0.17) and float32(0.44); a volume on a bound belongs to no size)."""
    assert corners.dtype == torch.float32 and corners.is_contiguous() and corners.shape[0] >= n and corners.shape[1:] == (8, 3)
    out = torch.empty(n, dtype=torch.uint8, device=corners.device)
    L.check(L.lib().vdetr_box3d_size_class_f32(L.ptr(corners), n, L.ptr(out), L.stream_ptr()), "box3d_size_class")
    return out


def match_store_sizes(store, nboxes, nscans, ngt, num_classes, box_size, gt_size):
    """vdetr_box3d_iou_max_size_f64: ``match_store`` with every detection competing for the ground truth of its own volume class
    only -> (ovmax, jmax, class, score, size class [P] u8)."""
    global MATCH_LAUNCHES
    P = nboxes * max(num_classes, 1)
    dev = store.device
    ovmax = torch.empty(P, dtype=torch.float64, device=dev)
    jmax = torch.empty(P, dtype=torch.int32, device=dev)
    det_cls = torch.empty(P, dtype=torch.int32, device=dev)
    det_score = torch.empty(P, dtype=torch.float32, device=dev)
    det_size = torch.empty(P, dtype=torch.uint8, device=dev)
    MATCH_LAUNCHES += 1
    L.check(L.lib().vdetr_box3d_iou_max_size_f64(ctypes.byref(store.desc()), nboxes, nscans, ngt, num_classes, L.ptr(box_size),
                                                 L.ptr(gt_size), L.ptr(ovmax), L.ptr(jmax), L.ptr(det_cls), L.ptr(det_score),
                                                 L.ptr(det_size), L.stream_ptr()), "box3d_iou_max_size")
    return ovmax, jmax, det_cls, det_score, det_size


def evaluate_sizes(store, thresholds, num_classes, per_class, curves=False):
    """``evaluate`` under the reference's size split (``--test_size``), S, M and L in one pass: segment k * C + c of the ranking
    holds size class k (0 = S, 1 = M, 2 = L), class c.  -> dict(result [3,T,4,C] numpy f64 = per size AP, last recall, number of
    detections, npos; present [2,C] numpy f64 = detections and ground-truth boxes of every class BEFORE the filter (the keys of
    every size's dictionary, eval_det.py:259-299); order [P], tp [T,P], seg [3C+1], rec / prec as ``evaluate`` gives them, the
    detections of no size ranked behind seg[3C]).  Host reads: the counters, then one buffer holding result and present."""
    counts = store.read_counters()                                          # host read 1
    store.require_complete(counts)
    nboxes, ngt, nscans, _ = counts
    dev, C, T = store.device, int(num_classes), len(thresholds)
    P = nboxes * (C if per_class else 1)
    classes = torch.arange(C + 1, dtype=torch.int32, device=dev)
    keys = torch.arange(3 * C + 1, dtype=torch.int32, device=dev)
    in_range = lambda cls: (cls >= 0) & (cls < C)  # noqa: E731
    gt_cls = store.gt_cls[:ngt]
    gt_size = size_classes(store.gt_corners, ngt)
    gseg = torch.searchsorted(torch.sort(gt_cls)[0], classes)
    gkey = torch.where((gt_size < 3) & in_range(gt_cls), gt_size.to(torch.int32) * C + gt_cls, 3 * C)   # no size: behind 3C
    gkseg = torch.searchsorted(torch.sort(gkey)[0], keys)
    npos = (gkseg[1:] - gkseg[:-1]).to(torch.int32)
    if per_class:       # every box is a detection of every class
        ndet_all = torch.full((C,), float(nboxes), dtype=torch.float64, device=dev)
    else:
        bseg = torch.searchsorted(torch.sort(store.box_cls[:nboxes])[0], classes)
        ndet_all = (bseg[1:] - bseg[:-1]).to(torch.float64)
    if P > 0:
        box_size = size_classes(store.box_corners, nboxes)
        ovmax, jmax, det_cls, det_score, det_size = match_store_sizes(store, nboxes, nscans, ngt, C if per_class else 0, box_size,
                                                                      gt_size)                 # once for all sizes and thresholds
        dkey = torch.where((det_size < 3) & in_range(det_cls), det_size.to(torch.int32) * C + det_cls, 3 * C)
        o1 = torch.sort(-det_score, stable=True)[1]          # rank: (size, class)-major, then as ``evaluate``
        key_sorted, o2 = torch.sort(dkey[o1], stable=True)
        order = o1[o2]
        rank = torch.empty(P, dtype=torch.int64, device=dev)
        rank[order] = torch.arange(P, device=dev)
        seg = torch.searchsorted(key_sorted, keys).to(torch.int32)
        j = jmax.long()
        tps = []
        for thr in thresholds:   # a box and the detections that can claim it are of one size: the claim rule needs no change
            hit = ovmax > thr
            slot = torch.where(hit, j, ngt)
            claim = torch.full((ngt + 1,), P, dtype=torch.int64, device=dev)
            claim.scatter_reduce_(0, slot, torch.where(hit, rank, P), reduce="amin")
            tps.append((hit & (claim[slot] == rank))[order])
        tp = torch.stack(tps).view(torch.uint8)
    else:
        order = torch.zeros(0, dtype=torch.int64, device=dev)
        tp = torch.zeros((T, 0), dtype=torch.uint8, device=dev)
        seg = torch.zeros(3 * C + 1, dtype=torch.int32, device=dev)
    out, rec, prec = voc_ap(tp, seg, npos, curves)                          # [T,4,3C]
    packed = torch.cat((out.reshape(-1), ndet_all, (gseg[1:] - gseg[:-1]).to(torch.float64))).cpu().numpy()   # host read 2
    result = np.ascontiguousarray(packed[:T * 4 * 3 * C].reshape(T, 4, 3, C).transpose(2, 0, 1, 3))
    return dict(result=result, present=packed[T * 4 * 3 * C:].reshape(2, C), order=order, tp=tp, rec=rec, prec=prec, seg=seg)


def expand_host(host, num_classes, per_class):
    """``DetectionStore.to_host()`` -> per scan the tuples ``ap_calculator.detections_flat`` makes (corners [n,8,3], classes [m],
    box index [m], scores [m]) and (ground-truth classes [g], corners [g,8,3]): what a host calculator's ``_flat_pred`` / ``_flat_gt``
    hold.  The size split went this way before ``evaluate_sizes``; tools/eval_loop_bench.py --sizes still times it."""
    preds, gts = {}, {}
    bb, gb = host["box_begin"], host["gt_begin"]
    for s in range(host["counts"][2]):
        rows = slice(int(bb[s]), int(bb[s + 1]))
        n = rows.stop - rows.start
        corners, score = host["box_corners"][rows], host["box_scores"][rows]
        if per_class:
            preds[s] = (corners, np.repeat(np.arange(num_classes), n), np.tile(np.arange(n), num_classes),
                        np.ascontiguousarray(score[:, :num_classes].T).ravel())
        else:
            preds[s] = (corners, host["box_cls"][rows].astype(np.int64), np.arange(n), score[:, 0])
        g = slice(int(gb[s]), int(gb[s + 1]))
        gts[s] = (host["gt_cls"][g].astype(np.int64), host["gt_corners"][g])
    return preds, gts
