"""GPU: APCalculator(resident=True) — the detections appended to a device store (vdetr_det_append_f32), matched once for all
thresholds (vdetr_box3d_iou_max_idx_f64) and turned into curves and AP on the device (vdetr_voc_ap_f64) — against the reference's
recorded metrics and against the host path of the same class: ranking and true-positive flags equal, curves equal, AP within the
two-summation-orders bound."""
import functools
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, K, C, G = 6, 70, 4, 5          # scenes (fed as calls of 2, 3, 1), queries, classes, ground-truth slots
CALLS = (2, 3, 1)
CONFIGS = {"per_class": dict(), "objectness": dict(per_class_proposal=False),
           "cls_confidence": dict(per_class_proposal=False, use_cls_confidence_only=True), "angle_conf": dict(angle_conf=True),
           "no_nms": dict(no_nms=True)}
TIE = (20, 41)                    # two boxes of scene 0 with bit-equal scores, far from everything else


def _config(name):
    from vdetr_amd.ap_calculator import get_ap_config_dict
    return get_ap_config_dict(dataset_config=types.SimpleNamespace(num_semcls=C), remove_empty_box=False, conf_thresh=0.05,
                              **CONFIGS[name])


@functools.lru_cache(maxsize=None)
def _scenes():
    """Six scenes.  Scene 1 keeps no box (every objectness below conf_thresh), scene 2 has no present ground truth, ground truth
    is of classes 0, 1, 3 only while class 3 is never a box's best class (ground truth without detection in the one-class-per-box
    forms) and class 2 is predicted but never labelled; boxes TIE of scene 0 share every probability."""
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    ds = ScannetDatasetConfig()
    rng = np.random.default_rng(7)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))  # noqa: E731
    gt_centers, gt_sizes = rng.uniform(1, 9, (S, G, 3)), rng.uniform(0.6, 1.4, (S, G, 3))
    gt_cls = rng.choice([0, 1, 3], (S, G))
    gt_cls[0, :3] = (0, 1, 3)
    present = np.ones((S, G), np.float32)
    present[2] = 0
    present[4, 3:] = 0
    centers, sizes = rng.uniform(0, 10, (S, K, 3)), rng.uniform(0.4, 1.2, (S, K, 3))
    # one box per ground-truth box: a tight one (IoU > 0.5) on the even slots, a loose one (about 0.3) on the odd slots ...
    centers[:, :G] = gt_centers + rng.normal(0, 0.03, (S, G, 3)) + np.array([0, 0.2, 0, 0.2, 0])[None, :, None] * gt_sizes
    sizes[:, :G] = gt_sizes * rng.uniform(0.92, 1.08, (S, G, 3))
    centers[:, G:2 * G] = gt_centers + rng.normal(0, 0.12, (S, G, 3))      # ... and a worse duplicate (suppressed, or a false positive)
    sizes[:, G:2 * G] = gt_sizes
    centers[0, TIE[0]], centers[0, TIE[1]] = (20, 20, 1), (30, 30, 1)
    sem = rng.uniform(0.05, 1, (S, K, C))
    sem[..., 3] *= 0.01                                                    # class 3 is never the arg-max
    for s in range(S):
        for g in range(G):
            if gt_cls[s, g] != 3:
                sem[s, g, gt_cls[s, g]] = sem[s, G + g, gt_cls[s, g]] = 1.5
    obj, ang = rng.uniform(0.1, 1, (S, K)), rng.uniform(0.5, 1, (S, K))
    obj[1] = 0.01
    sem[0, TIE[1]], obj[0, list(TIE)], ang[0, TIE[1]] = sem[0, TIE[0]], 0.9, ang[0, TIE[0]]
    centers, sizes = f32(centers), f32(sizes)
    out = {"box_corners": ds.box_parametrization_to_corners(centers, sizes, torch.zeros(S, K)), "sem_cls_prob": f32(sem),
           "objectness_prob": f32(obj), "angle_prob": f32(ang), "center_unnormalized": centers, "size_unnormalized": sizes,
           "angle_continuous": torch.zeros(S, K)}
    tgt = {"point_clouds": torch.zeros(S, 8, 3), "gt_box_sem_cls_label": torch.from_numpy(gt_cls).long(),
           "gt_box_corners": ds.box_parametrization_to_corners(f32(gt_centers), f32(gt_sizes), torch.zeros(S, G)) * f32(present)[..., None, None],
           "gt_box_present": f32(present)}
    return ({k: v.to(DEV) for k, v in out.items()}, {k: v.to(DEV) for k, v in tgt.items()})


def _feed(calc):
    out, tgt = _scenes()
    at = 0
    for b in CALLS:
        calc.step_meter({"outputs": {k: v[at:at + b] for k, v in out.items()}}, {k: v[at:at + b] for k, v in tgt.items()})
        at += b
    return calc


def _calc(name, **kw):
    from vdetr_amd.ap_calculator import APCalculator
    cfg = _config(name)
    return APCalculator(dataset_config=cfg["dataset_config"], ap_iou_thresh=[0.25, 0.5], ap_config_dict=cfg, **kw)


@functools.lru_cache(maxsize=None)
def _host(name):
    """the reference of every comparison: the host path, computed once per configuration and left unchanged"""
    calc = _feed(_calc(name))
    return dict(calc=calc, metrics=calc.compute_metrics(), ranking=calc._ranking(), curves=calc._curves())


def _same_metrics(got, want):
    assert list(got.keys()) == list(want.keys())
    for thr in want:
        assert list(got[thr].keys()) == list(want[thr].keys()), thr
        for key, w in want[thr].items():
            if key.endswith("Recall") or key == "AR":
                assert float(got[thr][key]) == float(w), (thr, key)
            else:   # AP (fp64) and the float32 mAP: two summation orders of at most G * S + 1 terms whose sum is <= 1
                assert abs(float(got[thr][key]) - float(w)) <= (G * S + 1) * 2.0 ** -52 + (2.0 ** -23 if key == "mAP" else 0), (thr, key)


def test_reference_fixture_metrics_and_text():
    from test_oracle_ap import NUM_SEMCLS
    from vdetr_amd.ap_calculator import APCalculator, get_ap_config_dict
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "ap_calculator.npz"))
    class2type = {int(i): str(n) for i, n in zip(z["class_ids"], z["class_names"])}
    cfg = types.SimpleNamespace(num_semcls=NUM_SEMCLS)
    calc = APCalculator(dataset_config=cfg, ap_iou_thresh=[0.25, 0.5], class2type_map=class2type, exact_eval=True,
                        ap_config_dict=get_ap_config_dict(dataset_config=cfg, remove_empty_box=True), resident=True)
    for bi in range(int(z["nbatch"])):
        out = {k.split(":")[2]: torch.from_numpy(z[k]).to(DEV) for k in z.files if k.startswith(f"b{bi}:out:")}
        tgt = {k.split(":")[2]: torch.from_numpy(z[k]).to(DEV) for k in z.files if k.startswith(f"b{bi}:tgt:")}
        calc.step_meter({"outputs": out}, tgt)
    ret = calc.compute_metrics()
    for thr in (0.25, 0.5):
        assert list(ret[thr].keys()) == [str(k) for k in z[f"t{thr}:keys"]]
        got = np.array([float(v) for v in ret[thr].values()])
        assert np.allclose(got, z[f"t{thr}:values"], rtol=1e-7, atol=1e-12), thr
    assert calc.metrics_to_str(ret) == str(z["text"])
    assert str(calc) == str(z["text"])
    assert calc.metrics_to_dict(ret).keys() == {"mAP_0.25", "AR_0.25", "mAP_0.5", "AR_0.5"}
    with pytest.raises(ValueError, match="resident"):
        calc.accumulate([], [])


def test_constructed_scenes_hold_every_case():
    """the inputs of the comparisons below really contain what they are meant to (read from the host path's own arrays)"""
    host = _host("objectness")
    calc = host["calc"]
    assert len(calc._flat_pred[1][2]) == 0 and all(len(calc._flat_pred[s][2]) > 0 for s in (0, 2, 3, 4, 5))   # scene 1 keeps nothing
    assert len(calc._flat_gt[2][0]) == 0 and len(calc._flat_gt[4][0]) == 3 and len(calc._flat_gt[0][0]) == G  # scene 2: nothing present
    rec, _, ap = host["curves"][0.25]
    assert sorted(ap) == [0, 1, 2, 3]
    assert isinstance(rec[3], int) and ap[3] == 0                       # class 3: ground truth, no detection
    gt_classes = np.concatenate([calc._flat_gt[s][0] for s in range(S)])
    assert 2 not in gt_classes and isinstance(rec[2], np.ndarray) and rec[2].size > 0 and not rec[2].any()   # class 2: detections only
    assert 0 < ap[0] <= 1 and 0 < ap[1] <= 1
    tp25, tp50 = host["ranking"][0.25][1], host["ranking"][0.5][1]
    assert tp50.sum() > 0 and tp25.sum() > tp50.sum()                   # the two thresholds see different true positives
    for name in CONFIGS:                                                # the tie survives every configuration's NMS and scoring
        corners, cls, idx, score = _host(name)["calc"]._flat_pred[0]
        out, _ = _scenes()
        kept = np.nonzero(np.isin(corners[:, 0, 0], out["box_corners"][0, list(TIE), 0, 0].cpu().numpy()))[0]
        assert len(kept) == 2, name
        a, b = (score[(idx == k)] for k in kept)
        assert np.array_equal(a, b) and len(a) == (C if name in ("per_class", "angle_conf", "no_nms") else 1), name


@pytest.mark.parametrize("name", list(CONFIGS))
def test_resident_equals_the_host_path(name):
    host = _host(name)
    calc = _feed(_calc(name, resident=True))
    _same_metrics(calc.compute_metrics(), host["metrics"])
    assert calc.metrics_to_str(calc.compute_metrics()) == host["calc"].metrics_to_str(host["metrics"])
    ranking = calc._ranking()
    for thr, (order, tp) in host["ranking"].items():
        assert np.array_equal(ranking[thr][0], order), thr                # the ranked order, ties included
        assert np.array_equal(ranking[thr][1], tp), thr                   # and who is a true positive
        assert tp.any()
    curves = calc._curves()
    gt_classes = np.concatenate([host["calc"]._flat_gt[s][0] for s in range(S)])
    for thr, (rec, prec, ap) in host["curves"].items():
        got_rec, got_prec, got_ap = curves[thr]
        assert sorted(got_ap) == sorted(ap)
        for c in ap:
            if isinstance(rec[c], np.ndarray):
                assert np.array_equal(got_rec[c], rec[c]) and np.array_equal(got_prec[c], prec[c]), (thr, c)
            else:
                assert got_rec[c] == 0 and got_prec[c] == 0
            npos = int((gt_classes == c).sum())
            print(f"{name} thr {thr} class {c}: AP {float(got_ap[c])!r} host {float(ap[c])!r} npos {npos}")
            assert abs(float(got_ap[c]) - float(ap[c])) <= (npos + 1) * 2.0 ** -52, (thr, c)


def test_voc_ap_walks_long_segments_backwards_in_chunks():
    """vdetr_voc_ap_f64 alone on segments longer than its chunk of 2048 ranks: three chunks with a partial last one, exactly one
    chunk, no rank at all; a class without ground truth among the long ones.  Against the curve and the VOC-12 AP of the host
    path (eval_det.evaluate_flat's cumsums and eval_det.voc_ap): curves, last recall and counts equal, AP within the bound of
    two summation orders."""
    from vdetr_amd import eval_det, eval_store
    chunk = 2048
    lengths = (2 * chunk + 37, 0, chunk, 2 * chunk + 37)
    seg = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    rng = np.random.default_rng(11)
    tp = rng.random((2, seg[-1])) < np.array([[0.3], [0.05]])              # T = 2: many and few true positives
    npos = np.array([int(tp[:, seg[c]:seg[c + 1]].sum(1).max()) + 7 for c in range(len(lengths))], np.int32)
    npos[3] = 0
    to_dev = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    out, rec, prec = eval_store.voc_ap(to_dev(tp.astype(np.uint8)), to_dev(seg), to_dev(npos), curves=True)
    out, rec, prec = out.cpu().numpy(), rec.cpu().numpy(), prec.cpu().numpy()
    for t in range(2):
        for c, n in enumerate(lengths):
            sel = tp[t, seg[c]:seg[c + 1]]
            tpc, fpc = np.cumsum(sel.astype(np.float64)), np.cumsum((~sel).astype(np.float64))
            r = tpc / float(npos[c]) if npos[c] else np.zeros_like(tpc)
            p = tpc / np.maximum(tpc + fpc, np.finfo(np.float64).eps)
            ap = eval_det.voc_ap(r, p) if n else 0.0
            assert np.array_equal(rec[t, seg[c]:seg[c + 1]], r) and np.array_equal(prec[t, seg[c]:seg[c + 1]], p), (t, c)
            assert out[t, 1, c] == (r[-1] if n else 0.0) and out[t, 2, c] == n and out[t, 3, c] == npos[c], (t, c)
            print(f"thr {t} class {c}: AP {float(out[t, 0, c])!r} host {float(ap)!r} npos {npos[c]}")
            assert abs(float(out[t, 0, c]) - float(ap)) <= (int(npos[c]) + 1) * 2.0 ** -52, (t, c)
            assert (ap > 0) == (n > 0 and npos[c] > 0)


def _rows(B, Kq, Gq, rng, keep_p, present_p):
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(DEV)  # noqa: E731
    keep = torch.from_numpy(rng.random((B, Kq)) < keep_p).to(DEV)
    present = torch.from_numpy(rng.random((B, Gq)) < present_p).to(DEV)
    return dict(keep=keep, corners=f(B, Kq, 8, 3), scores=f(B, Kq, 3), cls=torch.from_numpy(rng.integers(0, 9, (B, Kq))).to(DEV),
                gt_corners=f(B, Gq, 8, 3), gt_cls=torch.from_numpy(rng.integers(0, 9, (B, Gq))).to(DEV), gt_present=present)


@pytest.mark.parametrize("Kq,Gq", [(48, 5), (70, 0), (1100, 300)])
def test_append_kernel_rows_and_cursors(Kq, Gq):
    """the store after every call against np.nonzero of keep / present: rows in (scene, ascending index) order, begins, counters;
    B changes between the calls; a call that keeps everything, one that keeps nothing, all-zero `present`"""
    from vdetr_amd.eval_store import DetectionStore
    rng = np.random.default_rng(Kq)
    store = DetectionStore(3, DEV, initial_capacity=64)
    want = {k: [] for k in ("box_corners", "box_scores", "box_cls", "box_scan", "gt_corners", "gt_cls")}
    box_begin, gt_begin, scans = [0], [0], 0
    for B, keep_p, present_p in ((2, 0.4, 0.5), (3, 1.0, 0.0), (1, 0.0, 1.0), (4, 0.5, 0.5)):
        r = _rows(B, Kq, Gq, rng, keep_p, present_p)
        store.append(**r)
        h = {k: v.cpu().numpy() for k, v in r.items()}
        for b in range(B):
            js, gs = np.nonzero(h["keep"][b])[0], np.nonzero(h["gt_present"][b])[0]
            want["box_corners"].append(h["corners"][b][js]), want["box_scores"].append(h["scores"][b][js])
            want["box_cls"].append(h["cls"][b][js]), want["box_scan"].append(np.full(len(js), scans))
            want["gt_corners"].append(h["gt_corners"][b][gs]), want["gt_cls"].append(h["gt_cls"][b][gs])
            box_begin.append(box_begin[-1] + len(js)), gt_begin.append(gt_begin[-1] + len(gs))
            scans += 1
        got = store.to_host()
        assert got["counts"] == (box_begin[-1], gt_begin[-1], scans, 0)
        assert np.array_equal(got["box_begin"], box_begin) and np.array_equal(got["gt_begin"], gt_begin)
        for k, parts in want.items():
            assert np.array_equal(got[k], np.concatenate(parts)), (k, B)
    assert store.box_capacity >= 10 * Kq and box_begin[-1] > 3 * Kq       # it grew, and the all-kept call is in


def test_growth_from_a_small_store():
    want = _host("per_class")["metrics"]
    small = _feed(_calc("per_class", resident=True, initial_capacity=16))
    large = _feed(_calc("per_class", resident=True, initial_capacity=1 << 14))
    assert small._store.box_capacity >= S * K > 16 and large._store.box_capacity == 1 << 14
    a, b = small.compute_metrics(), large.compute_metrics()
    assert small._last_result.tobytes() == large._last_result.tobytes()
    _same_metrics(a, want)
    _same_metrics(b, want)


def test_fixed_capacity_too_small_raises_and_the_next_calculator_is_right():
    host = _host("objectness")
    kept = sum(len(host["calc"]._flat_pred[s][2]) for s in range(S))
    assert kept > 8
    calc = _feed(_calc("objectness", resident=True, capacity=8))
    with pytest.raises(RuntimeError, match=rf"\b{kept - 8} rows dropped"):
        calc.compute_metrics()
    roomy = _feed(_calc("objectness", resident=True, capacity=S * K))
    _same_metrics(roomy.compute_metrics(), host["metrics"])


def test_step_meter_reads_nothing_back():
    out, tgt = _scenes()
    calc = _calc("per_class", resident=True, initial_capacity=16)
    first = ({"outputs": {k: v[:2] for k, v in out.items()}}, {k: v[:2] for k, v in tgt.items()})
    rest = ({"outputs": {k: v[2:] for k, v in out.items()}}, {k: v[2:] for k, v in tgt.items()})
    calc.step_meter(*first)     # (first call: library, allocator and workspaces warm)
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            raises = False
        except RuntimeError:
            raises = True
        if raises:
            calc.step_meter(*rest)   # (the store grows here: 16 rows < 6 x 70)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raises:
        calc.step_meter(*rest)
    want = _feed(_calc("per_class", resident=True))
    _same_metrics(calc.compute_metrics(), want.compute_metrics())
    assert calc._last_result.tobytes() == want._last_result.tobytes()
    if not raises:
        pytest.skip("this runtime ignores torch.cuda.set_sync_debug_mode: the no-host-read check did not run (parity did, and passed)")


def test_one_matching_pass_for_two_thresholds():
    from vdetr_amd import eval_store
    calc = _feed(_calc("per_class", resident=True))
    before = eval_store.MATCH_LAUNCHES
    calc.compute_metrics()
    assert len(calc.ap_iou_thresh) == 2 and eval_store.MATCH_LAUNCHES - before == 1


def test_two_runs_give_the_same_bits():
    runs = []
    for _ in range(2):
        calc = _feed(_calc("angle_conf", resident=True))
        calc.compute_metrics()
        host = calc._store.to_host()
        runs.append((calc._last_result.tobytes(), {k: v.tobytes() for k, v in host.items() if k != "counts"}, host["counts"]))
    assert runs[0] == runs[1]
