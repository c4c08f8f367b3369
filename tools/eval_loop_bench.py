#!/usr/bin/env python3
"""The evaluation loop's join between forward and metrics, host path against the resident store, on synthetic
outputs of the C2 evaluation shape: 8 scenes per batch, 1024 queries, 18 classes, 40,000 points, 64 ground-truth slots of which
about 20 are present.  The queries cluster around 48 objects per scene (20 of them the ground truth), so the NMS has work to do.

  (a) host wall time per batch of ``APCalculator.step_meter`` behind device work that is still running: every batch first enqueues
      a stand-in for the forward (``--forward-ms`` of matrix products, no synchronise), then calls step_meter.  The host path waits
      for that work and copies seven tensors; the resident path launches and returns.  Also the wall time per batch of the whole
      loop, its final synchronise included.
  (b) ``compute_metrics`` over ``--batches`` such batches.

The two paths alternate, ``--rounds`` times each; medians and the spread are printed.
python tools/eval_loop_bench.py --steps 39 --warmup 5

``--sizes`` runs one other leg instead: the S / M / L metrics of ``--test_size`` on the same batches, read-back of
the store plus host path three times against one ``compute_metrics_by_size()``.
python tools/eval_loop_bench.py --sizes"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vdetr_amd.ap_calculator import APCalculator, get_ap_config_dict  # noqa: E402
from vdetr_amd.dataset_config import ScannetDatasetConfig  # noqa: E402

B, K, C, N, G, OBJECTS, PRESENT = 8, 1024, 18, 40000, 64, 48, 20


def make_batch(seed, dev):
    ds = ScannetDatasetConfig()
    rng = np.random.default_rng(seed)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))  # noqa: E731
    obj_c, obj_s = rng.uniform(0.5, 7.5, (B, OBJECTS, 3)), rng.uniform(0.3, 1.5, (B, OBJECTS, 3))
    obj_k = rng.integers(0, C, (B, OBJECTS))
    which = rng.integers(0, OBJECTS, (B, K))
    take = lambda a: np.take_along_axis(a, which[..., None], 1)  # noqa: E731
    centers = take(obj_c) + rng.normal(0, 0.06, (B, K, 3))
    sizes = take(obj_s) * rng.uniform(0.85, 1.15, (B, K, 3))
    sem = rng.uniform(0, 0.2, (B, K, C))
    np.put_along_axis(sem, np.take_along_axis(obj_k, which, 1)[..., None], rng.uniform(0.5, 1.0, (B, K, 1)), -1)
    present = np.zeros((B, G), np.float32)
    present[:, :PRESENT] = 1
    gt_c, gt_s, gt_k = np.zeros((B, G, 3)), np.ones((B, G, 3)), np.zeros((B, G), np.int64)
    gt_c[:, :PRESENT], gt_s[:, :PRESENT], gt_k[:, :PRESENT] = obj_c[:, :PRESENT], obj_s[:, :PRESENT], obj_k[:, :PRESENT]
    centers, sizes = f32(centers), f32(sizes)
    out = {"box_corners": ds.box_parametrization_to_corners(centers, sizes, torch.zeros(B, K)), "sem_cls_prob": f32(sem),
           "objectness_prob": f32(rng.uniform(0.05, 1, (B, K))), "angle_prob": torch.ones(B, K), "center_unnormalized": centers,
           "size_unnormalized": sizes, "angle_continuous": torch.zeros(B, K)}
    tgt = {"point_clouds": f32(rng.uniform(0, 8, (B, N, 3))), "gt_box_sem_cls_label": torch.from_numpy(gt_k),
           "gt_box_corners": ds.box_parametrization_to_corners(f32(gt_c), f32(gt_s), torch.zeros(B, G)) * f32(present)[..., None, None],
           "gt_box_present": f32(present)}
    return {"outputs": {k: v.to(dev) for k, v in out.items()}}, {k: v.to(dev) for k, v in tgt.items()}


def sizes_leg(a, make, batches):
    """--sizes: the S / M / L metrics of --test_size over ``--batches`` batches in a resident calculator.
    (a) the route taken before the device path existed: per size the store is read back, expanded into per-scan tuples and handed
        to the host path (numpy filter, upload, vdetr_box3d_iou_max_f64, curves in numpy) — three times;
    (b) one ``compute_metrics_by_size()``: one matching launch and one AP launch for all three, two host reads."""
    from vdetr_amd.eval_store import expand_host, size_classes
    sizes = ("S", "M", "L")
    calc = make(True)
    for i in range(a.batches):
        calc.step_meter(*batches[i % len(batches)])
    store = calc._store
    kept = store.read_counters()
    count = lambda corners, n: torch.bincount(size_classes(corners, n).long(), minlength=4).cpu().tolist()  # noqa: E731
    det_sizes, gt_sizes = count(store.box_corners, kept[0]), count(store.gt_corners, kept[1])

    def read_back():
        host, ret = make(False), {}
        for size in sizes:
            host._flat_pred, host._flat_gt = expand_host(store.to_host(), calc._num_classes, calc._per_class)
            host.scan_cnt = calc.scan_cnt
            ret[size] = host.compute_metrics(size)
        return ret

    def one_pass():
        calc._size_cache = None
        return calc.compute_metrics_by_size()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ret = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, ret

    for _ in range(max(1, a.warmup // 5)):     # every shape once, untimed
        read_back(), one_pass()
    ms, rets = {"read_back": [], "one_pass": []}, {}
    for _ in range(a.rounds):
        for name, fn in (("read_back", read_back), ("one_pass", one_pass)):
            t, rets[name] = timed(fn)
            ms[name].append(t)
    same = all(abs(float(rets["read_back"][s][t][k]) - float(rets["one_pass"][s][t][k])) <= 1e-6
               for s in sizes for t in rets["read_back"][s] for k in rets["read_back"][s][t])
    med = {n: statistics.median(v) for n, v in ms.items()}
    span = lambda v: f"{min(v):.1f}-{max(v):.1f}"  # noqa: E731
    print(f"eval_loop_bench --sizes: {B} scenes x {K} queries x {C} classes per batch, {a.batches} batches; {a.rounds} alternating rounds "
          f"behind {max(1, a.warmup // 5)} untimed; wall time, synchronised at both ends")
    print(f"store: {kept[0]} kept boxes, {kept[1]} ground-truth boxes, {kept[2]} scans; detections = boxes x {C} classes")
    print(f"boxes in S / M / L / none: {det_sizes}; ground-truth boxes in S / M / L / none: {gt_sizes}")
    print(f"(a) three compute_metrics(size), store read back + host path: median {med['read_back']:.1f} ms (rounds {span(ms['read_back'])})")
    print(f"(b) one compute_metrics_by_size() on the device:              median {med['one_pass']:.1f} ms (rounds {span(ms['one_pass'])})")
    print(f"(a) / (b) = {med['read_back'] / med['one_pass']:.1f}; metrics of the two routes agree to 1e-6: {same}")
    print(json.dumps({"tool": "eval_loop_bench", "leg": "sizes", "batches": a.batches, "rounds": a.rounds, "kept_boxes": kept[0],
                      "boxes_by_size": det_sizes, "gt_by_size": gt_sizes, "read_back_ms": med["read_back"], "one_pass_ms": med["one_pass"],
                      "same_metrics": bool(same)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=39, help="timed batches per round of (a)")
    ap.add_argument("--warmup", type=int, default=5, help="untimed batches in front of every round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=39, help="batches behind compute_metrics in (b)")
    ap.add_argument("--forward-ms", type=float, default=2.0, help="device time of the stand-in forward in front of every step_meter")
    ap.add_argument("--sizes", action="store_true", help="only the size-split leg: S / M / L metrics, store read-back against one device pass")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "eval_loop_bench needs a GPU"
    dev = torch.device("cuda")
    cfg_ds = types.SimpleNamespace(num_semcls=C)
    batches = [make_batch(s, dev) for s in range(4)]
    make = lambda resident: APCalculator(dataset_config=cfg_ds, ap_iou_thresh=[0.25, 0.5], resident=resident,  # noqa: E731
                                         ap_config_dict=get_ap_config_dict(dataset_config=cfg_ds, remove_empty_box=False))
    if a.sizes:
        return sizes_leg(a, make, batches)

    # the stand-in forward: as many 2048^2 products as take --forward-ms on this device
    w = torch.randn(2048, 2048, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        w @ w
    torch.cuda.synchronize()
    e0.record()
    for _ in range(20):
        w @ w
    e1.record()
    torch.cuda.synchronize()
    products = max(1, round(a.forward_ms / (e0.elapsed_time(e1) / 20)))

    def forward():
        for _ in range(products):
            w @ w

    def loop(resident):
        calc = make(resident)
        for i in range(a.warmup):
            forward()
            calc.step_meter(*batches[i % len(batches)])
        torch.cuda.synchronize()
        per_step = []
        t_loop = time.perf_counter()
        for i in range(a.steps):
            forward()
            t0 = time.perf_counter()
            calc.step_meter(*batches[i % len(batches)])
            per_step.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        return statistics.median(per_step), (time.perf_counter() - t_loop) * 1e3 / a.steps

    def metrics(resident):
        calc = make(resident)
        for i in range(a.batches):
            calc.step_meter(*batches[i % len(batches)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ret = calc.compute_metrics()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, ret, calc

    res = {"host": {"step": [], "loop": [], "metrics": []}, "resident": {"step": [], "loop": [], "metrics": []}}
    rets = {}
    metrics(True), metrics(False)          # every shape of (b) once, untimed
    for _ in range(a.rounds):
        for name, resident in (("host", False), ("resident", True)):
            step, whole = loop(resident)
            res[name]["step"].append(step), res[name]["loop"].append(whole)
        for name, resident in (("host", False), ("resident", True)):
            ms, rets[name], calc = metrics(resident)
            res[name]["metrics"].append(ms)
            if resident:
                kept = calc._store.read_counters()
    same = all(abs(float(rets["host"][t][k]) - float(rets["resident"][t][k])) <= 1e-6 for t in rets["host"] for k in rets["host"][t])
    med = {n: {k: statistics.median(v) for k, v in d.items()} for n, d in res.items()}
    span = lambda v: f"{min(v):.2f}-{max(v):.2f}"  # noqa: E731
    print(f"eval_loop_bench: {B} scenes x {K} queries x {C} classes, {N} points, {PRESENT} of {G} ground-truth boxes present; "
          f"{a.steps} timed batches behind {a.warmup} warm-up, {a.rounds} alternating rounds; stand-in forward {products} x 2048^2 "
          f"products (~{a.forward_ms} ms of device time)")
    print(f"store after {a.batches} batches: {kept[0]} kept boxes ({kept[0] / (a.batches * B):.0f} per scene), {kept[1]} ground-truth "
          f"boxes, {kept[2]} scans, {kept[3]} dropped")
    for name in ("host", "resident"):
        print(f"(a) {name:8s} step_meter host wall per batch: median {med[name]['step']:.3f} ms (rounds {span(res[name]['step'])}); "
              f"whole loop per batch incl. final synchronise: {med[name]['loop']:.3f} ms (rounds {span(res[name]['loop'])})")
    for name in ("host", "resident"):
        print(f"(b) {name:8s} compute_metrics over {a.batches} batches: median {med[name]['metrics']:.1f} ms (rounds {span(res[name]['metrics'])})")
    print(f"metrics of the two paths agree to 1e-6: {same}")
    print(json.dumps({"tool": "eval_loop_bench", "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "batches": a.batches,
                      "kept_boxes": kept[0], "step_ms": {n: med[n]["step"] for n in med}, "loop_ms": {n: med[n]["loop"] for n in med},
                      "metrics_ms": {n: med[n]["metrics"] for n in med}, "same_metrics": bool(same)}))


if __name__ == "__main__":
    main()
