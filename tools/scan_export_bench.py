#!/usr/bin/env python3
"""Times the scan export on a scan-sized input (150 k vertices in 1 500 segments, 40 objects) as one scan and as
a batch of four such scans:

  * host: the numpy restatement (tests/scan_export_restatement.py) and ``scan_tables`` per scan, on one core, in this process,
    which never opens the GPU; and, where the reference is at hand (the build container), its own ``export`` on the same scan,
    run by tools/make_scan_export_golden.py's wrapper;
  * device, in a child process under ``timeout``: the launches of ``export_scans`` alone between HIP events (buffers allocated
    and tables uploaded before; three windows of 200 so the spread shows; where the host enqueues slower than the device runs,
    the figure is the enqueue rate and says so), without and with a drop table, and whole ``export_scans`` calls on the host
    clock, uploads included.

Every line carries its leg's tag.  A leg that cannot run where the tool runs (no reference, no GPU) keeps the lines that the
output file already holds for it and says nothing new: the file is completed by a run in the build container and one on the GPU.
``[kernel]`` lines are never written here: they are the per-kernel averages of the trace below, copied in, and are kept.

    python tools/scan_export_bench.py [--out profiles/scan_export_bench.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/scan_export_bench.py --device-leg --one-scan   # per kernel: one scan, no drop table
"""
import os
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):   # one core for numpy, before it loads
    os.environ[_v] = "1"
import subprocess  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scan_export_restatement as SR  # noqa: E402
from test_scan_export_restatement import make_scan  # noqa: E402

VERTICES, OBJECTS = 150_000, 40
BATCHES = (("one scan", 1), ("batch", 4))
REPEATS = 3
TAGS = ("[reference]", "[host]", "[device]", "[kernel]")


def scan(seed=0):
    return make_scan(np.random.default_rng(seed), VERTICES, OBJECTS, seg_size=100, cover=0.8)


def clock(fn, repeats=REPEATS):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return min(times)


def reference_leg(emit):
    from oracle import make_golden as MG
    if not os.path.isdir(os.path.join(MG.REF, "scannet")):
        return False
    import contextlib
    import io
    import make_scan_export_golden as G
    s = scan()
    with contextlib.redirect_stdout(io.StringIO()):
        G.run_reference(s, ())                                         # imports, first call
        t0 = time.perf_counter()
        got = G.run_reference(s, ())
        ms = (time.perf_counter() - t0) * 1e3
    mine = SR.export(s["mesh"], s["seg_indices"], s["groups"], s["label_map"], s["axis_align"])
    assert all(a.tobytes() == got[k].tobytes() for a, k in zip(mine[1:4], ("ex_labels", "ex_instances", "ex_bboxes")))
    emit(f"[reference] export + export_one_scan of the reference on one scan ({VERTICES} vertices, {OBJECTS} objects), JSON parsing and "
         f"the four np.save included, one core of the build container: {ms:.0f} ms (one run after a first; labels and boxes equal the restatement's bits)")
    return True


def host_leg(emit):
    from vdetr_amd.scan_export import scan_tables
    s = scan()
    args = (s["mesh"], s["seg_indices"], s["groups"], s["label_map"], s["axis_align"])
    emit(f"[host] numpy restatement of export + export_one_scan, one core, one scan ({VERTICES} vertices, {len(set(s['seg_indices']))} "
         f"segments, {OBJECTS} objects): {clock(lambda: SR.export_one_scan(*args)):.1f} ms per scan (best of {REPEATS})")
    emit(f"[host] scan_tables (the host half of export_scans), one core: {clock(lambda: scan_tables(*args[1:])):.1f} ms per scan "
         f"(best of {REPEATS}; the segIndices list -> array conversion included)")


def device_leg():
    import torch
    from vdetr_amd import scan_export as SE
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    assert torch.cuda.is_available(), "the device leg needs a GPU"
    print(f"[device] {torch.cuda.get_device_name(0)}")
    cfg = ScannetDatasetConfig()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s = scan()
    args = (s["mesh"], s["seg_indices"], s["groups"], s["label_map"], s["axis_align"])
    tables = SE.scan_tables(*args[1:])
    one_scan = "--one-scan" in sys.argv                                # under a kernel trace: one shape per kernel name
    for name, B in BATCHES[:1] if one_scan else BATCHES:
        verts = torch.from_numpy(np.concatenate([s["mesh"]] * B)).cuda()
        off = np.arange(B + 1) * VERTICES
        for drop in ((),) if one_scan else ((), (1, 2)):
            want = SR.export_one_scan(*args, donotcare_ids=drop)
            seen, real = [], SE._launch_export
            SE._launch_export = lambda *a: (seen.append(a), real(*a))[1]
            try:
                got = SE.export_scans(verts, off, [tables] * B, cfg, donotcare_ids=drop)
            finally:
                SE._launch_export = real
            last = got["offsets"][-2]
            assert got["mesh_vertices"][last:].cpu().numpy().tobytes() == want[0].tobytes()
            assert np.array_equal(got["instance_labels"][last:].cpu().numpy(), want[2])
            assert got["boxes"][-1, :len(want[3])].cpu().numpy().tobytes() == want[3][:, :6].astype(np.float32).tobytes()
            fn = lambda: real(*seen[0])  # noqa: E731
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            windows, host = [], []
            for _ in range(3):
                t0 = time.perf_counter()
                e0.record()
                for _ in range(200):
                    fn()
                e1.record()
                host.append((time.perf_counter() - t0) / 200 * 1e6)
                torch.cuda.synchronize()
                windows.append(e0.elapsed_time(e1) / 200 * 1e3)
            bound = "host enqueue" if min(host) > 0.9 * min(windows) else "device"
            launches = "the three launches (drop table 1, 2)" if drop else "the two launches"
            print(f"[device] {name} ({B} x {VERTICES} vertices, {OBJECTS} objects), results equal the restatement's bits: {launches} "
                  f"{min(windows):.1f} us per batch between events (3 windows of 200: {min(windows):.1f} .. {max(windows):.1f}; host enqueue "
                  f"{min(host):.1f} us: {bound}-bound) = {min(windows) / B:.1f} us per scan")
        SE.export_scans(verts, off, [tables] * B, cfg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPEATS):
            SE.export_scans(verts, off, [tables] * B, cfg)
        torch.cuda.synchronize()
        print(f"[device] {name}: export_scans, whole call (tables concatenated and uploaded, two launches), host clock: "
              f"{(time.perf_counter() - t0) / REPEATS * 1e3:.2f} ms per batch")


def main():
    if "--device-leg" in sys.argv:
        device_leg()
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "scan_export_bench.txt")
    old = open(out).read().splitlines() if os.path.exists(out) else []
    lines = {tag: [] for tag in TAGS}

    def emit(s):
        print(s, flush=True)
        lines[s.split(" ", 1)[0]].append(s)

    if not reference_leg(emit):
        lines["[reference]"] = [s for s in old if s.startswith("[reference]")]
    lines["[kernel]"] = [s for s in old if s.startswith("[kernel]")]
    host_leg(emit)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--device-leg"], capture_output=True, text=True)
    measured = [s for s in r.stdout.splitlines() if s.startswith("[device]")]
    status = r.returncode if measured else 0
    for s in measured:
        emit(s)
    if not measured:                                                   # no GPU here (the child's first assertion)
        lines["[device]"] = [s for s in old if s.startswith("[device]")] or ["[device] no GPU here: not measured"]
    elif status != 0:
        emit(f"[device] the device leg ended with status {status}: the rest is not measured")
        sys.stderr.write(r.stderr[-4000:])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(s for tag in TAGS for s in lines[tag]) + "\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
