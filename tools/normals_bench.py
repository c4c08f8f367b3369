#!/usr/bin/env python3
"""Times the vertex normals on a scan-sized grid mesh (150 k vertices, 300 k faces) as one scene and as a batch
of four such scenes:

  * the numpy restatement (tests/normals_restatement.py) per scene, on one core, in this process, which never opens the GPU;
  * the device, in a child process under ``timeout``: the seven launches alone between HIP events (buffers allocated and the
    faces uploaded before; three windows of 200 so the spread shows; where the host enqueues slower than the device runs, the
    figure is the enqueue rate and says so) and whole ``vertex_normals`` calls on the host clock, the upload of the faces included.

    python tools/normals_bench.py [--out profiles/normals_bench.txt]
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
import normals_restatement as NR  # noqa: E402

GRID = (388, 388)            # 150 544 vertices, 299 538 faces
BATCHES = (("one scan", 1), ("batch", 4))
REPEATS = 3


def mesh(seed=0):
    rng = np.random.default_rng(seed)
    nx, ny = GRID
    gx, gy = np.meshgrid(np.linspace(-4, 4, nx), np.linspace(-3, 3, ny), indexing="ij")
    xyz = np.stack([gx, gy, rng.uniform(0, 0.05, gx.shape)], -1).reshape(-1, 3).astype(np.float32)
    at = np.arange(nx * ny).reshape(nx, ny)
    a, b, c, d = at[:-1, :-1], at[1:, :-1], at[:-1, 1:], at[1:, 1:]
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([b, d, c], -1).reshape(-1, 3)]).astype(np.int32)
    return xyz, faces


def clock(fn, repeats=REPEATS):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return min(times)


def host_leg(emit):
    xyz, faces = mesh()
    ms = clock(lambda: NR.vertex_normals(xyz, faces))
    emit(f"numpy restatement, one core, one scan ({len(xyz)} vertices, {len(faces)} faces): {ms:.1f} ms per scene (best of {REPEATS}); "
         f"the reference's own Python loop over the faces is not timed here")


def device_leg():
    import torch
    from vdetr_amd import scene_prep as SP
    assert torch.cuda.is_available(), "the device leg needs a GPU"
    print(f"device: {torch.cuda.get_device_name(0)}")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    xyz, faces = mesh()
    want = NR.vertex_normals(xyz, faces)
    for name, B in BATCHES:
        verts = torch.from_numpy(np.concatenate([xyz] * B)).cuda()
        faces_host = np.concatenate([faces] * B)
        faces_dev = torch.from_numpy(faces_host).cuda()
        voff, foff = np.arange(B + 1) * len(xyz), np.arange(B + 1) * len(faces)
        seen, real = [], SP._launch_normals
        SP._launch_normals = lambda *a: (seen.append(a), real(*a))[1]
        try:
            got = SP.vertex_normals(verts, voff, faces_dev, foff)
        finally:
            SP._launch_normals = real
        assert got[:len(xyz)].cpu().numpy().tobytes() == want.tobytes() and got[-len(xyz):].cpu().numpy().tobytes() == want.tobytes()
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
        print(f"{name} ({B} x {len(xyz)} vertices, {B} x {len(faces)} faces), results equal the restatement's bits: the seven launches "
              f"{min(windows):.1f} us per batch between events (3 windows of 200: {min(windows):.1f} .. {max(windows):.1f}; host enqueue "
              f"{min(host):.1f} us: {bound}-bound) = {min(windows) / B:.1f} us per scene")
        SP.vertex_normals(verts, voff, faces_host, foff)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPEATS):
            SP.vertex_normals(verts, voff, faces_host, foff)
        torch.cuda.synchronize()
        print(f"{name}: vertex_normals, whole call with host faces (range check, upload, seven launches), host clock: "
              f"{(time.perf_counter() - t0) / REPEATS * 1e3:.2f} ms per batch")


def main():
    if "--device-leg" in sys.argv:
        device_leg()
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "normals_bench.txt")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    host_leg(emit)
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--device-leg"], capture_output=True, text=True)
    for s in r.stdout.splitlines():
        emit(s)
    if r.returncode != 0:
        emit(f"device leg ended with status {r.returncode}: not measured")
        sys.stderr.write(r.stderr[-4000:])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
