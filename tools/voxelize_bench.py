"""Voxelisation of raw clouds: the map launches of sparse_ops.voxel_map against the composition they replace.

    python tools/voxelize_bench.py [--rounds 9] [--reps 20] [--out profiles/voxelize_bench.txt]

Two shapes: one 40k-point cloud (the C2 shape of bench.py) and 4 x 100k-point clouds, 6 feature columns, 2 cm voxels (several
points per voxel).  Per shape and route, the time from the list of clouds to (sites, the sites' feature rows):
  (a) composition  batch_sparse_collate + pack_keys(check=True) + the torch.unique / scatter_reduce(amin) of the former
                   insert_points + features[unique_index], restated here from the same torch calls
  (b) voxel_map    one torch.cat, the keys launch, a stable sort, the two sites launches, ONE host read, features[first]
  (c) (b) with the average mode's fold (voxel_reduce) in place of the row gather: the extra cost of UNWEIGHTED_AVERAGE
"device" is the time between two events around `reps` calls, per call; "host" is the wall time of the same calls with a
synchronise at both ends, per call (both routes end in host reads, so the two are close; the host figure is what a training
step waits for).  Rounds alternate the routes behind one untimed round; medians and ranges are printed.  The two routes are
compared word for word before anything is timed.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clouds_of(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:  # a floor and a wall, as the suite's scenes
        u = torch.rand((n, 2), generator=g)
        floor = torch.stack((u[:, 0] * 8, u[:, 1] * 6, torch.zeros(n)), 1)
        wall = torch.stack((u[:, 0] * 8, torch.zeros(n), u[:, 1] * 3), 1)
        xyz = torch.cat((floor[: n // 2], wall[n // 2:])) + 1.0 + torch.rand((n, 3), generator=g) * 0.02
        out.append(torch.cat((xyz, torch.rand((n, 6), generator=g)), 1).cuda())
    return out


def composition(clouds, voxel):
    from vdetr_amd import minkowski as ME
    from vdetr_amd import sparse_ops as S
    coordinates, features = ME.batch_sparse_collate([(p[:, :3] / voxel, p[:, 3:]) for p in clouds])
    keys_in = S.pack_keys(coordinates)
    num_scenes = int(coordinates[:, 0].max()) + 1
    keys, inverse = torch.unique(keys_in, return_inverse=True)
    first = torch.full((keys.shape[0],), keys_in.shape[0], dtype=torch.int64, device=keys.device)
    first.scatter_reduce_(0, inverse, torch.arange(keys_in.shape[0], device=keys.device), reduce="amin")
    return keys, first, features[first], num_scenes


def mapped(clouds, voxel, mode="first"):
    from vdetr_amd import sparse_ops as S
    packed = clouds[0] if len(clouds) == 1 else torch.cat(clouds)
    offsets = [0]
    for p in clouds:
        offsets.append(offsets[-1] + p.shape[0])
    vm = S.voxel_map(packed, offsets, voxel)
    feats = packed[:, 3:]
    rows = feats[vm.first] if mode == "first" else S.voxel_reduce(feats.contiguous(), vm, mode)
    return vm.sites, vm.first, rows, vm.num_scenes


def timed(fn, reps):
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps, (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxelize_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "voxelize_bench needs a GPU"
    lines = [f"voxelize_bench: voxel {args.voxel} m, 6 feature columns; {args.rounds} alternating rounds of {args.reps} calls behind 1 "
             "untimed; device = events around the calls, host = wall time synchronised at both ends; ms per call"]
    result = {"tool": "voxelize_bench", "voxel": args.voxel, "rounds": args.rounds, "reps": args.reps, "shapes": {}}
    for name, sizes in (("1x40k", (40000,)), ("4x100k", (100000,) * 4)):
        clouds = clouds_of(sizes, len(sizes))
        a, b = composition(clouds, args.voxel), mapped(clouds, args.voxel)
        same = all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
        routes = {"composition": lambda: composition(clouds, args.voxel), "voxel_map": lambda: mapped(clouds, args.voxel),
                  "voxel_map+average": lambda: mapped(clouds, args.voxel, "average")}
        times = {r: [] for r in routes}
        for rnd in range(args.rounds + 1):
            for r, fn in routes.items():
                t = timed(fn, args.reps)
                if rnd:
                    times[r].append(t)
        lines.append(f"{name}: {sum(sizes)} points -> {a[0].shape[0]} sites; keys, first rows and feature rows of the two routes equal: {same}")
        shape = {"points": sum(sizes), "sites": int(a[0].shape[0]), "same": bool(same)}
        for r in routes:
            dev, host = [t[0] for t in times[r]], [t[1] for t in times[r]]
            shape[r] = {"device_ms": statistics.median(dev), "host_ms": statistics.median(host)}
            lines.append(f"  {r:18s} device median {statistics.median(dev):7.3f} ({min(dev):.3f}-{max(dev):.3f})   "
                         f"host median {statistics.median(host):7.3f} ({min(host):.3f}-{max(host):.3f})")
        extra = shape["voxel_map+average"]["host_ms"] - shape["voxel_map"]["host_ms"]
        lines.append(f"  voxel_map / composition (host) = {shape['voxel_map']['host_ms'] / shape['composition']['host_ms']:.2f}; "
                     f"the average mode's extra cost {extra:+.3f} ms")
        result["shapes"][name] = shape
    lines.append(json.dumps(result))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
