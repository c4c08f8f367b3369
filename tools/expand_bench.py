#!/usr/bin/env python3
"""The key set of an expanding layer (``CoordinateManager.expanded``: the region-keys launch of csrc/sparse_voxel.hip, the stable
sort, the sites pass, one host read) against the ATen composition that ``CoordinateManager.generated`` uses (``unpack_keys``,
``repeat``, ``pack_keys`` with its four host reads of the range, ``torch.unique``), in ONE process, the two sides alternated round
by round.  A host clock around a whole call that ends in a device synchronise: both sides include their host reads, their offset
upload and the launches; each call runs on a fresh coordinate manager, so that no cache answers.  Median / min of the timed rounds
after a warm-up of both.

Tables: one scene's sites on a floor and a wall, ~35k sites at tensor stride 4 and ~5k at tensor stride 16 (the tables of the other
sparse benches).
Rows.  cube3/s1: the expanded set of a 3^3 stride-1 convolution (u = v - offset * ts), against the composition written out here
(``generated`` with the sign and stride of that case).  tr-cube2/s2: the children of a 2^3 stride-2 transposed convolution, against
``cm.generated`` itself.  Both sides give the same keys (asserted).

    python tools/expand_bench.py [--out profiles/expand_bench.txt]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sparse_modules_bench import launches, plane_sites  # noqa: E402


def host_timed(arms, iters, warmup):
    """arms: {name: callable}; -> {name: sorted wall times in ms of a call between two device synchronisations}"""
    times = {k: [] for k in arms}
    for it in range(warmup + iters):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {k: sorted(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("expand_bench: needs a GPU (no number is produced without one)")
    from vdetr_amd import minkowski as ME
    from vdetr_amd import sparse_ops as S
    dev = torch.device("cuda:0")
    med = lambda v: v[len(v) // 2]  # noqa: E731
    lines = [f"expanded key sets: the region-keys launch + sort + sites pass (cm.expanded) vs the ATen composition of cm.generated; median "
             f"/ min of {args.iters} alternated rounds (ms, host clock around a synchronised call, host reads and offset upload included, "
             f"a fresh coordinate manager per call), {torch.cuda.get_device_name(0)}",
             f"{'table':<10}{'row':<13}{'sites in':>9}{'sites out':>10}{'candidates':>11}{'expanded':>17}{'ATen':>17}{'ATen / expanded':>16}"
             f"{'launches e/a':>14}"]
    tables = {"s4": (plane_sites(190, 150, 40, 4, 0), 4), "s16": (plane_sites(70, 55, 16, 16, 1), 16)}
    for tname, (sites, ts) in tables.items():
        keys = S.pack_keys(torch.from_numpy(sites).to(dev))
        cube3, cube2 = ME._Offsets(ME._kernel_offsets(3)), ME._Offsets(ME._kernel_offsets(2))

        def aten_expanded():
            # cm.generated's composition with the step of the stride-1 case: u = v - offset * ts
            c = S.unpack_keys(keys).to(torch.int64)
            off = -torch.tensor(cube3, dtype=torch.int64, device=dev) * ts
            child = c[:, None, :].repeat(1, off.shape[0], 1)
            child[:, :, 1:] += off[None]
            return torch.unique(S.pack_keys(child.reshape(-1, 4)))

        rows = (("cube3/s1", 27, lambda: ME.CoordinateManager(dev).expanded(keys, ts, ts, cube3, False), aten_expanded),
                ("tr-cube2/s2", 8, lambda: ME.CoordinateManager(dev).expanded(keys, ts, ts // 2, cube2, True),
                 lambda: ME.CoordinateManager(dev).generated(keys, ts // 2, cube2)))
        for rname, K, new, old in rows:
            a, b = new(), old()
            assert torch.equal(a, b), (tname, rname)
            t = host_timed({"expanded": new, "aten": old}, args.iters, args.warmup)
            me, ma = med(t["expanded"]), med(t["aten"])
            lines.append(f"{tname:<10}{rname:<13}{len(sites):>9}{a.shape[0]:>10}{K * len(sites):>11}"
                         f"{me:>9.4f} /{t['expanded'][0]:>6.3f}{ma:>9.4f} /{t['aten'][0]:>6.3f}{ma / me:>16.2f}"
                         f"{launches(new) + ' / ' + launches(old):>14}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
