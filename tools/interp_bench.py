#!/usr/bin/env python3
"""Trilinear interpolation (csrc/sparse_interp.hip: sparse_ops.interp_map / interpolate) against the ATen composition a user would
write without it, in ONE process, the arms alternated round by round: medians of the rounds with their spread (device events
around a window of calls, each window after an untimed call of its own arm).

Tables: the two of tools/sparse_modules_bench.py — one scene's sites on a floor and a wall, [35018, 64] at tensor stride 4 and
[4830, 256] at tensor stride 16 — read at a cloud of 40k points (one scene) and at 4 x 100k points (four scenes, each with its own
copy of the sites).  The points lie on the floor and the wall, up to half a cell off the surfaces: the corners off the planes are
absent, as they are for a real scan.
Phases: the map (nbr, w); the map with the backward's order / seg (a stable library sort and one launch, once per map); the
forward; forward + backward through autograd on a cached map.
Composition: eight ``torch.searchsorted`` on the keys with the weights as tensor expressions; ``index_select`` of the 8 N rows,
multiply, sum over the corners; autograd's ``index_add_`` backward.
Reported with the bytes each phase NEEDS over its time, as GB/s and as a share of the HBM peak:
  map       16 N (tfield) + 64 N (nbr, w) + 8 M (keys)           (+ 32 N order + 4 M seg with the fold)
  forward   4 C (M + N) + 64 N
  fwd+bwd   forward + 4 C (N + M) + 64 N (w, order) + 4 M (seg)
No threshold: what comes out is written down, rows where ATen wins included.

    python tools/interp_bench.py [--out profiles/interp_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s
BIAS = 32768


def plane_sites(nx, ny, nz, ts, seed, scenes):
    """a floor nx x ny and a wall nx x nz of cells of size ts, 3 % of them missing, copied into every scene: [M, 4] sorted"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    floor = np.stack((x.ravel(), y.ravel(), np.zeros(x.size, np.int64)), 1)
    x, z = np.meshgrid(np.arange(nx), np.arange(1, nz + 1), indexing="ij")
    wall = np.stack((x.ravel(), np.zeros(x.size, np.int64), z.ravel()), 1)
    c = np.concatenate((floor, wall)) * ts
    c = c[rng.random(len(c)) > 0.03]
    return np.unique(np.concatenate([np.concatenate((np.full((len(c), 1), b, np.int64), c), 1) for b in range(scenes)]), axis=0)


def plane_points(nx, ny, nz, ts, n, scenes, seed):
    """n points per scene on the floor and the wall of ``plane_sites``, up to half a cell off the surface: [scenes * n, 4] fp32"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(scenes):
        u = rng.random((n, 3))
        floor = np.stack((u[:, 0] * (nx - 1), u[:, 1] * (ny - 1), u[:, 2] * 0.5), 1)
        wall = np.stack((u[:, 0] * (nx - 1), u[:, 1] * 0.5, 1 + u[:, 2] * (nz - 1)), 1)
        p = np.where((np.arange(n) % 2 == 0)[:, None], floor, wall) * ts
        out.append(np.concatenate((np.full((n, 1), float(b)), p), 1))
    return np.concatenate(out).astype(np.float32)


def aten_map(keys, s, tfield):
    """the composition: eight searchsorted on the keys (points inside the key range, as the bench's are)"""
    b = tfield[:, 0].to(torch.int64) << 48
    lo = torch.div(torch.floor(tfield[:, 1:]).to(torch.int64), s, rounding_mode="floor") * s
    t = (tfield[:, 1:] - lo.to(torch.float32)) / float(s)
    last = keys.shape[0] - 1
    nbr, w = [], []
    for k in range(8):
        bits = ((k >> 2) & 1, (k >> 1) & 1, k & 1)
        c = [lo[:, a] + bits[a] * s + BIAS for a in range(3)]
        key = b | (c[0] << 32) | (c[1] << 16) | c[2]
        at = torch.searchsorted(keys, key).clamp_(max=last)
        hit = keys[at] == key
        f = [t[:, a] if bits[a] else 1.0 - t[:, a] for a in range(3)]
        nbr.append(torch.where(hit, at, -1))
        w.append(torch.where(hit, f[0] * f[1] * f[2], 0.0))
    return torch.stack(nbr, 1).to(torch.int32), torch.stack(w, 1)


def aten_interpolate(feats, nbr, w):
    rows = nbr.clamp(min=0).to(torch.int64).view(-1)
    return (feats.index_select(0, rows).view(nbr.shape[0], 8, -1) * w[:, :, None]).sum(1)


def rounds(arms, n_rounds, inner):
    """arms: {name: callable} -> {name: sorted ms per call, one entry per round}; the arms alternate inside every round"""
    times = {k: [] for k in arms}
    for it in range(n_rounds + 1):  # (round 0 warms every arm and is dropped)
        for name, fn in arms.items():
            fn()  # not timed: the window starts from the state this arm leaves
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if it:
                times[name].append(e0.elapsed_time(e1) / inner)
    return {k: sorted(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("interp_bench: needs a GPU (no number is produced without one)")
    from vdetr_amd import sparse_ops as S
    dev = torch.device("cuda:0")
    med = lambda v: v[len(v) // 2]  # noqa: E731
    spread = lambda v: 100.0 * (v[-1] - v[0]) / med(v)  # noqa: E731
    lines = [f"trilinear interpolation vs the ATen composition; median of {args.rounds} alternated rounds of {args.inner} calls (ms per call) "
             f"and the rounds' spread (max - min over the median), {torch.cuda.get_device_name(0)}",
             f"needed bytes: see tools/interp_bench.py; share = of the {HBM_PEAK_GBS / 1000:.0f} TB/s HBM peak (bandwidth-bound)"]
    shapes = {"s4 C64": (190, 150, 40, 4, 0, 64), "s16 C256": (70, 55, 16, 16, 1, 256)}
    wins = []
    for tname, (nx, ny, nz, ts, seed, C) in shapes.items():
        for cname, (scenes, per) in {"40k": (1, 40000), "4x100k": (4, 100000)}.items():
            sites = plane_sites(nx, ny, nz, ts, seed, scenes)
            keys = S.pack_keys(torch.from_numpy(sites).to(dev))
            tfield = torch.from_numpy(plane_points(nx, ny, nz, ts, per, scenes, 7)).to(dev)
            M, N = keys.shape[0], tfield.shape[0]
            g = torch.Generator().manual_seed(0)
            feats = torch.randn(M, C, generator=g).to(dev)
            dy = torch.randn(N, C, generator=g).to(dev)
            imap = S.interp_map(keys, ts, tfield)
            imap.order  # the cached map of the forward / backward rows carries its fold
            a_nbr, a_w = aten_map(keys, ts, tfield)
            same = bool(torch.equal(a_nbr, imap.nbr))
            present = float((imap.nbr >= 0).float().mean())
            per_site = torch.bincount(imap.nbr[imap.nbr >= 0].view(-1).long(), minlength=M)
            lines.append(f"--- table {tname}: {M} sites x {C} channels at stride {ts}, cloud {cname}: {N} points; {100 * present:.1f}% of the "
                         f"pair slots present, pairs per site median {int(per_site.median())} / max {int(per_site.max())}; nbr == the composition's: {same}")
            lines.append(f"{'phase':<16}{'kernels':>18}{'ATen':>18}{'speed-up':>10}{'GB/s':>9}{'share':>8}")
            xk, xa = feats.clone().requires_grad_(True), feats.clone().requires_grad_(True)

            def both(x, fn):
                x.grad = None
                fn(x).backward(dy)

            def map_and_fold():
                S.interp_map(keys, ts, tfield).order

            phases = {
                "map": ({"kernels": lambda: S.interp_map(keys, ts, tfield), "ATen": lambda: aten_map(keys, ts, tfield)},
                        16 * N + 64 * N + 8 * M),
                "map + fold": ({"kernels": map_and_fold}, 16 * N + 64 * N + 8 * M + 32 * N + 4 * M),
                "forward": ({"kernels": lambda: S.interpolate(feats, imap), "ATen": lambda: aten_interpolate(feats, a_nbr, a_w)},
                            4 * C * (M + N) + 64 * N),
                "fwd+bwd": ({"kernels": lambda: both(xk, lambda x: S.interpolate(x, imap)),
                             "ATen": lambda: both(xa, lambda x: aten_interpolate(x, a_nbr, a_w))},
                            2 * 4 * C * (M + N) + 2 * 64 * N + 4 * M),
            }
            for pname, (arms, need) in phases.items():
                t = rounds(arms, args.rounds, args.inner)
                k = t["kernels"]
                gbs = need / (med(k) * 1e-3) / 1e9
                if "ATen" in t:
                    a = t["ATen"]
                    ratio = med(a) / med(k)
                    if ratio < 1.0:
                        wins.append(f"{tname} {cname} {pname} ({ratio:.2f}x)")
                    lines.append(f"{pname:<16}{med(k):>9.4f} ±{spread(k):>5.1f}%{med(a):>10.4f} ±{spread(a):>5.1f}%{ratio:>10.2f}{gbs:>9.0f}"
                                 f"{100 * gbs / HBM_PEAK_GBS:>7.1f}%")
                else:
                    lines.append(f"{pname:<16}{med(k):>9.4f} ±{spread(k):>5.1f}%{'':>18}{'':>10}{gbs:>9.0f}{100 * gbs / HBM_PEAK_GBS:>7.1f}%")
            err = (xk.grad - xa.grad).abs().max().item() / xa.grad.abs().max().item()
            lines.append(f"largest |dF kernels - dF ATen| / max |dF| = {err:.2e}")
    lines.append("rows where the ATen composition is faster: " + (", ".join(wins) if wins else "none"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
