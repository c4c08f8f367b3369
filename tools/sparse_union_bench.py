#!/usr/bin/env python3
"""The union add, the union map and MinkowskiPruning's two halves (csrc/sparse_union.hip) against the ATen compositions a user would
write without them, in ONE process, the arms alternated call by call, median / min of the timed calls after a warm-up of all of
them (device events around a whole call) — the method of tools/sparse_modules_bench.py, whose helpers this tool imports.

Tables: one scene's sites on a floor and a wall, [~35k, 64] at tensor stride 4 and [~5k, 256] at tensor stride 16, each with its
generated superset (the 8 children of every site of the next coarser stride: what a generative up block hands to the skip add).
  union add   skip [n, C] + generated [8 m, C] on the union.  ATen: ``torch.zeros(nu, C)`` plus two ``index_add_`` through row_a /
              row_b (three launches forward; autograd's two index_select backward).  Bytes needed: 4 C (na + nb + nu) + 8 nu
              forward, the same again + 4 (na + nb) with the backward.
  union map   the two launches and the one host read.  ATen: ``torch.unique(torch.cat((a, b)))`` and two ``torch.searchsorted``
              (row_a, row_b; src_a / src_b not even built).  Both arms end with the size on the host.
  pruning     half of the rows kept at random: ``prune_map`` + ``take_rows`` (the read of nk between them) against ``x[mask]`` and its
              autograd.  Bytes needed: 13 N + 12 nk + 8 C nk forward, + 4 C (nk + N) + 4 N with the backward.
The ``bwd`` rows time the backward LAUNCHES alone on both arms (two ``take_rows`` against two ``index_select``; one ``take_rows``
against ``zeros_like`` + ``index_put_``): through autograd a Python ``Function``'s backward costs the engine about 0.1 ms of host
time per call, which at these sizes is more than the launches and is what the ``fwd+bwd`` rows mostly show.
Launches per call are counted with torch.profiler.  A HIP form slower than the ATen one is said so in the last line of the tables.
The neck: ``backbone_forward`` forward + backward (train mode) of one 40k-point scene with woexpand_conv False (generative up
blocks, union adds, nothing pruned) against True (the default), with the sites of every level — for information.

    python tools/sparse_union_bench.py [--out profiles/sparse_union_bench.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sparse_modules_bench import HBM_PEAK_GBS, launches, plane_sites, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--neck-iters", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_union_bench: needs a GPU (no number is produced without one)")
    from vdetr_amd import minkowski as ME
    from vdetr_amd import sparse_ops as S
    dev = torch.device("cuda:0")
    med = lambda v: v[len(v) // 2]  # noqa: E731
    lines = [f"union add / union map / pruning vs ATen compositions; median / min of {args.iters} alternated calls (ms), each after an "
             f"untimed call of its own arm, {torch.cuda.get_device_name(0)}",
             f"share = needed bytes over the time, of the {HBM_PEAK_GBS / 1000:.0f} TB/s HBM peak; launches = HIP form / ATen form"]
    tables = {"s4 C64": (plane_sites(190, 150, 40, 4, 0), 4, 64), "s16 C256": (plane_sites(70, 55, 16, 16, 1), 16, 256)}
    slower = []
    for tname, (sites, ts, C) in tables.items():
        keys = S.pack_keys(torch.from_numpy(sites).to(dev))
        cm = ME.CoordinateManager(dev)
        cm.keys[ts], cm.num_scenes = keys, 1
        gen = cm.generated(cm.strided(keys, ts, 2 * ts), ts, 2)
        u, row_a, row_b, src_a, src_b = S.union_map(keys, gen)
        na, nb, nu = keys.shape[0], gen.shape[0], u.shape[0]
        g = torch.Generator().manual_seed(0)
        fa = torch.randn(na, C, generator=g).to(dev).requires_grad_(True)
        fb = torch.randn(nb, C, generator=g).to(dev).requires_grad_(True)
        dy = torch.randn(nu, C, generator=g).to(dev)
        ra, rb = row_a.long(), row_b.long()
        lines.append(f"--- table {tname}: {na} sites x {C} channels, generated superset {nb}, union {nu}")
        lines.append(f"{'op':<22}{'pass':<9}{'HIP':>16}{'ATen':>16}{'speed-up':>10}{'GB/s':>9}{'share':>8}{'launches':>12}")

        def add_hip():
            return S.union_add(fa, fb, row_a, row_b, src_a, src_b)

        def add_aten():
            return torch.zeros((nu, C), dtype=torch.float32, device=dev).index_add_(0, ra, fa).index_add_(0, rb, fb)

        assert torch.equal(add_hip(), add_aten())

        def with_backward(fwd, leaves):
            def run():
                torch.autograd.grad(fwd(), leaves, dy_of[fwd])
            return run

        mask = (torch.rand(na, generator=g) < 0.5).to(dev)
        x = fa

        def prune_hip():
            kept, pos, _ = S.prune_map(mask, keys)
            return S.take_rows(x, kept, back=pos)

        def prune_aten():
            return x[mask]

        assert torch.equal(prune_hip(), prune_aten())
        nk = int(mask.sum())
        dyk = torch.randn(nk, C, generator=g).to(dev)
        dy_of = {add_hip: dy, add_aten: dy, prune_hip: dyk, prune_aten: dyk}

        def map_hip():
            return S.union_map(keys, gen)

        def map_aten():
            uu = torch.unique(torch.cat((keys, gen)))
            return uu, torch.searchsorted(uu, keys), torch.searchsorted(uu, gen), int(uu.shape[0])

        assert torch.equal(map_aten()[0], u) and torch.equal(map_aten()[1].int(), row_a)
        add_bytes = 4 * C * (na + nb + nu) + 8 * nu
        prune_bytes = 13 * na + 12 * nk + 8 * C * nk
        _, pos, _ = S.prune_map(mask, keys)
        xd = x.detach()

        def add_bwd_hip():  # the backward LAUNCHES on both arms (through autograd the engine's host time hides them)
            return S._take_rows(dy, row_a, 1), S._take_rows(dy, row_b, 1)

        def add_bwd_aten():
            return dy.index_select(0, ra), dy.index_select(0, rb)

        def prune_bwd_hip():
            return S._take_rows(dyk, pos, 1)

        def prune_bwd_aten():
            return torch.zeros_like(xd).index_put_((mask,), dyk)

        assert all(torch.equal(a, b) for a, b in zip(add_bwd_hip(), add_bwd_aten())) and torch.equal(prune_bwd_hip(), prune_bwd_aten())
        rows = [("union add", "fwd", add_hip, add_aten, add_bytes),
                ("union add", "bwd", add_bwd_hip, add_bwd_aten, add_bytes + 4 * (na + nb) - 8 * nu),
                ("union add", "fwd+bwd", with_backward(add_hip, (fa, fb)), with_backward(add_aten, (fa, fb)), 2 * add_bytes + 4 * (na + nb) - 8 * nu),
                ("union map", "", map_hip, map_aten, 8 * (na + nb + nu) + 4 * (na + nb + 2 * nu)),
                ("pruning", "fwd", prune_hip, prune_aten, prune_bytes),
                ("pruning", "bwd", prune_bwd_hip, prune_bwd_aten, 4 * C * (nk + na) + 4 * na),
                ("pruning", "fwd+bwd", with_backward(prune_hip, (x,)), with_backward(prune_aten, (x,)), prune_bytes + 4 * C * (nk + na) + 4 * na)]
        for op, pname, hip, aten, need in rows:
            t = timed({"hip": hip, "aten": aten}, args.iters, args.warmup)
            mh, mt = med(t["hip"]), med(t["aten"])
            gbs = need / (mh * 1e-3) / 1e9
            lines.append(f"{op:<22}{pname:<9}{mh:>9.4f} /{t['hip'][0]:>6.3f}{mt:>9.4f} /{t['aten'][0]:>6.3f}{mt / mh:>10.2f}{gbs:>9.0f}"
                         f"{gbs / HBM_PEAK_GBS * 100:>7.1f}%{launches(hip) + ' / ' + launches(aten):>12}")
            if mh > mt:
                slower.append(f"{tname} {op} {pname}".strip() + f" ({mh * 1e3:.1f} us against {mt * 1e3:.1f} us)")
    lines.append("HIP form slower than the ATen form: " + ("; ".join(slower) if slower else "nowhere"))

    # ---- the neck ----------------------------------------------------------------------------------------------------------------
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    from vdetr_amd.model_vdetr import build_vdetr, default_args
    g = torch.Generator().manual_seed(1)
    n = 40000
    uv = torch.rand((n, 2), generator=g)
    floor = torch.stack((uv[:, 0] * 7.6, uv[:, 1] * 6.0, torch.zeros(n)), 1)
    wall = torch.stack((uv[:, 0] * 7.6, torch.zeros(n), uv[:, 1] * 1.6), 1)
    inputs = {"point_clouds": [torch.cat((floor[: 3 * n // 4], wall[3 * n // 4:])).to(dev) + 1.0]}
    lines.append(f"--- neck: backbone_forward forward + backward (train mode, prepared geometry) of one {n}-point scene; median / min of "
                 f"{args.neck_iters} alternated calls (ms)")
    arms, levels = {}, {}
    for woexpand in (False, True):
        torch.manual_seed(0)
        model = build_vdetr(default_args(nqueries=32, dec_nlayers=2, preenc_npoints=256, woexpand_conv=woexpand), ScannetDatasetConfig(),
                            "minkowski").to(dev).train()
        geo = model.prepare_geometry(inputs)
        canonical = {ts: k.shape[0] for ts, k in geo.keys.items()}
        unions = [v[0].shape[0] for v in geo.__dict__.get("_union_maps", {}).values()]
        levels[woexpand] = (canonical, unions)

        def step(model=model, geo=geo):
            model.zero_grad(set_to_none=True)
            sum(f.square().sum() for _, f in model.backbone_forward(dict(inputs, geometry=geo))).backward()

        arms["generative" if not woexpand else "default"] = step
    t = timed(arms, args.neck_iters, 3)
    canonical, unions = levels[False]
    lines.append("sites per tensor stride, canonical (the default neck's levels): " + ", ".join(f"s{ts}: {canonical[ts]}" for ts in sorted(canonical)))
    lines.append("sites per level of the generative neck (union of skip and generated, nothing pruned): "
                 + ", ".join(f"s{ts}: {nu}" for ts, nu in zip((16, 8, 4), unions)))
    mg, md = med(t["generative"]), med(t["default"])
    lines.append(f"woexpand_conv False {mg:.3f} / {t['generative'][0]:.3f} ms    True {md:.3f} / {t['default'][0]:.3f} ms    ratio {mg / md:.2f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
