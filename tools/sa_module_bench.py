#!/usr/bin/env python3
"""Eval forward of the PointNet++ layers: the fused launch (csrc/group_mlp.hip) against the composition of ops, in ONE process,
the two forms alternated call by call, median of 30 timed calls each after a warm-up of both (device events around each call).
What is timed is the layer after the centres are known: ball query + (gather, MLP, max) for the set abstractions (``inds`` given, so
furthest point sampling is outside both forms), three_nn + weights + (interpolation, concatenation, MLP) for the feature
propagation.  The two forms' outputs are compared on the same inputs before anything is timed.

Shapes: (a) the 3DETR pre-encoder on bench.py's synthetic 40 k-point scene (2048 centres, r = 0.2, 64 neighbours, no features,
3 -> 64 -> 128 -> 256, normalize_xyz); (b) VoteNet SA2 (2048 -> 1024 points, r = 0.4, 32 neighbours, 128 channels,
-> 128 -> 128 -> 256); (c) VoteNet FP (1024 unknown, 512 known points, 256 + 256 channels, -> 256 -> 256).

    python tools/sa_module_bench.py [--out profiles/sa_module_bench.txt] [--batch 1]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def flops(rows, widths):
    return 2 * rows * sum(a * b for a, b in zip(widths[:-1], widths[1:]))


def build_cases(dev, batch):
    import bench
    from vdetr_amd import pointnet2_modules as PM
    from vdetr_amd import pointnet2_utils as PU
    g = torch.Generator().manual_seed(0)
    cases = []
    xyz, _ = bench.make_scene(40000, 0, dev)
    xyz = xyz[None].repeat(batch, 1, 1).contiguous()
    m = PM.PointnetSAModuleVotes(mlp=[0, 64, 128, 256], npoint=2048, radius=0.2, nsample=64, normalize_xyz=True).to(dev).eval()
    inds = PU.furthest_point_sample(xyz, 2048)
    cases.append(("a: 3DETR pre-encoder", m, (xyz, None, inds), flops(batch * 2048 * 64, [3, 64, 128, 256])))
    xyz2 = (torch.rand(batch, 2048, 3, generator=g) * torch.tensor([8.0, 6.0, 3.0])).to(dev)
    f2 = torch.randn(batch, 128, 2048, generator=g).to(dev)
    m = PM.PointnetSAModuleVotes(mlp=[128, 128, 128, 256], npoint=1024, radius=0.4, nsample=32, normalize_xyz=True).to(dev).eval()
    inds = PU.furthest_point_sample(xyz2, 1024)
    cases.append(("b: VoteNet SA2", m, (xyz2, f2, inds), flops(batch * 1024 * 32, [131, 128, 128, 256])))
    unknown, known = xyz2[:, :1024].contiguous(), xyz2[:, 1024:1536].contiguous()
    uf, kf = torch.randn(batch, 256, 1024, generator=g).to(dev), torch.randn(batch, 256, 512, generator=g).to(dev)
    m = PM.PointnetFPModule(mlp=[512, 256, 256]).to(dev).eval()
    cases.append(("c: VoteNet FP", m, (unknown, known, uf, kf), flops(batch * 1024, [512, 256, 256])))
    gen = torch.Generator().manual_seed(1)
    for _, mod, _, _ in cases:  # BatchNorm that is no identity fold
        with torch.no_grad():
            for bn in mod.modules():
                if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
                    bn.weight.copy_(torch.randn(bn.weight.shape, generator=gen))
                    bn.bias.copy_(torch.randn(bn.bias.shape, generator=gen) * 0.5)
                    bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=gen) * 0.5)
                    bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=gen) + 0.5)
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sa_module_bench: needs a GPU (no number is produced without one)")
    from vdetr_amd import pointnet2_modules as PM
    dev = torch.device("cuda:0")
    lines = [f"eval forward, fused launch vs composition of ops; batch {args.batch}, median / min of {args.iters} alternated calls (ms), "
             f"{torch.cuda.get_device_name(0)}",
             f"{'shape':<24}{'fused':>16}{'composition':>18}{'speed-up':>10}{'fused TFLOP/s':>15}{'max rel diff':>14}"]

    def call(mod, inputs, fused):
        PM.FUSED = fused
        with torch.no_grad():
            out = mod(*inputs)
        assert mod.last_paths == ["fused" if fused else "composition"], mod.last_paths
        return out[1] if isinstance(out, tuple) else out

    for name, mod, inputs, fl in build_cases(dev, args.batch):
        a, b = call(mod, inputs, True), call(mod, inputs, False)
        diff = ((a - b).abs().max() / b.abs().max()).item()
        times = {True: [], False: []}
        for it in range(args.warmup + args.iters):
            for fused in (True, False):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(mod, inputs, fused)
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    times[fused].append(e0.elapsed_time(e1))
        t = {k: sorted(v) for k, v in times.items()}
        med = {k: v[len(v) // 2] for k, v in t.items()}
        lines.append(f"{name:<24}{med[True]:>9.4f} /{t[True][0]:>6.3f}{med[False]:>11.4f} /{t[False][0]:>6.3f}{med[False] / med[True]:>10.2f}"
                     f"{fl / med[True] / 1e9:>15.2f}{diff:>14.2e}")
    PM.FUSED = True
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
