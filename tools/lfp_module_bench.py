#!/usr/bin/env python3
"""Eval forward of PointnetLFPModuleMSG: the fused launches (csrc/group_mlp.hip: one set-abstraction launch per scale and one
post-MLP launch per four scales) against the composition of ops, in ONE process, the arms alternated call by call, median / min of
30 timed calls each after a warm-up of all of them (device events around a whole call, ball queries included in every arm).  The
arms' outputs are compared on the same inputs before anything is timed.

Every timed call follows an untimed, synchronised call of the SAME arm.  Without it the order of the arms decides the result: the
call that follows the composition (its grouped [B, 3 + C, N2, nsample] tensors pass through the caches) took 35 to 45 us longer
than the same call after a fused one, whichever arm it was, which is more than the difference that is to be measured.  A model
runs one form call after call, so each arm is timed from the state its own last call left.

Arms: `fused` (everything the gates allow), `sa only` (the fused set-abstraction launches, the post MLP as the composition: the
difference to `fused` is what the post-MLP launch alone buys), `composition` (``FUSED = False``) twice — the distance between its
two medians is the run-to-run spread the verdict line is judged against.

Shapes (B = 1, 1024 points with 256 channels propagated to 2048 points with 128 channels):
(a) radii [0.4], nsamples [32], mlps [[256, 128, 128]], post_mlp [256, 256];
(b) radii [0.2, 0.4], nsamples [16, 32], mlps [[256, 128, 128]] x 2, post_mlp [256, 128].

    python tools/lfp_module_bench.py [--shape a|b|all] [--out profiles/lfp_module_bench.txt] [--append]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "a": dict(radii=[0.4], nsamples=[32], mlps=[[256, 128, 128]], post_mlp=[256, 256]),
    "b": dict(radii=[0.2, 0.4], nsamples=[16, 32], mlps=[[256, 128, 128], [256, 128, 128]], post_mlp=[256, 128]),
}
ARMS = ("fused", "sa only", "composition", "composition'")


def build_case(shape, dev, batch):
    from vdetr_amd import pointnet2_modules as PM
    g = torch.Generator().manual_seed(0)
    room = torch.tensor([8.0, 6.0, 3.0])
    xyz1 = (torch.rand(batch, 1024, 3, generator=g) * room).to(dev)
    xyz2 = (torch.rand(batch, 2048, 3, generator=g) * room).to(dev)
    f1, f2 = torch.randn(batch, 256, 1024, generator=g).to(dev), torch.randn(batch, 128, 2048, generator=g).to(dev)
    mod = PM.PointnetLFPModuleMSG(**SHAPES[shape]).to(dev).eval()
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():  # BatchNorm that is no identity fold
        for bn in mod.modules():
            if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
                bn.weight.copy_(torch.randn(bn.weight.shape, generator=gen))
                bn.bias.copy_(torch.randn(bn.bias.shape, generator=gen) * 0.5)
                bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=gen) * 0.5)
                bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=gen) + 0.5)
    return mod, (xyz2, xyz1, f2, f1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["a", "b", "all"])
    ap.add_argument("--out", default="")
    ap.add_argument("--append", action="store_true", help="add the rows to --out instead of starting it (one shape per process)")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lfp_module_bench: needs a GPU (no number is produced without one)")
    from vdetr_amd import pointnet2_modules as PM
    dev = torch.device("cuda:0")
    post_gate = PM._post_fusable
    lines = []
    if not args.append:
        lines += [f"eval forward of PointnetLFPModuleMSG, fused launches vs composition of ops; batch {args.batch}, median / min of {args.iters} "
                  f"alternated calls (ms), each after an untimed call of its own arm, {torch.cuda.get_device_name(0)}",
                  "sa only = fused set-abstraction launches, post MLP as the composition; spread = |median A - median B| / median B with the "
                  "composition on both arms",
                  f"{'shape':<10}{'fused':>16}{'sa only':>16}{'composition':>16}{'vs comp.':>10}{'vs sa only':>12}{'spread':>8}{'launches':>10}"
                  f"{'max rel diff':>14}"]

    def call(mod, inputs, arm):
        PM.FUSED = not arm.startswith("composition")
        PM._post_fusable = (lambda *a: None) if arm == "sa only" else post_gate
        with torch.no_grad():
            out = mod(*inputs)
        nscales = len(mod.groupers)
        want = {"fused": ["fused"] * (nscales + 1), "sa only": ["fused"] * nscales + ["composition"]}.get(arm, ["composition"] * (nscales + 1))
        assert mod.last_paths == want, (arm, mod.last_paths)
        return out

    verdicts = []
    try:
        for shape in (("a", "b") if args.shape == "all" else (args.shape,)):
            mod, inputs = build_case(shape, dev, args.batch)
            n0 = PM.FUSED_LAUNCHES
            outs = {arm: call(mod, inputs, arm) for arm in ARMS[:3]}
            launches = PM.FUSED_LAUNCHES - n0 - len(mod.groupers)  # of the `fused` arm alone
            scale = outs["composition"].abs().max()
            diff = max(((outs[arm] - outs["composition"]).abs().max() / scale).item() for arm in ("fused", "sa only"))
            assert diff < 1e-4, diff
            times = {arm: [] for arm in ARMS}
            for it in range(args.warmup + args.iters):
                for arm in ARMS:
                    call(mod, inputs, arm)  # not timed: the timed call starts from the state this arm leaves
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call(mod, inputs, arm)
                    e1.record()
                    e1.synchronize()
                    if it >= args.warmup:
                        times[arm].append(e0.elapsed_time(e1))
            t = {k: sorted(v) for k, v in times.items()}
            med = {k: v[len(v) // 2] for k, v in t.items()}
            spread = abs(med["composition"] - med["composition'"]) / med["composition'"]
            lines.append(f"{shape:<10}" + "".join(f"{med[arm]:>9.4f} /{t[arm][0]:>6.3f}" for arm in ARMS[:3])
                         + f"{med['composition'] / med['fused']:>10.2f}{med['sa only'] / med['fused']:>12.2f}{spread * 100:>7.1f}%{launches:>10d}{diff:>14.2e}")
            verdicts.append((shape, med["fused"] <= med["sa only"] * (1 + spread)))
    finally:
        PM.FUSED, PM._post_fusable = True, post_gate
    lines.append("fused post MLP not slower than `sa only` by more than the spread: " + ", ".join(f"{n}: {'yes' if ok else 'NO'}" for n, ok in verdicts))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a" if args.append else "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
