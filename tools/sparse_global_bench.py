#!/usr/bin/env python3
"""Global pooling, broadcast and the squeeze-excite layer (csrc/sparse_global.hip) against the ATen compositions a user would
write without them, in ONE process, the arms alternated call by call, median / min of the timed calls after a warm-up of all of
them (device events around a whole call).  The conventions are tools/sparse_modules_bench.py's.

Tables: [~36k, 64] (tensor stride 4) and [~5k, 256] (tensor stride 16) as one scene and cut into four scenes of unequal size.
  pooling    forward, and forward + backward through autograd, in the three modes; composition: ``index_add_`` (sum, avg) /
             ``scatter_reduce(amax)`` over a batch-index column built beforehand (float atomics: not reproducible run to run)
  broadcast  multiply, forward and forward + backward; composition: ``x * g[batch_index]`` through autograd
  SE         ``sparse_ops.se_scale`` (three launches) against the module's composition (pooling, two linears with ReLU and sigmoid
             in ATen, broadcast multiply), plain and with the SE block's tail (residual add and ReLU), under no_grad
The composition runs as two arms; the distance between their medians is the run-to-run spread a verdict is judged against.
Needed bytes over time is reported as GB/s and as a share of the HBM peak.  Launches per call are counted with torch.profiler
(``not measured`` when it is unavailable).  No speed-up is promised: the rows say what was measured.

    python tools/sparse_global_bench.py [--out profiles/sparse_global_bench.txt]
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_global_bench: needs a GPU (no number is produced without one)")
    from vdetr_amd import sparse_ops as S
    dev = torch.device("cuda:0")
    med = lambda v: v[len(v) // 2]  # noqa: E731
    lines = [f"global pooling, broadcast and squeeze-excite vs ATen compositions; median / min of {args.iters} alternated calls (ms), each "
             f"after an untimed call of its own arm, {torch.cuda.get_device_name(0)}",
             f"share = needed bytes over time, of the {HBM_PEAK_GBS / 1000:.0f} TB/s HBM peak; spread = distance of the two composition arms' medians",
             f"{'row':<30}{'kernel':>16}{'composition':>16}{'speed-up':>10}{'spread':>8}{'GB/s':>8}{'share':>8}{'launches k/c':>14}{'  not slower':>12}"]
    rows = {"s4 C64": (len(plane_sites(190, 150, 40, 4, 0)), 64), "s16 C256": (len(plane_sites(70, 55, 16, 16, 1)), 256)}

    def report(name, kern, comp, need):
        t = timed({"kernel": kern, "composition": comp, "composition'": comp}, args.iters, args.warmup)
        mk, mc, mc2 = med(t["kernel"]), med(t["composition"]), med(t["composition'"])
        spread = abs(mc - mc2) / mc2
        gbs = need / (mk * 1e-3) / 1e9
        ok = mk <= min(mc, mc2) * (1 + spread)
        lines.append(f"{name:<30}{mk:>9.4f} /{t['kernel'][0]:>6.3f}{mc:>9.4f} /{t['composition'][0]:>6.3f}{mc / mk:>10.2f}{spread * 100:>7.1f}%"
                     f"{gbs:>8.0f}{gbs / HBM_PEAK_GBS * 100:>7.1f}%{launches(kern) + ' / ' + launches(comp):>14}{'yes' if ok else 'NO':>12}")

    for tname, (N, C) in rows.items():
        for nseg in (1, 4):
            cuts = [0, N] if nseg == 1 else [0, N // 8, N // 2, N - N // 5, N]
            seg = torch.tensor(cuts, dtype=torch.int32, device=dev)
            bidx = torch.repeat_interleave(torch.arange(nseg, device=dev), (seg[1:] - seg[:-1]).long())
            counts = (seg[1:] - seg[:-1]).float()[:, None]
            gen = torch.Generator().manual_seed(0)
            x = torch.randn(N, C, generator=gen).to(dev)
            xr = x.clone().requires_grad_(True)
            dyp, dyn = torch.randn(nseg, C, generator=gen).to(dev), torch.randn(N, C, generator=gen).to(dev)
            lines.append(f"--- table {tname}: {N} rows x {C} channels, {nseg} scene{'s' if nseg > 1 else ''}")
            col = bidx[:, None].expand(N, C)
            for mode in ("sum", "avg", "max"):
                def comp(t=xr, mode=mode):
                    if mode == "max":
                        return torch.zeros((nseg, C), device=dev).scatter_reduce(0, col, t, "amax", include_self=False)
                    y = torch.zeros((nseg, C), device=dev).index_add(0, bidx, t)
                    return y / counts if mode == "avg" else y

                def kern(t=xr, mode=mode):
                    return S.global_pool(t, seg, nseg, mode)

                assert float((kern(x) - comp(x)).abs().max()) <= 1e-3 * float(comp(x).abs().max())
                report(f"pool {mode} fwd", lambda: kern(x), lambda: comp(x), 4 * C * (N + nseg))
                report(f"pool {mode} fwd+bwd", lambda: torch.autograd.grad(kern(), xr, dyp), lambda: torch.autograd.grad(comp(), xr, dyp),
                       4 * C * (2 * N + 2 * nseg))
            g = torch.rand(nseg, C, generator=gen).to(dev)
            gr = g.clone().requires_grad_(True)
            assert torch.equal(S.broadcast(x, g, seg, nseg, "mul"), x * g[bidx])
            report("broadcast mul fwd", lambda: S.broadcast(x, g, seg, nseg, "mul"), lambda: x * g[bidx], 8 * C * N)
            report("broadcast mul fwd+bwd", lambda: torch.autograd.grad(S.broadcast(xr, gr, seg, nseg, "mul"), (xr, gr), dyn),
                   lambda: torch.autograd.grad(xr * gr[bidx], (xr, gr), dyn), 20 * C * N)
            H = C // 16
            w1, b1 = (torch.randn(H, C, generator=gen) / C ** 0.5).to(dev), torch.randn(H, generator=gen).to(dev)
            w2, b2 = (torch.randn(C, H, generator=gen) / H ** 0.5).to(dev), torch.randn(C, generator=gen).to(dev)
            res = torch.randn(N, C, generator=gen).to(dev)

            def se_comp(residual=None, relu=False):
                p = S.global_pool(x, seg, nseg, "avg")
                gate = torch.sigmoid(torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(p, w1, b1)), w2, b2))
                y = S.broadcast(x, gate, seg, nseg, "mul")
                if residual is not None:
                    y = y + residual
                return torch.relu(y) if relu else y

            with torch.no_grad():
                a, b = S.se_scale(x, seg, nseg, w1, b1, w2, b2, res, True), se_comp(res, True)
                assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
                report("SELayer (no_grad)", lambda: S.se_scale(x, seg, nseg, w1, b1, w2, b2), se_comp, 12 * C * N)
                report("SE block tail (no_grad)", lambda: S.se_scale(x, seg, nseg, w1, b1, w2, b2, res, True), lambda: se_comp(res, True),
                       16 * C * N)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
