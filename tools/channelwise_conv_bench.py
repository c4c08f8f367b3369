#!/usr/bin/env python3
"""The channelwise convolution (csrc/sparse_cwconv.hip) against the two forms that were available before it, in ONE process, the
arms alternated call by call, median / min of the timed calls after a warm-up of all of them (device events around a whole call).

Tables: one scene's sites on a floor and a wall, [~35k, 64] at tensor stride 4 and [~5k, 256] at tensor stride 16; a cube 3 at
stride 1 and a cube 2 at stride 2.
Arms.  kernel: ``sparse_ops.channelwise_conv``.  dense: ``sparse_ops.sparse_conv`` (the pair path) with the kernel expanded to its
diagonal [K, C, C].  gather: ``gather_cols`` (writes the [nout, K, C] table) followed by ``(col * W).sum(1)`` in ATen; its backward
spreads dy over K, gathers it back with ``gather_sum`` and reduces col * dy over the rows.
Rows.  fwd: the forward alone.  fwd+bwd: forward and all gradients (kernel and dense through autograd, gather by hand).  dgrad /
wgrad: the backward launches of the kernel arm alone (through autograd the engine's host time hides them).
Needed bytes of a pass over the tables: 4 C (nin + nout) + 4 K nout + 4 K C; forward 1 pass, forward + backward 3; reported as
GB/s of the kernel arm and as a share of the HBM peak.

    python tools/channelwise_conv_bench.py [--out profiles/channelwise_conv_bench.txt]
"""
import argparse
import ctypes
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
        raise SystemExit("channelwise_conv_bench: needs a GPU (no number is produced without one)")
    from vdetr_amd import _lib as L
    from vdetr_amd import minkowski as ME
    from vdetr_amd import sparse_ops as S
    dev = torch.device("cuda:0")
    med = lambda v: v[len(v) // 2]  # noqa: E731
    lines = [f"channelwise convolution vs the dense diagonal kernel and the gather composition; median / min of {args.iters} alternated "
             f"calls (ms), each after an untimed call of its own arm, {torch.cuda.get_device_name(0)}",
             f"needed bytes per pass = 4 C (nin + nout) + 4 K nout + 4 K C (fwd 1 pass, fwd+bwd 3); share = of the "
             f"{HBM_PEAK_GBS / 1000:.0f} TB/s HBM peak"]
    tables = {"s4 C64": (plane_sites(190, 150, 40, 4, 0), 4, 64), "s16 C256": (plane_sites(70, 55, 16, 16, 1), 16, 256)}
    for tname, (sites, ts, C) in tables.items():
        keys = S.pack_keys(torch.from_numpy(sites).to(dev))
        cm = ME.CoordinateManager(dev)
        cm.keys[ts], cm.num_scenes = keys, 1
        g = torch.Generator().manual_seed(0)
        x = torch.randn(len(sites), C, generator=g).to(dev).requires_grad_(True)
        lines.append(f"--- table {tname}: {len(sites)} sites x {C} channels")
        lines.append(f"{'geometry':<12}{'pass':<9}{'kernel':>16}{'dense diag':>16}{'gather+ATen':>16}{'k vs dense':>11}{'k vs gather':>12}"
                     f"{'GB/s':>8}{'share':>8}{'launches k/d/g':>16}")
        for ks, stride in ((3, 1), (2, 2)):
            out_ts = ts * stride
            out_keys = keys if stride == 1 else cm.strided(keys, ts, out_ts)
            nbr, _, plan = cm.kernel_map(keys, out_keys, ts, out_ts, ks, False)
            _, inv = cm.pool_map(keys, out_keys, ts, out_ts, ks, False)
            K, nout, nin = nbr.shape[0], nbr.shape[1], len(sites)
            need = 4 * C * (nin + nout) + 4 * K * nout + 4 * K * C
            w = (torch.randn(K, C, generator=g) / (K * C) ** 0.5).to(dev).requires_grad_(True)
            b = torch.randn(C, generator=g).to(dev).requires_grad_(True)
            wd = torch.diag_embed(w.detach()).contiguous().requires_grad_(True)
            dy = torch.randn(nout, C, generator=g).to(dev)

            def k_fwd():
                return S.channelwise_conv(x, w, nbr, inv, b)

            def d_fwd():
                return S.sparse_conv(x, wd, nbr, inv, plan) + b

            def g_fwd():
                col = S.gather_cols(x.detach(), nbr)
                return (col * w.detach()).sum(1) + b.detach(), col

            def k_all():
                return torch.autograd.grad(k_fwd(), (x, w, b), dy)

            def d_all():
                return torch.autograd.grad(d_fwd(), (x, wd, b), dy)

            def g_all():
                _, col = g_fwd()
                spread = dy[:, None, :]
                return S.gather_sum((spread * w.detach()).contiguous(), inv), (col * spread).sum(0), dy.sum(0)

            yk, yd, yg = k_fwd().detach(), d_fwd().detach(), g_fwd()[0]
            scale = float(yk.abs().max())
            assert float((yk - yg).abs().max()) <= 1e-4 * scale
            gk, gd, gg = k_all(), d_all(), g_all()
            for a, c in zip(gk, gg):
                assert float((a - c).abs().max()) <= 1e-4 * float(c.abs().max()) + 1e-6
            # (the dense arm multiplies split-bf16 operands where C is a multiple of 64: its distance is reported, not judged)
            dense_gap = max(float((yk - yd).abs().max()) / scale, float((gk[0] - gd[0]).abs().max()) / float(gk[0].abs().max()),
                            float((gk[1] - torch.diagonal(gd[1], dim1=1, dim2=2)).abs().max()) / float(gk[1].abs().max()))

            d = L.SpCwConvDesc()
            d.K, d.nout, d.nin, d.C = K, nout, nin, C
            ws = L.workspace(L.lib().vdetr_sp_cwconv_workspace_bytes(K, nout, C), dev)
            d.x, d.nbr, d.w, d.workspace = x.data_ptr(), nbr.data_ptr(), w.data_ptr(), ws.data_ptr()
            dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)

            def k_dgrad():
                L.check(L.lib().vdetr_sp_cwconv_dgrad_f32(ctypes.byref(d), L.ptr(inv), L.ptr(dy), L.ptr(dx), L.stream_ptr()), "dgrad")

            def k_wgrad():
                L.check(L.lib().vdetr_sp_cwconv_wgrad_f32(ctypes.byref(d), L.ptr(dy), L.ptr(dw), L.ptr(db), L.stream_ptr()), "wgrad")

            k_dgrad(), k_wgrad()
            assert torch.equal(dx, gk[0]) and torch.equal(dw, gk[1]) and torch.equal(db, gk[2])
            geo = f"cube{ks}/s{stride}"
            for pname, passes, arms in (("fwd", 1, {"kernel": k_fwd, "dense": d_fwd, "gather": g_fwd}),
                                        ("fwd+bwd", 3, {"kernel": k_all, "dense": d_all, "gather": g_all})):
                t = timed(arms, args.iters, args.warmup)
                mk, md, mg = (med(t[a]) for a in ("kernel", "dense", "gather"))
                gbs = passes * need / (mk * 1e-3) / 1e9
                lines.append(f"{geo:<12}{pname:<9}" + "".join(f"{med(t[a]):>9.4f} /{t[a][0]:>6.3f}" for a in ("kernel", "dense", "gather")) +
                             f"{md / mk:>11.2f}{mg / mk:>12.2f}{gbs:>8.0f}{gbs / HBM_PEAK_GBS * 100:>7.1f}%"
                             f"{' / '.join(launches(arms[a]) for a in ('kernel', 'dense', 'gather')):>16}")
            t = timed({"dgrad": k_dgrad, "wgrad": k_wgrad}, args.iters, args.warmup)
            chunks = -(-nout // S.cwconv_chunk_rows(nout))
            for pname in ("dgrad", "wgrad"):
                mk = med(t[pname])
                gbs = need / (mk * 1e-3) / 1e9
                note = (f"   {chunks} chunks, partials {chunks * (K + 1) * C * 4 / 1e6:.2f} MB" if pname == "wgrad" else
                        f"   largest relative distance kernel - dense (y, dx, dW): {dense_gap:.1e}")
                lines.append(f"{geo:<12}{pname:<9}{mk:>9.4f} /{t[pname][0]:>6.3f}{'':>32}{'':>23}{gbs:>8.0f}{gbs / HBM_PEAK_GBS * 100:>7.1f}%{note}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
