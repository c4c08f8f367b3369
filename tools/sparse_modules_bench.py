#!/usr/bin/env python3
"""Sparse pooling (csrc/sparse_pool.hip) and InstanceNorm (csrc/sp_inorm.hip) against the compositions that were available before
them, in ONE process, the arms alternated call by call, median / min of the timed calls after a warm-up of all of them (device
events around a whole call).

Tables: one scene's sites on a floor and a wall, [~36k, 64] at tensor stride 4 and [~5k, 256] at tensor stride 16.
Pooling: forward and backward of cube 2 / stride 2 and cube 3 / stride 1 in the three modes.  Composition: ``gather_cols`` (writes the
[nout, K, C] table) followed by sum / amax over K; its backward spreads dy over K and gathers it back with ``gather_sum``.  The
backward rows time the backward LAUNCH on both arms (through autograd the engine's host time, about 0.1 ms, hides it).  Reported
with the bytes the operation NEEDS, 4 C (nin + nout) + 4 K nout, over the time, as GB/s and as a share of the HBM peak: these are
bandwidth-bound kernels.
InstanceNorm: forward and backward against the tensor-expression composition MinkowskiInstanceNorm.forward held before (it reads
the scene count back in the middle of the forward).  The composition runs as two arms; the distance between their medians is the
run-to-run spread the verdict is judged against.
Launches per call are counted with torch.profiler (``not measured`` when it is unavailable).

    python tools/sparse_modules_bench.py [--out profiles/sparse_modules_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s


def plane_sites(nx, ny, nz, ts, seed):
    """a floor nx x ny and a wall nx x nz of cells of size ts, 3 % of them missing: [N, 4] sorted"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    floor = np.stack((x.ravel(), y.ravel(), np.zeros(x.size, np.int64)), 1)
    x, z = np.meshgrid(np.arange(nx), np.arange(1, nz + 1), indexing="ij")
    wall = np.stack((x.ravel(), np.zeros(x.size, np.int64), z.ravel()), 1)
    c = np.concatenate((floor, wall)) * ts
    c = c[rng.random(len(c)) > 0.03]
    return np.unique(np.concatenate((np.zeros((len(c), 1), np.int64), c), 1), axis=0)


def timed(arms, iters, warmup):
    """arms: {name: callable}; -> {name: sorted times in ms}"""
    times = {k: [] for k in arms}
    for it in range(warmup + iters):
        for name, fn in arms.items():
            fn()  # not timed: the timed call starts from the state this arm leaves
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return {k: sorted(v) for k, v in times.items()}


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return str(sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA))
    except Exception:  # noqa: BLE001
        return "not measured"


def old_instance_norm(feats, keys, weight, bias, eps):
    """the composition MinkowskiInstanceNorm.forward held before csrc/sp_inorm.hip"""
    b = keys >> 48
    nb = int(b.max()) + 1
    cnt = torch.bincount(b, minlength=nb).clamp(min=1).to(feats.dtype)[:, None]
    mean = torch.zeros((nb, feats.shape[1]), dtype=feats.dtype, device=feats.device).index_add_(0, b, feats) / cnt
    d = feats - mean[b]
    var = torch.zeros_like(mean).index_add_(0, b, d * d) / cnt
    return d / torch.sqrt(var[b] + eps) * weight + bias


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_modules_bench: needs a GPU (no number is produced without one)")
    from vdetr_amd import minkowski as ME
    from vdetr_amd import sparse_ops as S
    dev = torch.device("cuda:0")
    med = lambda v: v[len(v) // 2]  # noqa: E731
    lines = [f"sparse pooling and InstanceNorm vs the earlier compositions; median / min of {args.iters} alternated calls (ms), each after an "
             f"untimed call of its own arm, {torch.cuda.get_device_name(0)}",
             f"needed bytes = 4 C (nin + nout) + 4 K nout; share = of the {HBM_PEAK_GBS / 1000:.0f} TB/s HBM peak (bandwidth-bound)"]
    tables = {"s4 C64": (plane_sites(190, 150, 40, 4, 0), 4, 64), "s16 C256": (plane_sites(70, 55, 16, 16, 1), 16, 256)}
    verdicts = []
    for tname, (sites, ts, C) in tables.items():
        coords = torch.from_numpy(sites).to(dev)
        keys = S.pack_keys(coords)
        cm = ME.CoordinateManager(dev)
        cm.keys[ts], cm.num_scenes = keys, 1
        g = torch.Generator().manual_seed(0)
        x = torch.randn(len(sites), C, generator=g).to(dev)
        lines.append(f"--- table {tname}: {len(sites)} sites x {C} channels")
        lines.append(f"{'pooling':<22}{'pass':<6}{'kernel':>16}{'composition':>16}{'speed-up':>10}{'GB/s':>9}{'share':>8}{'launches k/c':>14}")
        for ks, stride in ((2, 2), (3, 1)):
            out_ts = ts * stride
            out_keys = keys if stride == 1 else cm.strided(keys, ts, out_ts)
            nbr, inv = cm.pool_map(keys, out_keys, ts, out_ts, ks, False)
            K, nout, nin = nbr.shape[0], nbr.shape[1], len(sites)
            need = 4 * C * (nin + nout) + 4 * K * nout
            dy = torch.randn(nout, C, generator=g).to(dev)
            for mode in ("sum", "avg", "max"):
                y, inv_count, arg = S.sparse_pool(x, nbr, inv, mode, return_aux=True)
                cfg = (K, nout, nin, C, S.POOL_MODES[mode])

                def comp_fwd():
                    col = S.gather_cols(x, nbr)
                    if mode == "max":
                        return torch.where((nbr >= 0).t()[:, :, None], col, torch.full_like(col, -float("inf"))).amax(1), col
                    s = col.sum(1)
                    return (s / (nbr >= 0).sum(0).clamp(min=1)[:, None] if mode == "avg" else s), col

                yc, col = comp_fwd()
                ok = torch.isfinite(yc).all(1)
                assert float((y.detach()[ok] - yc[ok]).abs().max()) <= 1e-4 * float(yc[ok].abs().max())

                def comp_bwd():
                    d = dy[:, None, :].expand(-1, K, -1)
                    if mode == "max":
                        d = d * (col == yc[:, None, :])
                    elif mode == "avg":
                        d = d / (nbr >= 0).sum(0).clamp(min=1)[:, None, None]
                    return S.gather_sum(d.contiguous(), inv)

                def kern_bwd():  # the backward launch itself (through autograd the engine's ~0.1 ms of host time hides it)
                    return S._sparse_pool_backward(dy, inv, cfg, inv_count, arg)

                assert float((kern_bwd() - comp_bwd()).abs().max()) <= 1e-4 * float(dy.abs().max()) * K or mode == "max"

                for pname, kern, comp in (("fwd", lambda: S.sparse_pool(x, nbr, inv, mode), comp_fwd), ("bwd", kern_bwd, comp_bwd)):
                    t = timed({"kernel": kern, "composition": comp}, args.iters, args.warmup)
                    mk, mc = med(t["kernel"]), med(t["composition"])
                    gbs = need / (mk * 1e-3) / 1e9
                    lines.append(f"{f'cube{ks}/s{stride} {mode}':<22}{pname:<6}{mk:>9.4f} /{t['kernel'][0]:>6.3f}{mc:>9.4f} /{t['composition'][0]:>6.3f}"
                                 f"{mc / mk:>10.2f}{gbs:>9.0f}{gbs / HBM_PEAK_GBS * 100:>7.1f}%{launches(kern) + ' / ' + launches(comp):>14}")
        # InstanceNorm
        norm = ME.MinkowskiInstanceNorm(C).to(dev)
        seg, nseg = cm.scene_segments(keys)
        dyn = torch.randn(len(sites), C, generator=g).to(dev)
        xr = x.clone().requires_grad_(True)

        def new_fwd():
            return S.instance_norm(xr, seg, nseg, norm.weight, norm.bias, norm.eps)

        def old_fwd():
            return old_instance_norm(xr, keys, norm.weight, norm.bias, norm.eps)

        def fb(fwd):
            def run():
                y = fwd()
                torch.autograd.grad(y, (xr, norm.weight, norm.bias), dyn)
            return run

        assert float((new_fwd() - old_fwd()).detach().abs().max()) < 1e-3
        lines.append(f"{'InstanceNorm':<22}{'':<6}{'kernels':>16}{'composition':>16}{'speed-up':>10}{'spread':>9}{'launches k/c':>16}")
        for pname, new, old in (("fwd", lambda: new_fwd(), lambda: old_fwd()), ("fwd+bwd", fb(new_fwd), fb(old_fwd))):
            t = timed({"kernel": new, "composition": old, "composition'": old}, args.iters, args.warmup)
            mk, mc, mc2 = med(t["kernel"]), med(t["composition"]), med(t["composition'"])
            spread = abs(mc - mc2) / mc2
            lines.append(f"{'':<22}{pname:<8}{mk:>7.4f} /{t['kernel'][0]:>6.3f}{mc:>9.4f} /{t['composition'][0]:>6.3f}{mc / mk:>10.2f}"
                         f"{spread * 100:>8.1f}%{launches(new) + ' / ' + launches(old):>16}")
            verdicts.append((f"{tname} {pname}", mk <= min(mc, mc2) * (1 + spread)))
    lines.append("InstanceNorm not slower than the composition by more than the spread: " + ", ".join(f"{n}: {'yes' if ok else 'NO'}" for n, ok in verdicts))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
