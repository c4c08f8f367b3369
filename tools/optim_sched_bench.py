#!/usr/bin/env python3
"""Times the two AdamW entry points (csrc/optim.hip) on flat buffers of the sizes bench.py trains: the C2 decoder's FlatParams and
the with-backbone model's.  The yardstick is vdetr_adamw_clip_f32, the launch bench.py issues, measured in the same run; next to it
vdetr_adamw_sched_f32 with neither option (null table, null mask), and with a ScanNet-sized rate table plus the --filter_biases_wd
mask of the model's own parameters.  Every variant clips (partial sums as the pack leaves them), as bench.py's step does.

Method: after a warm-up, ROUNDS rounds; each round times LAUNCHES back-to-back launches of every variant between two device events,
the variants in rotating order.  Reported per variant: the median, the fastest and the slowest round in microseconds per launch, and
the spread (slowest - fastest) / median; for the new entry the difference of the medians to the yardstick, to be read against the
yardstick's own spread.  Needs a GPU: there is no fallback.

    python tools/optim_sched_bench.py [--out profiles/optim_sched_bench.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, LAUNCHES, WARMUP = 15, 200, 50
TABLE_ENTRIES = 540 * 150  # main.py:177 epochs x ~150 iterations (1201 ScanNet training scans, global batch 8)


def flat_of(kind, device):
    """FlatParams of the model bench.py builds for its decoder step ("decoder": config c2) or for its with-backbone step"""
    import bench
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    from vdetr_amd.dist import FlatParams
    from vdetr_amd.model_vdetr import build_vdetr, default_args
    if kind == "decoder":
        model = bench.build_model("c2", device)
    else:
        _, _, npre, nq, nl, angle_type, _ = bench.CONFIGS["c2"]
        model = build_vdetr(default_args(dec_nlayers=nl, nqueries=nq, preenc_npoints=npre, angle_type=angle_type), ScannetDatasetConfig(),
                            "minkowski").to(device).train()
    flat = FlatParams([p for p in model.parameters() if p.requires_grad], groups=model.flat_param_groups())
    return flat, flat.decay_mask(model.named_parameters())


def measure(n, mask, device, log):
    from vdetr_amd import _lib as L
    lib = L.lib()
    gen = torch.Generator(device=device).manual_seed(0)
    p, g = torch.randn(n, device=device, generator=gen) * 0.02, torch.randn(n, device=device, generator=gen) * 1e-3
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    nsum = lib.vdetr_sumsq_blocks(n)
    partial = torch.empty(nsum, device=device)
    L.check(lib.vdetr_sumsq_f32(g.data_ptr(), n, partial.data_ptr(), nsum, L.stream_ptr()), "sumsq")
    step, ticket = torch.zeros((), device=device), torch.zeros(4, dtype=torch.int32, device=device)
    norm, lr_out = torch.zeros((), device=device), torch.zeros((), dtype=torch.float64, device=device)
    table = torch.from_numpy(np.linspace(7e-4, 1e-6, TABLE_ENTRIES)).to(device)

    def desc(cls):
        d = cls()
        d.param, d.grad, d.exp_avg, d.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
        d.n, d.step, d.ticket = n, step.data_ptr(), ticket.data_ptr()
        d.sumsq, d.nsumsq, d.max_norm, d.norm_eps, d.norm_out = partial.data_ptr(), nsum, 0.1, 1e-6, norm.data_ptr()
        d.lr, d.beta1, d.beta2, d.eps, d.weight_decay = 7e-4, 0.9, 0.999, 1e-8, 0.1
        return d

    old, bare, full = desc(L.AdamWDesc), desc(L.AdamWSchedDesc), desc(L.AdamWSchedDesc)
    bare.lr_out = full.lr_out = lr_out.data_ptr()
    full.lr_table, full.n_lr, full.decay_mask = table.data_ptr(), table.numel(), mask.data_ptr()
    variants = [("adamw_clip (yardstick)", lib.vdetr_adamw_clip_f32, old), ("adamw_sched, no table, no mask", lib.vdetr_adamw_sched_f32, bare),
                ("adamw_sched, table + mask", lib.vdetr_adamw_sched_f32, full)]
    stream = L.stream_ptr()

    def run(fn, d, k):
        for _ in range(k):
            status = fn(ctypes.byref(d), stream)
            if status != 0:
                raise RuntimeError(lib.vdetr_last_error().decode())

    for _, fn, d in variants:
        run(fn, d, WARMUP)
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for r in range(ROUNDS):
        for k in range(len(variants)):
            name, fn, d = variants[(r + k) % len(variants)]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(fn, d, LAUNCHES)
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / LAUNCHES)
    if not bool(torch.isfinite(p).all()):
        raise RuntimeError("the timed updates left non-finite parameters")
    base = statistics.median(times[variants[0][0]])
    for name, _, _ in variants:
        t = times[name]
        med = statistics.median(t)
        log(f"  {name:32s} median {med:8.2f} us  fastest {min(t):8.2f}  slowest {max(t):8.2f}  spread {(max(t) - min(t)) / med * 100:5.2f} %"
            f"  vs yardstick {(med - base) / base * 100:+6.2f} %  ({28 * n / med * 1e-3:6.0f} GB/s of p, g, m, v)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_sched_bench: needs a GPU")
    device = torch.device("cuda:0")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"{torch.cuda.get_device_name(0)}; {ROUNDS} rounds x {LAUNCHES} launches per variant, rotating order, {WARMUP} warm-up launches each; "
        f"rate table of {TABLE_ENTRIES} doubles")
    for kind in ("decoder", "with backbone"):
        flat, mask = flat_of(kind, device)
        n = flat.data.numel()
        set_bits = int(sum(bin(int(w) & 0xFFFFFFFF).count("1") for w in mask.cpu().tolist()))
        log(f"{kind}: {n} elements ({4 * n / 2 ** 20:.1f} MiB per buffer), {mask.numel()} mask words, {set_bits} decayed elements")
        del flat
        measure(n, mask, device, log)
    if opts.out:
        with open(opts.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
