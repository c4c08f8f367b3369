#!/usr/bin/env python3
"""Measures what engine.train_one_epoch's ClipAdamW form is built on:

  1. the host wall time per iteration of the loop on the small real model of tests/test_gpu_train_epoch.py (ModelVDETR behind the
     sparse backbone, dec_nlayers 2, 32 queries, the device criterion; the batches of tests/train_epoch_cases.py already on the
     device), as it is -- the meter read only after the loop -- and with ``LossMeter.read()`` forced behind every ``update``, which
     is where the reference's loop reads the loss (engine.py:100).  Rounds of one epoch each, the two variants alternating, the
     device drained only at a round's two ends.  (The C2 decoder of bench.py takes backbone features, not the loop's three input
     keys: it is not measured here.)
  2. vdetr_adamw_guard_f32 with a clear flag against vdetr_adamw_sched_f32 (table + mask, clipping) on the C2 decoder's flat
     buffer, in rotating order, as tools/optim_sched_bench.py measures; and the guard with a raised flag.
  3. the meter launch alone.

Reported: median, fastest and slowest round and the spread (slowest - fastest) / median.  Needs a GPU: there is no fallback.

    python tools/train_loop_bench.py [--out profiles/train_loop_bench.txt]
"""
import argparse
import contextlib
import ctypes
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOOP_ROUNDS, LOOP_ITERS = 7, 20
ROUNDS, LAUNCHES, WARMUP = 15, 200, 50
DECODER_ELEMENTS = 11827284   # the C2 decoder's FlatParams (profiles/optim_sched_bench.txt)


def report(log, name, t, unit, extra=""):
    med = statistics.median(t)
    log(f"  {name:44s} median {med:9.3f} {unit}  fastest {min(t):9.3f}  slowest {max(t):9.3f}  spread {(max(t) - min(t)) / med * 100:5.2f} %{extra}")
    return med


def loop_bench(device, log):
    import train_epoch_cases as CASES
    from vdetr_amd import engine
    from vdetr_amd.criterion import build_criterion, default_criterion_args
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    from vdetr_amd.dist import FlatParams
    from vdetr_amd.model_vdetr import build_vdetr, default_args
    from vdetr_amd.optim import build_optimizer
    ds = ScannetDatasetConfig()
    torch.manual_seed(0)
    model = build_vdetr(default_args(dec_nlayers=2, nqueries=32, preenc_npoints=256), ds, "minkowski").to(device)
    criterion = build_criterion(default_criterion_args(), ds)
    args = CASES.settings(max_epoch=10 ** 6, warm_lr_epochs=0, base_lr=1e-5, weight_decay=0.1, filter_biases_wd=True, log_every=10 ** 9)
    flat = FlatParams(list(model.parameters()))
    opt = build_optimizer(args, model, flat)
    scenes = [{k: v.to(device) for k, v in b.items()} for b in CASES.real_scenes(ds)]
    loader = [scenes[i % 2] for i in range(LOOP_ITERS)]

    class ReadingMeter(engine.LossMeter):
        def update(self, loss, curr_iter):
            super().update(loss, curr_iter)
            self.read()

    plain_meter = engine.LossMeter
    epoch = [1]   # (epoch 0's first iteration would be a logging one)

    def one_round(meter_cls):
        engine.LossMeter = meter_cls
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                engine.train_one_epoch(args, epoch[0], model, opt, criterion, ds, [dict(b) for b in loader])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
        finally:
            engine.LossMeter = plain_meter
        epoch[0] += 1
        return (t1 - t0) * 1e3 / LOOP_ITERS

    for cls in (plain_meter, ReadingMeter):   # warm-up: allocator, tuning, lazy initialisation
        one_round(cls)
    walls = {"no read in the loop": [], "meter.read() every iteration": []}
    for r in range(LOOP_ROUNDS):
        order = [("no read in the loop", plain_meter), ("meter.read() every iteration", ReadingMeter)]
        for name, cls in (order if r % 2 == 0 else order[::-1]):
            walls[name].append(one_round(cls))
    log(f"train_one_epoch, ClipAdamW form, small real model ({flat.data.numel()} parameters), {LOOP_ROUNDS} rounds x {LOOP_ITERS} iterations "
        "per variant, alternating; ms per iteration")
    meds = {}
    for name in walls:
        meds[name] = report(log, name, walls[name], "ms")
    a, b = meds["no read in the loop"], meds["meter.read() every iteration"]
    own = max(walls["no read in the loop"]) - min(walls["no read in the loop"])
    log(f"  a read per iteration costs {b - a:+.3f} ms per iteration ({(b - a) / a * 100:+.2f} %); the loop's own spread across rounds: {own:.3f} ms")
    if not bool(torch.isfinite(flat.data).all()):
        raise RuntimeError("the timed epochs left non-finite parameters")


def launch_bench(device, log):
    from vdetr_amd import _lib as L
    lib = L.lib()
    n = DECODER_ELEMENTS
    gen = torch.Generator(device=device).manual_seed(0)
    p, g = torch.randn(n, device=device, generator=gen) * 0.02, torch.randn(n, device=device, generator=gen) * 1e-3
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    nsum = lib.vdetr_sumsq_blocks(n)
    partial = torch.empty(nsum, device=device)
    L.check(lib.vdetr_sumsq_f32(g.data_ptr(), n, partial.data_ptr(), nsum, L.stream_ptr()), "sumsq")
    step, ticket = torch.zeros((), device=device), torch.zeros(4, dtype=torch.int32, device=device)
    norm, lr_out = torch.zeros((), device=device), torch.zeros((), dtype=torch.float64, device=device)
    table = torch.from_numpy(np.linspace(7e-4, 1e-6, 81000)).to(device)
    mask = torch.full(((n + 31) // 32,), 0x77777777, dtype=torch.int32, device=device)
    clear, raised = torch.zeros((), dtype=torch.int32, device=device), torch.ones((), dtype=torch.int32, device=device)

    def desc(cls, skip=None):
        d = cls()
        d.param, d.grad, d.exp_avg, d.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
        d.n, d.step, d.ticket = n, step.data_ptr(), ticket.data_ptr()
        d.sumsq, d.nsumsq, d.max_norm, d.norm_eps, d.norm_out = partial.data_ptr(), nsum, 0.1, 1e-6, norm.data_ptr()
        d.lr, d.beta1, d.beta2, d.eps, d.weight_decay = 7e-4, 0.9, 0.999, 1e-8, 0.1
        d.lr_table, d.n_lr, d.decay_mask, d.lr_out = table.data_ptr(), table.numel(), mask.data_ptr(), lr_out.data_ptr()
        if skip is not None:
            d.skip = skip.data_ptr()
        return d

    from vdetr_amd import engine
    meter = engine.LossMeter(device=device)
    loss = torch.full((), 4.25, device=device)
    md = L.LossMeterDesc(loss=loss.data_ptr(), state=meter.state.data_ptr(), iter=0)
    variants = [("adamw_sched, table + mask (yardstick)", lib.vdetr_adamw_sched_f32, desc(L.AdamWSchedDesc)),
                ("adamw_guard, skip == 0", lib.vdetr_adamw_guard_f32, desc(L.AdamWGuardDesc, clear)),
                ("adamw_guard, skip == 1", lib.vdetr_adamw_guard_f32, desc(L.AdamWGuardDesc, raised)),
                ("loss_meter_update", lib.vdetr_loss_meter_update_f32, md)]
    stream = L.stream_ptr()

    def run(fn, d, k):
        for _ in range(k):
            if fn(ctypes.byref(d), stream) != 0:
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
    if not bool(torch.isfinite(p).all()) or int(ticket[0]) != 0:
        raise RuntimeError("the timed updates left non-finite parameters or a drawn ticket")
    log(f"launches on the C2 decoder's flat buffer ({n} elements), {ROUNDS} rounds x {LAUNCHES} launches per variant, rotating order; "
        "us per launch, back to back on one stream")
    meds = {name: report(log, name, times[name], "us") for name, _, _ in variants}
    t = times[variants[0][0]]
    base, own_spread = meds[variants[0][0]], max(t) - min(t)
    diff = meds["adamw_guard, skip == 0"] - base
    log(f"  guard (skip == 0) - sched: {diff:+.3f} us ({diff / base * 100:+.2f} %); the sched launch's own spread across rounds: {own_spread:.3f} us "
        f"-> {'within' if diff <= own_spread else 'BEYOND'} it")
    snap = meter.read()
    log(f"  (the meter took {snap.count} updates; window average {snap.avg})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_loop_bench: needs a GPU")
    device = torch.device("cuda:0")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(torch.cuda.get_device_name(0))
    loop_bench(device, log)
    launch_bench(device, log)
    if opts.out:
        with open(opts.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
