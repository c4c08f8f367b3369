#!/usr/bin/env python3
"""Generates tests/golden/train_meter.npz and tests/golden/train_epoch.npz from the reference's own code on the CPU (build
container only, like oracle/make_golden.py, whose import recipe it reuses).  Numbers, names and printed text only.

  train_meter.npz   the reference's ``SmoothedValue(window_size=10)`` (utils/misc.py:40-91) fed 25 float32 losses the way the loop
                    feeds it (``loss_reduced.item()``): every property after every update.
  train_epoch.npz   the reference's ``engine.train_one_epoch`` (engine.py:59-122) on the model, criterion, settings and batches of
                    tests/train_epoch_cases.py with ``torch.optim.AdamW``: per epoch the returned values and the printed lines
                    (without the ETA), the parameters before and after; then the run whose batch 3 holds an inf: the exit code
                    and the parameters at the exit.

    python tools/make_train_epoch_golden.py
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import make_golden as MG  # noqa: E402
import train_epoch_cases as CASES  # noqa: E402


def meter_fixture(SmoothedValue):
    rng = np.random.default_rng(7)
    losses = np.abs(rng.normal(6.0, 3.0, 25)).astype(np.float32)
    losses[4], losses[13] = losses[2], losses[12]      # ties inside a window; (an even window's median is its lower middle)
    losses[20] = np.float32(1e-3)
    losses[21] = np.float32(3e4)
    meter = SmoothedValue(window_size=10)
    rows = {k: [] for k in ("avg", "median", "global_avg", "value", "max", "count", "total")}
    for x in losses:
        meter.update(torch.tensor(x).item())           # a Python float holding a float32, as `loss_reduced.item()` is
        for k in rows:
            rows[k].append(getattr(meter, k))
    arrays = {k: np.array(v, dtype=np.int64 if k == "count" else np.float64) for k, v in rows.items()}
    MG.save("train_meter", losses=losses, window=np.array(10), **arrays)


def epoch_fixture(E):
    args = CASES.settings()
    torch.manual_seed(0)
    model = CASES.DictModel()
    x, target = CASES.make_batches()
    arrays = {"x": x.numpy(), "target": target.numpy(), "bad_iter": np.array(CASES.BAD_ITER)}
    initial = {n: p.detach().clone() for n, p in model.named_parameters()}
    for n, p in initial.items():
        arrays[f"param:{n}"] = p.numpy()

    def optimizer(m):
        return torch.optim.AdamW(m.parameters(), lr=args.base_lr, weight_decay=CASES.WEIGHT_DECAY)

    opt = optimizer(model)
    for epoch in range(CASES.EPOCHS):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            ap, curr_iter, curr_lr, loss_avg, loss_dict = E.train_one_epoch(args, epoch, model, opt, CASES.mse_criterion, None,
                                                                            CASES.loader(x, target, epoch))
        assert ap is None and list(loss_dict) == ["loss_mse"]
        arrays[f"epoch{epoch}:curr_iter"] = np.array(curr_iter)
        arrays[f"epoch{epoch}:curr_lr"] = np.array(curr_lr, dtype=np.float64)
        arrays[f"epoch{epoch}:loss_avg"] = np.array(loss_avg, dtype=np.float64)
        arrays[f"epoch{epoch}:loss_mse"] = loss_dict["loss_mse"].numpy()
        arrays[f"epoch{epoch}:lines"] = np.array(CASES.cut_eta(out.getvalue()))
        for n, p in model.named_parameters():
            arrays[f"epoch{epoch}:param:{n}"] = p.detach().numpy().copy()
    # the run that meets a non-finite loss
    bad = CASES.load_params(CASES.DictModel(), arrays)
    code = None
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            E.train_one_epoch(args, 0, bad, optimizer(bad), CASES.mse_criterion, None, CASES.loader(x, target, 0, bad_iter=CASES.BAD_ITER))
    except SystemExit as e:
        code = e.code
    assert code is not None
    arrays["bad:exit_code"] = np.array(code)
    for n, p in bad.named_parameters():
        arrays[f"bad:param:{n}"] = p.detach().numpy().copy()
    MG.save("train_epoch", **arrays)


def main():
    MG.import_reference()
    ap = types.ModuleType("utils.ap_calculator")  # engine.py imports the AP calculator, which needs the unbuilt pointnet2 extension
    ap.APCalculator = None
    sys.modules["utils.ap_calculator"] = ap
    import engine as E  # noqa  (the reference's engine.py)
    from utils.misc import SmoothedValue  # noqa
    meter_fixture(SmoothedValue)
    epoch_fixture(E)


if __name__ == "__main__":
    main()
