#!/usr/bin/env python3
"""Generates tests/golden/lr_schedule.npz: the reference's own engine.compute_learning_rate over every iteration of the schedules
of tests/optim_sched_cases.py (engine.py:70-81: ``curr_iter / max_iters``), and the parameter names its optimizer.build_optimizer
puts into the two groups under ``--filter_biases_wd`` for that file's small model (build container only, like oracle/make_golden.py,
whose import recipe it reuses).  Settings, names and numbers only.

    python tools/make_lr_schedule_golden.py
"""
import json
import os
import sys
import types
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import make_golden as MG  # noqa: E402
import optim_sched_cases as CASES  # noqa: E402

FIELDS = ("base_lr", "warm_lr", "warm_lr_epochs", "final_lr", "lr_scheduler", "max_epoch", "step_epoch")


def main():
    MG.import_reference()
    ap = types.ModuleType("utils.ap_calculator")  # engine.py imports the AP calculator, which needs the unbuilt pointnet2 extension
    ap.APCalculator = None
    sys.modules["utils.ap_calculator"] = ap
    import engine as E  # noqa  (the reference's engine.py)
    import optimizer as O  # noqa  (the reference's optimizer.py)
    # main.py holds the defaults; of what it imports, the sparse-convolution library and the logger are absent and unused here
    for absent in ("MinkowskiEngine", "wandb"):
        sys.modules[absent] = types.ModuleType(absent)
    sys.modules["models"].build_model = None
    MG.import_reference_criterion()
    import main as M  # noqa
    arrays = {}
    for name, (settings, ipe) in CASES.SCHEDULES.items():
        if settings is None:
            d = vars(M.make_args_parser().parse_args(["--dataset_name", "scannet"]))
            settings = {k: d[k] for k in FIELDS}
        a = Namespace(**settings)
        max_iters = a.max_epoch * ipe
        arrays[f"{name}:settings"] = np.array(json.dumps(settings))
        arrays[f"{name}:iters_per_epoch"] = np.array(ipe)
        arrays[f"{name}:table"] = np.array([E.compute_learning_rate(a, i / max_iters) for i in range(max_iters)], dtype=np.float64)
    model = CASES.small_model()
    names = {id(p): n for n, p in model.named_parameters()}
    opt = O.build_optimizer(Namespace(filter_biases_wd=True, weight_decay=0.1, base_lr=7e-4), model)
    no_decay, decay = opt.param_groups
    assert no_decay["weight_decay"] == 0.0 and decay["weight_decay"] == 0.1
    arrays["names:no_decay"] = np.array([names[id(p)] for p in no_decay["params"]])
    arrays["names:decay"] = np.array([names[id(p)] for p in decay["params"]])
    arrays["names:all"] = np.array([n for n, _ in model.named_parameters()])
    arrays["shapes:all"] = np.array(json.dumps([list(p.shape) for p in model.parameters()]))
    MG.save("lr_schedule", **arrays)


if __name__ == "__main__":
    main()
