#!/usr/bin/env python3
"""Generates tests/golden/pointnet2_lfp.npz: the reference's own ``PointnetLFPModuleMSG`` run forward and backward on CPU (build
container only), its ``pointnet2._ext`` replaced by the C oracle exactly as tools/make_pointnet2_modules_golden.py does it.

Per configuration of tests/pointnet2_lfp_cases.py, what that tool records: the seeded inputs, ``keys`` (the state dict's order:
``post_mlp`` first), ``sd0``, the train-mode output, ``wout``, the gradients of ``features`` / ``features2`` and of every
parameter, ``after_train`` (running statistics and ``num_batches_tracked``: the shared post MLP counts one batch per scale),
``sd1`` (randomised BatchNorm, some weights negative) and the eval-mode output.

    python tools/make_pointnet2_lfp_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_pointnet2_modules_golden as G  # noqa: E402  (OracleExt / import_reference_modules; puts ROOT and tests/ on the path)
import pointnet2_lfp_cases as K  # noqa: E402


def main():
    G.O.build()
    R = G.import_reference_modules()
    arrays = {"cases": np.array(sorted(K.CASES))}
    for name in sorted(K.CASES):
        cls, _, names = K.CASES[name]
        torch.manual_seed(sum(map(ord, name)))
        module = getattr(R, cls)(**K.fresh_kwargs(name)).train()
        inputs = K.make_inputs(name)
        for key in names:
            if key is not None:
                arrays[f"{name}/in/{key}"] = inputs[key].numpy()
        sd = module.state_dict()
        arrays[f"{name}/keys"] = np.array(list(sd))
        for k, v in sd.items():
            arrays[f"{name}/sd0/{k}"] = v.numpy().copy()
        # shapes of the outputs first (a dry forward; the state is restored after it), then the seeded output weights
        probe, _ = K.run_case(module, inputs, names)
        module.load_state_dict({k: torch.from_numpy(arrays[f"{name}/sd0/{k}"].copy()) for k in sd})
        g = torch.Generator().manual_seed(99)
        wout = [torch.randn(o.shape, generator=g) for o in probe]
        out, grads = K.run_case(module, inputs, names, wout)
        for i, (o, w) in enumerate(zip(out, wout)):
            arrays[f"{name}/out/{i}"] = o.detach().numpy()
            arrays[f"{name}/wout/{i}"] = w.numpy()
        for key, gr in grads.items():
            arrays[f"{name}/grad_in/{key}"] = gr.numpy()
        for pname, p in module.named_parameters():
            arrays[f"{name}/grad_param/{pname}"] = p.grad.numpy()
        for k, v in module.state_dict().items():
            if "running_" in k or "num_batches" in k:
                arrays[f"{name}/after_train/{k}"] = v.numpy().copy()
        K.randomise_eval_state(module, name)
        for k, v in module.state_dict().items():
            arrays[f"{name}/sd1/{k}"] = v.numpy().copy()
        module.eval()
        with torch.no_grad():
            ev, _ = K.run_case(module, inputs, names)
        for i, o in enumerate(ev):
            arrays[f"{name}/eval/{i}"] = o.numpy()
        print(f"{name}: {cls}, {len(sd)} state entries, outputs {[tuple(o.shape) for o in out]}")
    path = os.path.join(ROOT, "tests", "golden", "pointnet2_lfp.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
