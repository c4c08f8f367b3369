#!/usr/bin/env python3
"""Generates tests/golden/pointnet2_modules.npz: the reference's own ``third_party/pointnet2/pointnet2_modules.py`` run forward
and backward on CPU (build container only, like oracle/make_golden.py).

The reference's modules call the ``pointnet2._ext`` CUDA extension, which is not built here.  ``builtins.__POINTNET2_SETUP__``
lets its ``pointnet2_utils`` import without it, and ``_ext`` is then set to a stand-in that forwards the nine functions to the C
oracle (oracle/pointnet2_oracle.py).  Everything above that — grouping, the shared MLPs, BatchNorm, the poolings, the
interpolation weights, autograd — is the reference's code, so the fixture pins that composition.

Per configuration of tests/pointnet2_modules_cases.py: the seeded inputs, the state dict, the train-mode outputs (sampled
indices included), the running statistics after that call, the gradients of the feature inputs and of every parameter, and,
after BatchNorm weights / statistics were randomised (some weights negative), that state dict and the eval-mode outputs.

    python tools/make_pointnet2_modules_golden.py
"""
import builtins
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import make_golden as MG  # noqa: E402
from oracle import pointnet2_oracle as O  # noqa: E402
import pointnet2_modules_cases as K  # noqa: E402


class OracleExt:
    """``pointnet2._ext`` on the C oracle: tensors in, tensors out"""

    def __getattr__(self, name):
        def call(*args):
            out = getattr(O, name)(*[a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a for a in args])
            if isinstance(out, (tuple, list)):
                return tuple(torch.from_numpy(np.ascontiguousarray(o)) for o in out)
            return torch.from_numpy(np.ascontiguousarray(out))
        return call


def import_reference_modules():
    builtins.__POINTNET2_SETUP__ = True
    sys.path.insert(0, os.path.join(MG.REF, "third_party", "pointnet2"))
    import pointnet2_utils  # noqa  (the reference's)
    pointnet2_utils._ext = OracleExt()
    import pointnet2_modules  # noqa  (the reference's)
    return pointnet2_modules


def main():
    O.build()
    R = import_reference_modules()
    arrays = {"cases": np.array(sorted(K.CASES))}
    for name in sorted(K.CASES):
        cls, _, names = K.CASES[name]
        torch.manual_seed(sum(map(ord, name)))
        module = getattr(R, cls)(**K.fresh_kwargs(name)).train()
        for m in module.modules():  # the reference's GroupAll reads a flag its constructor never stores: give it the default
            if type(m).__name__ == "GroupAll" and not hasattr(m, "ret_grouped_xyz"):
                m.ret_grouped_xyz = False
        inputs = K.make_inputs(name)
        for key in names:
            if key is not None:
                arrays[f"{name}/in/{key}"] = inputs[key].numpy()
        sd = module.state_dict()
        arrays[f"{name}/keys"] = np.array(list(sd))
        for k, v in sd.items():
            arrays[f"{name}/sd0/{k}"] = v.numpy().copy()
        # shapes of the outputs first (a dry forward on a copy of the state), then the seeded output weights
        probe, _ = K.run_case(module, inputs, names)
        module.load_state_dict({k: torch.from_numpy(arrays[f"{name}/sd0/{k}"].copy()) for k in sd})
        g = torch.Generator().manual_seed(99)
        wout = [torch.randn(o.shape, generator=g) if (o is not None and o.is_floating_point() and o.requires_grad) else None for o in probe]
        out, grads = K.run_case(module, inputs, names, wout)
        for i, (o, w) in enumerate(zip(out, wout)):
            if o is not None:
                arrays[f"{name}/out/{i}"] = o.detach().numpy()
            if w is not None:
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
            if o is not None:
                arrays[f"{name}/eval/{i}"] = o.numpy()
        print(f"{name}: {cls}, {len(sd)} state entries, outputs {[tuple(o.shape) if o is not None else None for o in out]}")
    path = os.path.join(ROOT, "tests", "golden", "pointnet2_modules.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
