"""The configurations of tests/golden/pointnet2_modules.npz: shared by tools/make_pointnet2_modules_golden.py (which runs the
reference's modules on them) and the tests (which run this package's).  Fixture sizes: B = 2, N = 50, C = 4."""
import torch

B, N, C = 2, 50, 4

_VOTES = dict(mlp=[4, 16, 32], npoint=7, radius=0.6, nsample=16, normalize_xyz=True)
_MSG = dict(npoint=5, radii=[0.5, 1.0], nsamples=[16, 32], mlps=[[4, 8], [4, 16]])

# name -> (class name, constructor arguments, names of the forward's positional inputs)
CASES = {
    "votes_max": ("PointnetSAModuleVotes", dict(_VOTES, pooling="max"), ("xyz", "features")),
    "votes_avg": ("PointnetSAModuleVotes", dict(_VOTES, pooling="avg"), ("xyz", "features")),
    "votes_rbf": ("PointnetSAModuleVotes", dict(_VOTES, pooling="rbf"), ("xyz", "features")),
    "votes_nofeat": ("PointnetSAModuleVotes", dict(_VOTES, mlp=[0, 16]), ("xyz", None)),
    "votes_nobn": ("PointnetSAModuleVotes", dict(_VOTES, bn=False), ("xyz", "features")),
    "sa_groupall": ("PointnetSAModule", dict(mlp=[4, 16], npoint=None), ("xyz", "features")),
    "sa_msg": ("PointnetSAModuleMSG", dict(_MSG), ("xyz", "features")),
    "msg_votes": ("PointnetSAModuleMSGVotes", dict(_MSG), ("xyz", "features")),
    "fp_both": ("PointnetFPModule", dict(mlp=[36, 24]), ("xyz", "known", "features", "known_feats")),
    "fp_known_only": ("PointnetFPModule", dict(mlp=[32, 24]), ("xyz", "known", None, "known_feats")),
}


def fresh_kwargs(name):
    """constructor arguments with lists of their own (the reference's constructors write into them)"""
    return {k: ([list(x) if isinstance(x, list) else x for x in v] if isinstance(v, list) else v) for k, v in CASES[name][1].items()}


def make_inputs(name):
    """the case's seeded inputs, by name"""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    return {"xyz": torch.rand(B, N, 3, generator=g), "features": torch.randn(B, C, N, generator=g),
            "xyz2": torch.rand(B, 9, 3, generator=g), "features2": torch.randn(B, 4, 9, generator=g),
            "known": torch.rand(B, 12, 3, generator=g), "known_feats": torch.randn(B, 32, 12, generator=g)}


def differentiable(key):
    return key is not None and "feat" in key


def run_case(module, inputs, names, wout=None):
    """forward (+ backward of sum(out * wout) when `wout` is given); returns (outputs tuple, {input name: grad})"""
    args = []
    for key in names:
        t = None if key is None else inputs[key].clone()
        if wout is not None and differentiable(key):
            t.requires_grad_(True)
        args.append(t)
    out = module(*args)
    out = out if isinstance(out, tuple) else (out,)
    grads = {}
    if wout is not None:
        loss = sum((o * w.to(o.device)).sum() for o, w in zip(out, wout) if w is not None)
        loss.backward()
        grads = {key: a.grad for key, a in zip(names, args) if differentiable(key)}
    return out, grads


def randomise_eval_state(module, name):
    """BatchNorm weights (some negative), biases and running statistics that make the eval forward no identity fold"""
    g = torch.Generator().manual_seed(7 + sum(map(ord, name)))
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.5)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
            elif isinstance(m, torch.nn.Conv2d) and m.bias is not None:
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
