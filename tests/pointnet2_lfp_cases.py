"""The configurations of tests/golden/pointnet2_lfp.npz (PointnetLFPModuleMSG): shared by tools/make_pointnet2_lfp_golden.py
(which runs the reference's module on them) and the tests (which run this package's).  The seeded inputs, the forward / backward
driver and the eval-state randomiser are those of pointnet2_modules_cases.  Fixture sizes: B = 2, N1 = 50, N2 = 9, C1 = C2 = 4."""
from pointnet2_modules_cases import make_inputs, randomise_eval_state, run_case  # noqa: F401  (re-exported)

_CLS = "PointnetLFPModuleMSG"
_NAMES = ("xyz2", "xyz", "features2", "features")  # forward(xyz2, xyz1, features2, features1)
_TWO = dict(mlps=[[4, 16], [4, 16]], radii=[0.5, 1.0], nsamples=[16, 32], post_mlp=[20, 24])

# name -> (class name, constructor arguments, names of the forward's positional inputs)
CASES = {
    "lfp_two": (_CLS, dict(_TWO), _NAMES),
    "lfp_nofeat2": (_CLS, dict(mlps=[[4, 8, 16]], radii=[0.4], nsamples=[16], post_mlp=[16, 32, 16]), ("xyz2", "xyz", None, "features")),
    "lfp_nobn": (_CLS, dict(_TWO, bn=False), _NAMES),
    "lfp_noxyz": (_CLS, dict(_TWO, use_xyz=False), _NAMES),
}


def fresh_kwargs(name):
    """constructor arguments with lists of their own (the reference's constructor writes into them)"""
    return {k: ([list(x) if isinstance(x, list) else x for x in v] if isinstance(v, list) else v) for k, v in CASES[name][1].items()}


def cancels_in_train_mode(name, pname):
    """True for a parameter whose train-mode gradient is zero by construction, so that the fixture holds only the rounding of a sum
    that cancels (about 2e-6 next to gradients of 15 to 60) and a tolerance relative to that tensor's own magnitude asks for the
    reference's noise: the bias of the LAST BatchNorm of a scale's MLP.  Every centre of these cases has a positive pooled value in
    every channel, so that bias adds the same constant to the channel's pooled feature at every (scene, point); the post MLP's first
    convolution turns it into a per-channel constant, and its train-mode BatchNorm subtracts the batch mean.  The tests bound such
    a gradient (the fixture's and the module's) by atol x the largest parameter gradient of the case instead."""
    args = CASES[name][1]
    if not args.get("bn", True):
        return False
    return any(pname == f"mlps.{k}.layer{len(spec) - 2}.bn.bn.bias" for k, spec in enumerate(args["mlps"]))
