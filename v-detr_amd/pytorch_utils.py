"""Shared-MLP building blocks of the PointNet++ layers — the module nesting (and so the state-dict keys) of the reference's
``third_party/pointnet2/pytorch_utils.py``: ``SharedMLP`` holds ``layer{i}`` blocks, a block holds ``conv`` (or ``fc``), ``bn`` and
``activation``, and ``bn`` wraps the torch BatchNorm once more as ``bn``.  A checkpoint of the reference therefore loads as it is:
``…layer{i}.conv.weight`` and ``…layer{i}.bn.bn.{weight,bias,running_mean,running_var,num_batches_tracked}``; ``conv.bias`` exists
only without BatchNorm.

Every BatchNorm call goes through ``bn_act.batch_norm_module``, so cross-replica statistics (``--sync-bn``) cover these layers
like every other one.  The eval-mode fast path of the layers built from these blocks is in ``pointnet2_modules``.
"""
import torch.nn as nn

from . import bn_act as BNA


class _BNBase(nn.Sequential):
    """``bn``: one torch BatchNorm with weight 1 and bias 0"""

    def __init__(self, in_size, batch_norm=None, name=""):
        super().__init__()
        norm = batch_norm(in_size)
        nn.init.ones_(norm.weight)
        nn.init.zeros_(norm.bias)
        self.add_module(name + "bn", norm)

    def forward(self, x):
        return BNA.batch_norm_module(self[0], x)


class BatchNorm1d(_BNBase):
    def __init__(self, in_size, *, name=""):
        super().__init__(in_size, batch_norm=nn.BatchNorm1d, name=name)


class BatchNorm2d(_BNBase):
    def __init__(self, in_size, name=""):
        super().__init__(in_size, batch_norm=nn.BatchNorm2d, name=name)


def _assemble(block, name, unit_name, unit, norm, activation, preact):
    """the members of a block in the order they run: (bn, activation,) unit (, bn, activation)"""
    tail = [(name + "bn", norm), (name + "activation", activation)]
    members = (tail if preact else []) + [(name + unit_name, unit)] + ([] if preact else tail)
    for key, member in members:
        if member is not None:
            block.add_module(key, member)


class _ConvBase(nn.Sequential):
    def __init__(self, in_size, out_size, kernel_size, stride, padding, activation, bn, init, conv=None, batch_norm=None, bias=True,
                 preact=False, name=""):
        super().__init__()
        has_bias = bias and not bn  # BatchNorm's shift makes the convolution's bias redundant
        unit = conv(in_size, out_size, kernel_size=kernel_size, stride=stride, padding=padding, bias=has_bias)
        init(unit.weight)
        if has_bias:
            nn.init.zeros_(unit.bias)
        norm = batch_norm(in_size if preact else out_size) if bn else None
        _assemble(self, name, "conv", unit, norm, activation, preact)


class Conv1d(_ConvBase):
    def __init__(self, in_size, out_size, *, kernel_size=1, stride=1, padding=0, activation=nn.ReLU(inplace=False), bn=False,
                 init=nn.init.kaiming_normal_, bias=True, preact=False, name=""):
        super().__init__(in_size, out_size, kernel_size, stride, padding, activation, bn, init, conv=nn.Conv1d, batch_norm=BatchNorm1d,
                         bias=bias, preact=preact, name=name)


class Conv2d(_ConvBase):
    def __init__(self, in_size, out_size, *, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0), activation=nn.ReLU(inplace=False),
                 bn=False, init=nn.init.kaiming_normal_, bias=True, preact=False, name=""):
        super().__init__(in_size, out_size, kernel_size, stride, padding, activation, bn, init, conv=nn.Conv2d, batch_norm=BatchNorm2d,
                         bias=bias, preact=preact, name=name)


class FC(nn.Sequential):
    def __init__(self, in_size, out_size, *, activation=nn.ReLU(inplace=False), bn=False, init=None, preact=False, name=""):
        super().__init__()
        unit = nn.Linear(in_size, out_size, bias=not bn)
        if init is not None:
            init(unit.weight)
        if not bn:
            nn.init.zeros_(unit.bias)
        norm = BatchNorm1d(in_size if preact else out_size) if bn else None
        _assemble(self, name, "fc", unit, norm, activation, preact)


class SharedMLP(nn.Sequential):
    """``args[0] -> args[1] -> …`` as 1x1 ``Conv2d`` blocks on [B, C, npoint, nsample].  With ``first`` and ``preact`` the first
    block has neither BatchNorm nor activation in front of its convolution."""

    def __init__(self, args, *, bn=False, activation=nn.ReLU(inplace=False), preact=False, first=False, name=""):
        super().__init__()
        for i, (cin, cout) in enumerate(zip(args[:-1], args[1:])):
            bare = first and preact and i == 0
            self.add_module(f"{name}layer{i}", Conv2d(cin, cout, bn=bn and not bare, activation=None if bare else activation,
                                                      preact=preact))
