"""Residual blocks of the reference's sparse module library (models/modules/resnet_block.py): ``BasicBlock`` / ``Bottleneck``
with BatchNorm, InstanceNorm (``IN``) or InstanceNorm followed by BatchNorm (``INBN``), the kernel region chosen by a
``ConvType``.  Attribute names, and with them the state-dict keys, are the reference's: ``conv1.kernel``, ``norm1.bn.weight``
(BatchNorm), ``norm1.weight`` (IN), ``norm1.0.weight`` / ``norm1.1.bn.weight`` (INBN).

forward: conv -> norm -> ReLU ... conv -> norm, ``out += residual``, ReLU.  Where a norm ends in BatchNorm, the ReLU (and in the
last stage the residual add in front of it) run inside that layer's fused launch: the same composition, fewer launches.
"""
import torch.nn as nn

from .. import minkowski as ME
from .common import ConvType, NormType, conv, get_norm


def _norm_relu(norm, relu, x, residual=None):
    """relu(norm(x) + residual)"""
    layers = list(norm) if isinstance(norm, nn.Sequential) else [norm]
    for layer in layers[:-1]:
        x = layer(x)
    if isinstance(layers[-1], ME.MinkowskiBatchNorm):
        return layers[-1](x, act="relu", residual=residual)
    x = layers[-1](x)
    return relu(x if residual is None else x + residual)


class BasicBlockBase(nn.Module):
    expansion = 1
    NORM_TYPE = NormType.BATCH_NORM

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, conv_type=ConvType.HYPERCUBE, bn_momentum=0.1, D=3):
        super().__init__()
        self.conv1 = conv(inplanes, planes, kernel_size=3, stride=stride, dilation=dilation, conv_type=conv_type, D=D)
        self.norm1 = get_norm(self.NORM_TYPE, planes, D, bn_momentum=bn_momentum)
        self.conv2 = conv(planes, planes, kernel_size=3, stride=1, dilation=dilation, bias=False, conv_type=conv_type, D=D)
        self.norm2 = get_norm(self.NORM_TYPE, planes, D, bn_momentum=bn_momentum)
        self.relu = ME.MinkowskiReLU(inplace=False)
        self.downsample = downsample

    def forward(self, x):
        residual = x if self.downsample is None else self.downsample(x)
        out = _norm_relu(self.norm1, self.relu, self.conv1(x))
        return _norm_relu(self.norm2, self.relu, self.conv2(out), residual)


class BasicBlock(BasicBlockBase):
    NORM_TYPE = NormType.BATCH_NORM


class BasicBlockIN(BasicBlockBase):
    NORM_TYPE = NormType.INSTANCE_NORM


class BasicBlockINBN(BasicBlockBase):
    NORM_TYPE = NormType.INSTANCE_BATCH_NORM


class BottleneckBase(nn.Module):
    expansion = 4
    NORM_TYPE = NormType.BATCH_NORM

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, conv_type=ConvType.HYPERCUBE, bn_momentum=0.1, D=3):
        super().__init__()
        self.conv1 = conv(inplanes, planes, kernel_size=1, D=D)
        self.norm1 = get_norm(self.NORM_TYPE, planes, D, bn_momentum=bn_momentum)
        self.conv2 = conv(planes, planes, kernel_size=3, stride=stride, dilation=dilation, conv_type=conv_type, D=D)
        self.norm2 = get_norm(self.NORM_TYPE, planes, D, bn_momentum=bn_momentum)
        self.conv3 = conv(planes, planes * self.expansion, kernel_size=1, D=D)
        self.norm3 = get_norm(self.NORM_TYPE, planes * self.expansion, D, bn_momentum=bn_momentum)
        self.relu = ME.MinkowskiReLU(inplace=False)
        self.downsample = downsample

    def forward(self, x):
        residual = x if self.downsample is None else self.downsample(x)
        out = _norm_relu(self.norm1, self.relu, self.conv1(x))
        out = _norm_relu(self.norm2, self.relu, self.conv2(out))
        return _norm_relu(self.norm3, self.relu, self.conv3(out), residual)


class Bottleneck(BottleneckBase):
    NORM_TYPE = NormType.BATCH_NORM


class BottleneckIN(BottleneckBase):
    NORM_TYPE = NormType.INSTANCE_NORM


class BottleneckINBN(BottleneckBase):
    NORM_TYPE = NormType.INSTANCE_BATCH_NORM
