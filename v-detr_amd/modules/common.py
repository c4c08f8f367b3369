"""Layer factories of the reference's sparse module library (models/modules/common.py) with its public names and signatures,
built on ``vdetr_amd.minkowski`` instead of MinkowskiEngine: norm and convolution kinds as enums, and ``conv`` / ``conv_tr`` /
``avg_pool`` / ``avg_unpool`` / ``sum_pool`` over a ``KernelGenerator``.

Three spatial dimensions only: ``D = 4`` and the spatio-temporal kinds that need it raise NotImplementedError; with ``D = 3``
every ``ConvType`` is accepted (the temporal part of a kind has nothing to act on).  Offset orders, and what of this is this
package's own definition and not MinkowskiEngine's, are in ``minkowski.KernelGenerator`` and DESIGN 6.10.
"""
from collections.abc import Sequence
from enum import Enum

import torch.nn as nn

from .. import minkowski as ME


class NormType(Enum):
    BATCH_NORM = 0
    INSTANCE_NORM = 1
    INSTANCE_BATCH_NORM = 2


def get_norm(norm_type, n_channels, D, bn_momentum=0.1):
    if norm_type == NormType.BATCH_NORM:
        return ME.MinkowskiBatchNorm(n_channels, momentum=bn_momentum)
    if norm_type == NormType.INSTANCE_NORM:
        return ME.MinkowskiInstanceNorm(n_channels)
    if norm_type == NormType.INSTANCE_BATCH_NORM:
        return nn.Sequential(ME.MinkowskiInstanceNorm(n_channels), ME.MinkowskiBatchNorm(n_channels, momentum=bn_momentum))
    raise ValueError(f"Norm type: {norm_type} not supported")


class ConvType(Enum):
    """the kernel region of a layer; ``int(kind)`` is its number, ``kind.fullname`` its name"""
    HYPERCUBE = 0, "HYPERCUBE"
    SPATIAL_HYPERCUBE = 1, "SPATIAL_HYPERCUBE"
    SPATIO_TEMPORAL_HYPERCUBE = 2, "SPATIO_TEMPORAL_HYPERCUBE"
    HYPERCROSS = 3, "HYPERCROSS"
    SPATIAL_HYPERCROSS = 4, "SPATIAL_HYPERCROSS"
    SPATIO_TEMPORAL_HYPERCROSS = 5, "SPATIO_TEMPORAL_HYPERCROSS"
    SPATIAL_HYPERCUBE_TEMPORAL_HYPERCROSS = 6, "SPATIAL_HYPERCUBE_TEMPORAL_HYPERCROSS"

    def __new__(cls, value, fullname):
        member = object.__new__(cls)
        member._value_ = value
        member.fullname = fullname
        return member

    def __int__(self):
        return self.value


_CROSS = (ConvType.HYPERCROSS, ConvType.SPATIAL_HYPERCROSS, ConvType.SPATIO_TEMPORAL_HYPERCROSS)
_SPATIAL = (ConvType.SPATIAL_HYPERCUBE, ConvType.SPATIAL_HYPERCROSS)
conv_to_region_type = {kind: (ME.RegionType.HYPER_CROSS if kind in _CROSS else ME.RegionType.HYPER_CUBE) for kind in ConvType}
int_to_region_type = {m: ME.RegionType(m) for m in range(3)}


def convert_region_type(region_type):
    """the RegionType of an integer"""
    return int_to_region_type[region_type]


def convert_conv_type(conv_type, kernel_size, D):
    """-> (region_type, axis_types, kernel_size) of a ConvType in D dimensions"""
    assert isinstance(conv_type, ConvType), "conv_type must be of ConvType"
    if D != 3:
        raise NotImplementedError(f"D = {D}: three spatial dimensions only (the temporal axis of D = 4 is not built)")
    axis_types = None
    if conv_type in _SPATIAL:  # the spatial part of the size, one entry per axis
        kernel_size = list(kernel_size[:3]) if isinstance(kernel_size, Sequence) else [kernel_size] * 3
    elif conv_type == ConvType.SPATIAL_HYPERCUBE_TEMPORAL_HYPERCROSS:
        axis_types = [ME.RegionType.HYPER_CUBE] * 3
    return conv_to_region_type[conv_type], axis_types, kernel_size


def _generator(kernel_size, stride, dilation, region_type, axis_types, D):
    return ME.KernelGenerator(kernel_size, stride, dilation, region_type=region_type, axis_types=axis_types, dimension=D)


def conv(in_planes, out_planes, kernel_size, stride=1, dilation=1, bias=False, conv_type=ConvType.HYPERCUBE, D=-1):
    assert D > 0, "Dimension must be a positive integer"
    region_type, _, kernel_size = convert_conv_type(conv_type, kernel_size, D)
    generator = _generator(kernel_size, stride, dilation, region_type, None, D)  # (the reference passes no axis_types here)
    return ME.MinkowskiConvolution(in_channels=in_planes, out_channels=out_planes, kernel_size=kernel_size, stride=stride,
                                   dilation=dilation, bias=bias, kernel_generator=generator, dimension=D)


def conv_tr(in_planes, out_planes, kernel_size, upsample_stride=1, dilation=1, bias=False, conv_type=ConvType.HYPERCUBE, D=-1):
    assert D > 0, "Dimension must be a positive integer"
    region_type, axis_types, kernel_size = convert_conv_type(conv_type, kernel_size, D)
    generator = _generator(kernel_size, upsample_stride, dilation, region_type, axis_types, D)
    return ME.MinkowskiConvolutionTranspose(in_channels=in_planes, out_channels=out_planes, kernel_size=kernel_size,
                                            stride=upsample_stride, dilation=dilation, bias=bias, kernel_generator=generator,
                                            dimension=D)


def _pooling(cls, kernel_size, stride, dilation, conv_type, D):
    assert D > 0, "Dimension must be a positive integer"
    region_type, axis_types, kernel_size = convert_conv_type(conv_type, kernel_size, D)
    generator = _generator(kernel_size, stride, dilation, region_type, axis_types, D)
    return cls(kernel_size=kernel_size, stride=stride, dilation=dilation, kernel_generator=generator, dimension=D)


def avg_pool(kernel_size, stride=1, dilation=1, conv_type=ConvType.HYPERCUBE, in_coords_key=None, D=-1):
    return _pooling(ME.MinkowskiAvgPooling, kernel_size, stride, dilation, conv_type, D)


def avg_unpool(kernel_size, stride=1, dilation=1, conv_type=ConvType.HYPERCUBE, D=-1):
    return _pooling(ME.MinkowskiAvgUnpooling, kernel_size, stride, dilation, conv_type, D)


def sum_pool(kernel_size, stride=1, dilation=1, conv_type=ConvType.HYPERCUBE, D=-1):
    return _pooling(ME.MinkowskiSumPooling, kernel_size, stride, dilation, conv_type, D)
