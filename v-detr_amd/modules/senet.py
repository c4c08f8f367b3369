"""Squeeze-and-excitation blocks of the sparse module library: the third file of the family that ``common`` and
``resnet_block`` come from.  ``SELayer`` scales every channel of a sparse tensor by a gate computed from the scene's average,
``gate = sigmoid(W2 relu(W1 avg_s(x) + b1) + b2)``; the blocks apply it after their last norm and before ``out += residual; relu``.
Attribute names, and with them the state-dict keys, are the library's: ``se.fc.0.linear.weight`` ... ``se.fc.2.linear.bias``.

forward: ``broadcast_mul(x, fc(pooling(x)))``.  In inference (``heads.inference``, ``minkowski.INFER_FUSED``) the layer is
``sparse_ops.se_scale``: pooling partials, fold + gate, broadcast multiply — three launches, the block's residual add and ReLU
inside the last one.  ``SELayer.last_path`` says which form ran.
"""
import torch
import torch.nn as nn

from .. import heads as HD
from .. import minkowski as ME
from .. import sparse_ops as S
from .common import ConvType
from .resnet_block import BasicBlockBase, BottleneckBase, NormType, _norm_relu


class SELayer(nn.Module):
    def __init__(self, channel, reduction=16, D=3):
        super().__init__()
        if D != 3:
            raise NotImplementedError(f"D = {D}: three spatial dimensions only")
        hidden = channel // reduction
        if hidden < 1:
            raise ValueError(f"SELayer: channel {channel} // reduction {reduction} leaves no hidden unit")
        self.fc = nn.Sequential(ME.MinkowskiLinear(channel, hidden), ME.MinkowskiReLU(inplace=True),
                                ME.MinkowskiLinear(hidden, channel), ME.MinkowskiSigmoid())
        self.pooling = ME.MinkowskiGlobalPooling()
        self.broadcast_mul = ME.MinkowskiBroadcastMultiplication()
        self.last_path = None  # "fused" / "composition": the form of the last forward

    def _fusable(self, x, residual):
        """the gate of the inference form; everything else — training, autograd, CPU tensors, widths the launch does not take, a
        residual on other sites — takes the composition, unchanged"""
        if not (ME.INFER_FUSED and HD.inference(self)) or ME._geometry_only():
            return False
        w1, w2 = self.fc[0].linear, self.fc[2].linear
        tables = [x.F] + ([] if residual is None else [residual.F])
        if residual is not None and not (x._same_map(residual) and residual.F.shape == x.F.shape):
            return False
        if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tables):
            return False
        params = [p for p in (w1.weight, w1.bias, w2.weight, w2.bias) if p is not None]
        if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in params):
            return False
        C = x.F.shape[1]
        return C % 4 == 0 and C <= 1024 and 1 <= w1.out_features <= 256 and w1.in_features == C

    def forward(self, x, residual=None, relu=None):
        """x scaled by its scene's gate; the SE blocks also hand over their tail: ``relu(out + residual)`` with ``relu`` the
        block's MinkowskiReLU"""
        if self._fusable(x, residual):
            seg, nseg = x.coordinate_manager.scene_segments(x.keys)
            w1, w2 = self.fc[0].linear, self.fc[2].linear
            self.last_path = "fused"
            return x._like(S.se_scale(x.F, seg, nseg, w1.weight, w1.bias, w2.weight, w2.bias,
                                      None if residual is None else residual.F, relu is not None))
        if not ME._geometry_only():
            self.last_path = "composition"
        out = self.broadcast_mul(x, self.fc(self.pooling(x)))
        if residual is not None:
            out = out + residual
        return out if relu is None else relu(out)


class SEBasicBlock(BasicBlockBase):
    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, conv_type=ConvType.HYPERCUBE, reduction=16,
                 bn_momentum=0.1, D=3):
        super().__init__(inplanes, planes, stride=stride, dilation=dilation, downsample=downsample, conv_type=conv_type,
                         bn_momentum=bn_momentum, D=D)
        self.se = SELayer(planes * self.expansion, reduction=reduction, D=D)

    def forward(self, x):
        residual = x if self.downsample is None else self.downsample(x)
        out = _norm_relu(self.norm1, self.relu, self.conv1(x))
        out = self.norm2(self.conv2(out))
        return self.se(out, residual, self.relu)


class SEBasicBlockIN(SEBasicBlock):
    NORM_TYPE = NormType.INSTANCE_NORM


class SEBasicBlockINBN(SEBasicBlock):
    NORM_TYPE = NormType.INSTANCE_BATCH_NORM


class SEBottleneck(BottleneckBase):
    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, conv_type=ConvType.HYPERCUBE, reduction=16,
                 bn_momentum=0.1, D=3):
        super().__init__(inplanes, planes, stride=stride, dilation=dilation, downsample=downsample, conv_type=conv_type,
                         bn_momentum=bn_momentum, D=D)
        self.se = SELayer(planes * self.expansion, reduction=reduction, D=D)

    def forward(self, x):
        residual = x if self.downsample is None else self.downsample(x)
        out = _norm_relu(self.norm1, self.relu, self.conv1(x))
        out = _norm_relu(self.norm2, self.relu, self.conv2(out))
        out = self.norm3(self.conv3(out))
        return self.se(out, residual, self.relu)


class SEBottleneckIN(SEBottleneck):
    NORM_TYPE = NormType.INSTANCE_NORM


class SEBottleneckINBN(SEBottleneck):
    NORM_TYPE = NormType.INSTANCE_BATCH_NORM
