"""PointNet++ set-abstraction and feature-propagation layers — the classes, constructor arguments, forward signatures, return
conventions and state-dict keys of the reference's ``third_party/pointnet2/pointnet2_modules.py``, on this package's HIP ops.

Two paths:

* the **composition** (train and eval mode, differentiable): FPS, ``gather_operation``, ``QueryAndGroup`` / ``GroupAll``,
  ``three_nn``, ``three_interpolate`` of ``pointnet2_utils`` and the ``SharedMLP`` of ``pytorch_utils`` — the reference's own
  sequence of ops, BatchNorm through ``bn_act`` so that cross-replica statistics cover it;
* the **fused eval forward** (``csrc/group_mlp.hip``): under ``heads.inference(module)`` (eval mode, autograd off) a max-pooled
  set abstraction, and a feature propagation, run as ONE launch after the ball query / ``three_nn``: gather, 1 to 3 folded
  ``relu(scale * (W x) + shift)`` layers on an LDS tile, pooling.  The grouped [B, C, npoint, nsample] tensors never exist.
  Shapes it is not built for take the composition (``_sa_fusable`` / ``_fp_fusable``); a missing kernel is an error, not a
  fallback.  ``FUSED = False`` keeps every call on the composition (A/B runs, parity tests); ``LAST_PATHS`` and each module's
  ``last_paths`` record which path every scale of the last call took, ``FUSED_LAUNCHES`` counts the fused launches.
  ``PointnetLFPModuleMSG`` adds a third launch: its shared post MLP on every scale's pooled features (``_post_fusable``), up to
  four scales at a time, written straight into the scales' channel slices; its ``last_paths`` end with that stage's entry.

One deliberate difference from the reference: the constructors work on a COPY of the caller's ``mlp`` / ``mlps`` lists.  The
reference adds 3 to the caller's first entry in place (``use_xyz``), so building two layers from one list gives the second a wrong
width there.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import heads as HD
from . import pointnet2_utils
from . import pytorch_utils as pt_utils

FUSED = True          # the fused eval forward where it applies (tests and tools/sa_module_bench.py set False: the A/B reference)
LAST_PATHS = []       # "fused" / "composition" per scale of the last forward of any layer of this file
FUSED_LAUNCHES = 0    # fused launches so far in this process

_NSAMPLES = (16, 32, 64)
_LIMIT = 2 ** 31


def _pad(n, to):
    return (n + to - 1) // to * to


# ---- the packed form of a SharedMLP: transposed zero-padded weight images and folded BatchNorm vectors ---------------------------
def _mlp_layers(mlp):
    """[(conv, norm or None)] of a SharedMLP whose blocks are 1x1 convolution -> (BatchNorm ->) ReLU, else None"""
    layers = []
    for block in mlp:
        if not isinstance(block, pt_utils.Conv2d):
            return None
        members = list(block.children())
        conv, rest = members[0], members[1:]
        if not isinstance(conv, nn.Conv2d) or conv.kernel_size != (1, 1) or conv.stride != (1, 1) or conv.padding != (0, 0) \
                or conv.groups != 1:
            return None
        norm = None
        if rest and isinstance(rest[0], pt_utils.BatchNorm2d):
            norm, rest = rest[0][0], rest[1:]
            if not (isinstance(norm, nn.BatchNorm2d) and norm.affine and norm.track_running_stats and norm.running_mean is not None):
                return None
        if len(rest) != 1 or type(rest[0]) is not nn.ReLU:
            return None
        layers.append((conv, norm))
    return layers


def _mlp_shape_ok(layers, cin):
    return (layers is not None and 1 <= len(layers) <= 3 and 1 <= cin <= 512 and layers[0][0].in_channels == cin
            and all(c.out_channels % 16 == 0 and 16 <= c.out_channels <= 256 for c, _ in layers))


def _sources(layers):
    src = []
    for conv, norm in layers:
        src += [conv.weight] + ([conv.bias] if conv.bias is not None else [])
        if norm is not None:
            src += [norm.weight, norm.bias, norm.running_mean, norm.running_var]
    return src


def packed_mlp(owner, key, layers):
    """The images and vectors of `layers`, packed once and cached on `owner` under `key`.  The cache is valid while the tensors it
    was made from are the same objects at the same ``_version`` on the same device: an optimiser step, a train-mode forward (the
    running statistics), ``load_state_dict`` and ``.to()`` all invalidate it.  A writer that goes through raw pointers (no version
    bump) must call ``invalidate_packed(owner)``."""
    src = _sources(layers)
    stamp = tuple(t._version for t in src) + (str(src[0].device),)
    cache = owner.__dict__.setdefault("_packed_mlps", {})
    ent = cache.get(key)
    if ent is not None and ent["stamp"] == stamp and len(ent["src"]) == len(src) and all(a is b for a, b in zip(ent["src"], src)):
        return ent
    dev = src[0].device
    sizes, kin = [], layers[0][0].in_channels
    for conv, _ in layers:
        sizes.append((_pad(kin, 16), _pad(conv.out_channels, 64)))
        kin = conv.out_channels
    buf = torch.empty(sum(k * c + 2 * c for k, c in sizes), dtype=torch.float32, device=dev)
    offsets, off = [], 0
    with torch.no_grad():
        for (conv, norm), (k, c) in zip(layers, sizes):
            wt, sc, sh = buf[off:off + k * c], buf[off + k * c:off + k * c + c], buf[off + k * c + c:off + k * c + 2 * c]
            off += k * c + 2 * c
            w = conv.weight.detach().reshape(conv.out_channels, conv.in_channels).contiguous()
            bn = [t.detach().contiguous() for t in (norm.weight, norm.bias, norm.running_mean, norm.running_var)] if norm is not None \
                else [None] * 4
            bias = conv.bias.detach().contiguous() if conv.bias is not None else None
            L.check(L.lib().vdetr_group_mlp_pack_f32(L.ptr(w), L.ptr(bias), *[L.ptr(t) for t in bn],
                                                     float(norm.eps) if norm is not None else 0.0, conv.in_channels, conv.out_channels,
                                                     L.ptr(wt), L.ptr(sc), L.ptr(sh), L.stream_ptr()), "group_mlp_pack")
            offsets.append((off - k * c - 2 * c, off - 2 * c, off - c))
    ent = {"stamp": stamp, "src": src, "buf": buf, "cin": layers[0][0].in_channels, "widths": [c.out_channels for c, _ in layers],
           "offsets": offsets, "cout": layers[-1][0].out_channels}
    cache[key] = ent
    return ent


def _fill_desc(desc, ent):
    """the MLP part of a launch descriptor from a packed entry (plain numbers in the cache: a module with one still deep-copies)"""
    desc.nlayers, desc.cin = len(ent["widths"]), ent["cin"]
    base = ent["buf"].data_ptr()
    for i, (width, (wt, sc, sh)) in enumerate(zip(ent["widths"], ent["offsets"])):
        desc.width[i] = width
        desc.wt[i], desc.scale[i], desc.shift[i] = base + 4 * wt, base + 4 * sc, base + 4 * sh


def invalidate_packed(module):
    """drop the packed images of `module` and everything below it"""
    for m in module.modules():
        m.__dict__.pop("_packed_mlps", None)


def _dense(t):
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


def _record(owner, paths):
    global LAST_PATHS
    LAST_PATHS = list(paths)
    owner.__dict__["last_paths"] = list(paths)


# ---- set abstraction ------------------------------------------------------------------------------------------------------------
def _sa_fusable(owner, grouper, mlp, xyz, new_xyz, features, pooling="max"):
    if not (FUSED and HD.inference(owner) and pooling == "max" and isinstance(grouper, pointnet2_utils.QueryAndGroup)):
        return None
    if grouper.sample_uniformly or grouper.nsample not in _NSAMPLES or new_xyz is None:
        return None
    if not (_dense(xyz) and _dense(new_xyz) and (features is None or _dense(features))):
        return None
    if features is None and not grouper.use_xyz:
        return None
    B, N, _ = xyz.shape
    M, S = new_xyz.shape[1], grouper.nsample
    C = 0 if features is None else features.shape[1]
    cin = (3 if grouper.use_xyz else 0) + C
    layers = _mlp_layers(mlp)
    if not _mlp_shape_ok(layers, cin):
        return None
    if max(B * M * S, B * max(C, 3) * N, B * 256 * M, B * (cin + 256) * M * S) >= _LIMIT:
        return None
    return layers


def _sa_fused(owner, key, layers, grouper, xyz, new_xyz, features):
    """ball query, then gather + MLP + max as one launch: [B, mlp[-1], npoint]"""
    global FUSED_LAUNCHES
    idx = pointnet2_utils.ball_query(grouper.radius, grouper.nsample, xyz, new_xyz)
    ent = packed_mlp(owner, key, layers)
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    out = torch.empty((B, ent["cout"], M), dtype=torch.float32, device=xyz.device)
    d = L.SaMlpDesc()
    d.B, d.N, d.M, d.S = B, N, M, grouper.nsample
    d.C, d.use_xyz = (0 if features is None else features.shape[1]), int(bool(grouper.use_xyz))
    d.inv_radius = 1.0 / float(grouper.radius) if grouper.normalize_xyz else 1.0
    d.xyz, d.new_xyz, d.idx, d.out = xyz.data_ptr(), new_xyz.data_ptr(), idx.data_ptr(), out.data_ptr()
    d.features = features.data_ptr() if features is not None else None
    _fill_desc(d.mlp, ent)
    L.check(L.lib().vdetr_sa_mlp_max_infer_f32(ctypes.byref(d), L.stream_ptr()), "sa_mlp_max_infer")
    FUSED_LAUNCHES += 1
    return out


def _max_over_samples(x):
    return F.max_pool2d(x, kernel_size=[1, x.size(3)]).squeeze(-1)


def _sample_centres(xyz, npoint, inds=None):
    """(new_xyz [B, npoint, 3] or None, inds): furthest point sampling unless the caller names the centres"""
    if npoint is None:
        return None, inds
    if inds is None:
        inds = pointnet2_utils.furthest_point_sample(xyz, npoint)
    else:
        assert inds.shape[1] == npoint
    flipped = xyz.transpose(1, 2).contiguous()
    return pointnet2_utils.gather_operation(flipped, inds).transpose(1, 2).contiguous(), inds


def _make_scales(group_all, radii, nsamples, mlps, bn, use_xyz, sample_uniformly):
    assert len(radii) == len(nsamples) == len(mlps)
    groupers, nets = nn.ModuleList(), nn.ModuleList()
    for radius, nsample, spec in zip(radii, nsamples, mlps):
        groupers.append(pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz, sample_uniformly=sample_uniformly)
                        if not group_all else pointnet2_utils.GroupAll(use_xyz))
        spec = list(spec)  # a copy: the caller's list stays as it is
        if use_xyz:
            spec[0] += 3
        nets.append(pt_utils.SharedMLP(spec, bn=bn))
    return groupers, nets


def _scales_forward(owner, xyz, new_xyz, features):
    """every scale's max-pooled features [B, mlps[k][-1], npoint], fused where it applies"""
    outs, paths = [], []
    for k, (grouper, mlp) in enumerate(zip(owner.groupers, owner.mlps)):
        layers = _sa_fusable(owner, grouper, mlp, xyz, new_xyz, features)
        if layers is not None:
            outs.append(_sa_fused(owner, k, layers, grouper, xyz, new_xyz, features))
            paths.append("fused")
        else:
            outs.append(_max_over_samples(mlp(grouper(xyz, new_xyz, features))))
            paths.append("composition")
    return outs, paths


class _PointnetSAModuleBase(nn.Module):
    def __init__(self):
        super().__init__()
        self.npoint = None
        self.groupers = None
        self.mlps = None

    def forward(self, xyz, features=None):
        """xyz [B, N, 3], features [B, C, N] or None -> (new_xyz [B, npoint, 3] or None, new_features [B, sum_k mlps[k][-1], npoint])"""
        new_xyz, _ = _sample_centres(xyz, self.npoint)
        outs, paths = _scales_forward(self, xyz, new_xyz, features)
        _record(self, paths)
        return new_xyz, torch.cat(outs, dim=1)


class PointnetSAModuleMSG(_PointnetSAModuleBase):
    """Set abstraction with multi-scale grouping: one ball query, shared MLP and max per (radius, nsample, mlp).
    ``npoint=None`` groups all points (one centre at the origin).  Works on a copy of ``mlps``."""

    def __init__(self, *, npoint, radii, nsamples, mlps, bn=True, use_xyz=True, sample_uniformly=False):
        super().__init__()
        self.npoint = npoint
        self.groupers, self.mlps = _make_scales(npoint is None, radii, nsamples, mlps, bn, use_xyz, sample_uniformly)


class PointnetSAModule(PointnetSAModuleMSG):
    """Set abstraction with one scale.  Works on a copy of ``mlp``."""

    def __init__(self, *, mlp, npoint=None, radius=None, nsample=None, bn=True, use_xyz=True):
        super().__init__(mlps=[mlp], npoint=npoint, radii=[radius], nsamples=[nsample], bn=bn, use_xyz=use_xyz)


class PointnetSAModuleVotes(nn.Module):
    """Set abstraction that also returns the sampled indices: ``(new_xyz, new_features, inds[, unique_cnt])``.
    ``pooling``: "max", "avg" or "rbf" (weights exp(-|d|^2 / (2 sigma^2)) / nsample, sigma = radius / 2 unless given).
    Works on a copy of ``mlp``."""

    def __init__(self, *, mlp, npoint=None, radius=None, nsample=None, bn=True, use_xyz=True, pooling="max", sigma=None,
                 normalize_xyz=False, sample_uniformly=False, ret_unique_cnt=False):
        super().__init__()
        self.npoint, self.radius, self.nsample = npoint, radius, nsample
        self.pooling, self.use_xyz = pooling, use_xyz
        self.sigma = sigma if sigma is not None else (radius / 2 if radius is not None else None)
        self.normalize_xyz, self.ret_unique_cnt = normalize_xyz, ret_unique_cnt
        if npoint is not None:
            self.grouper = pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz, ret_grouped_xyz=True,
                                                         normalize_xyz=normalize_xyz, sample_uniformly=sample_uniformly,
                                                         ret_unique_cnt=ret_unique_cnt)
        else:
            self.grouper = pointnet2_utils.GroupAll(use_xyz, ret_grouped_xyz=True)
        spec = list(mlp)  # a copy: the caller's list stays as it is
        if use_xyz and len(spec) > 0:
            spec[0] += 3
        self.mlp_module = pt_utils.SharedMLP(spec, bn=bn)

    def forward(self, xyz, features=None, inds=None):
        """xyz [B, N, 3], features [B, C, N] or None, inds [B, npoint] int32 or None"""
        new_xyz, inds = _sample_centres(xyz, self.npoint, inds)
        layers = None if self.ret_unique_cnt else _sa_fusable(self, self.grouper, self.mlp_module, xyz, new_xyz, features, self.pooling)
        if layers is not None:
            _record(self, ["fused"])
            return new_xyz, _sa_fused(self, 0, layers, self.grouper, xyz, new_xyz, features), inds
        _record(self, ["composition"])
        grouped = self.grouper(xyz, new_xyz, features)
        unique_cnt = grouped[2] if self.ret_unique_cnt else None
        act = self.mlp_module(grouped[0])  # [B, mlp[-1], npoint, nsample]
        if self.pooling == "max":
            pooled = _max_over_samples(act)
        elif self.pooling == "avg":
            pooled = F.avg_pool2d(act, kernel_size=[1, act.size(3)]).squeeze(-1)
        elif self.pooling == "rbf":
            rbf = torch.exp(-1 * grouped[1].pow(2).sum(1, keepdim=False) / (self.sigma ** 2) / 2)  # [B, npoint, nsample]
            pooled = torch.sum(act * rbf.unsqueeze(1), -1) / float(self.nsample)
        else:
            raise ValueError(f"pooling {self.pooling!r} is not max, avg or rbf")
        if self.ret_unique_cnt:
            return new_xyz, pooled, inds, unique_cnt
        return new_xyz, pooled, inds


class PointnetSAModuleMSGVotes(nn.Module):
    """Multi-scale set abstraction that also returns the sampled indices: ``(new_xyz, new_features, inds)``.
    Works on a copy of ``mlps``."""

    def __init__(self, *, mlps, npoint, radii, nsamples, bn=True, use_xyz=True, sample_uniformly=False):
        super().__init__()
        self.npoint = npoint
        self.groupers, self.mlps = _make_scales(npoint is None, radii, nsamples, mlps, bn, use_xyz, sample_uniformly)

    def forward(self, xyz, features=None, inds=None):
        new_xyz, inds = _sample_centres(xyz, self.npoint, inds)
        outs, paths = _scales_forward(self, xyz, new_xyz, features)
        _record(self, paths)
        return new_xyz, torch.cat(outs, dim=1), inds


# ---- feature propagation --------------------------------------------------------------------------------------------------------
def _fp_fusable(owner, mlp, unknown, known, unknow_feats, known_feats):
    if not (FUSED and HD.inference(owner) and known is not None):
        return None
    if not (_dense(unknown) and _dense(known) and _dense(known_feats) and (unknow_feats is None or _dense(unknow_feats))):
        return None
    B, n, _ = unknown.shape
    m, C2 = known.shape[1], known_feats.shape[1]
    C1 = 0 if unknow_feats is None else unknow_feats.shape[1]
    layers = _mlp_layers(mlp)
    if not _mlp_shape_ok(layers, C1 + C2):
        return None
    if max(B * n * max(C1 + C2, 256), B * C2 * m) >= _LIMIT:
        return None
    return layers


def _three_weights(unknown, known):
    """(idx, weight) [B, n, 3]: the three nearest known points and their normalised reciprocal distances"""
    dist, idx = pointnet2_utils.three_nn(unknown, known)
    dist_recip = 1.0 / (dist + 1e-8)
    norm = torch.sum(dist_recip, dim=2, keepdim=True)
    return idx, dist_recip / norm


class PointnetFPModule(nn.Module):
    """Propagates the features of the `known` points to the `unknown` ones: inverse-distance interpolation over the three nearest,
    concatenation with the unknown points' own features, shared MLP."""

    def __init__(self, *, mlp, bn=True):
        super().__init__()
        self.mlp = pt_utils.SharedMLP(list(mlp), bn=bn)

    def forward(self, unknown, known, unknow_feats, known_feats):
        """unknown [B, n, 3], known [B, m, 3] or None, unknow_feats [B, C1, n] or None, known_feats [B, C2, m] -> [B, mlp[-1], n]"""
        global FUSED_LAUNCHES
        layers = _fp_fusable(self, self.mlp, unknown, known, unknow_feats, known_feats)
        if layers is not None:
            idx, weight = _three_weights(unknown, known)
            ent = packed_mlp(self, 0, layers)
            B, n, _ = unknown.shape
            out = torch.empty((B, ent["cout"], n), dtype=torch.float32, device=unknown.device)
            weight = weight.contiguous()
            d = L.FpMlpDesc()
            d.B, d.n, d.m = B, n, known.shape[1]
            d.C1, d.C2 = (0 if unknow_feats is None else unknow_feats.shape[1]), known_feats.shape[1]
            d.known_feats, d.idx, d.weight, d.out = known_feats.data_ptr(), idx.data_ptr(), weight.data_ptr(), out.data_ptr()
            d.unknow_feats = unknow_feats.data_ptr() if unknow_feats is not None else None
            _fill_desc(d.mlp, ent)
            L.check(L.lib().vdetr_fp_mlp_infer_f32(ctypes.byref(d), L.stream_ptr()), "fp_mlp_infer")
            FUSED_LAUNCHES += 1
            _record(self, ["fused"])
            return out
        _record(self, ["composition"])
        if known is not None:
            idx, weight = _three_weights(unknown, known)
            interpolated = pointnet2_utils.three_interpolate(known_feats, idx, weight)
        else:
            interpolated = known_feats.expand(*known_feats.size()[0:2], unknown.size(1))
        joint = interpolated if unknow_feats is None else torch.cat([interpolated, unknow_feats], dim=1)  # [B, C2 + C1, n]
        return self.mlp(joint.unsqueeze(-1)).squeeze(-1)


# ---- learnable feature propagation ----------------------------------------------------------------------------------------------
_PW_SCALES = 4  # scales per post-MLP launch (vdetr_pw_mlp_desc.pooled)


def _post_fusable(owner, pooled, features2):
    """the post MLP's layers if one launch per four scales can run it on `pooled` (one [B, Ck, n] per scale) and `features2`"""
    if not (FUSED and HD.inference(owner) and pooled):
        return None
    if not (all(_dense(p) for p in pooled) and (features2 is None or _dense(features2))):
        return None
    B, Ck, n = pooled[0].shape
    if any(p.shape != pooled[0].shape for p in pooled) or B * n == 0:
        return None
    C2 = 0
    if features2 is not None:
        if features2.dim() != 3 or features2.shape[0] != B or features2.shape[2] != n or features2.shape[1] == 0:
            return None
        C2 = features2.shape[1]
    layers = _mlp_layers(owner.post_mlp)
    if not _mlp_shape_ok(layers, Ck + C2):
        return None
    if max(B * max(Ck, C2) * n, len(pooled) * B * layers[-1][0].out_channels * n) >= _LIMIT:
        return None
    return layers


def _post_fused(owner, layers, pooled, features2):
    """concat(pooled_k, features2) -> post MLP for every scale k, written to its channel slice: [B, K post_mlp[-1], n]"""
    global FUSED_LAUNCHES
    ent = packed_mlp(owner, "post", layers)
    B, Ck, n = pooled[0].shape
    K, P = len(pooled), ent["cout"]
    out = torch.empty((B, K * P, n), dtype=torch.float32, device=pooled[0].device)
    for k0 in range(0, K, _PW_SCALES):
        chunk = pooled[k0:k0 + _PW_SCALES]
        d = L.PwMlpDesc()
        d.B, d.n, d.K, d.Ck = B, n, len(chunk), Ck
        d.C2 = 0 if features2 is None else features2.shape[1]
        d.out_channels, d.out_channel0 = K * P, k0 * P
        for j, p in enumerate(chunk):
            d.pooled[j] = p.data_ptr()
        d.features2 = features2.data_ptr() if features2 is not None else None
        d.out = out.data_ptr()
        _fill_desc(d.mlp, ent)
        L.check(L.lib().vdetr_pw_mlp_infer_f32(ctypes.byref(d), L.stream_ptr()), "pw_mlp_infer")
        FUSED_LAUNCHES += 1
    return out


class PointnetLFPModuleMSG(nn.Module):
    """Learnable feature propagation: a multi-scale set abstraction of (xyz1, features1) around the GIVEN centres xyz2, then the
    same ``post_mlp`` on ``concat(pooled_k, features2)`` once per scale, the results concatenated over the scales.  ``post_mlp`` is
    registered before ``groupers`` / ``mlps`` (the reference's state-dict order); in train mode its BatchNorm sees one batch per
    scale.  ``last_paths``: one entry per scale, then one for the post MLP.  Works on a copy of ``mlps`` and ``post_mlp``."""

    def __init__(self, *, mlps, radii, nsamples, post_mlp, bn=True, use_xyz=True, sample_uniformly=False):
        super().__init__()
        self.post_mlp = pt_utils.SharedMLP(list(post_mlp), bn=bn)
        self.groupers, self.mlps = _make_scales(False, radii, nsamples, mlps, bn, use_xyz, sample_uniformly)

    def forward(self, xyz2, xyz1, features2, features1):
        """xyz2 [B, N2, 3] (the centres), xyz1 [B, N1, 3], features2 [B, C2, N2] or None, features1 [B, C1, N1]
        -> [B, len(mlps) * post_mlp[-1], N2]"""
        pooled, paths = _scales_forward(self, xyz1, xyz2, features1)
        layers = _post_fusable(self, pooled, features2)
        if layers is not None:
            out = _post_fused(self, layers, pooled, features2)
            _record(self, paths + ["fused"])
            return out
        _record(self, paths + ["composition"])
        outs = []
        for p in pooled:  # one call per scale: in train mode the BatchNorm's statistics are each call's own
            joint = p if features2 is None else torch.cat([p, features2], dim=1)  # [B, mlps[k][-1] + C2, N2]
            outs.append(self.post_mlp(joint.unsqueeze(-1)))
        return torch.cat(outs, dim=1).squeeze(-1)
