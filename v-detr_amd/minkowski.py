"""The slice of MinkowskiEngine's module API that the reference's backbone uses (models/mink_resnet.py:4-5,38-84;
models/model_vdetr.py:8,139-185,248-280), on the MI355X sparse primitives of ``sparse_ops``.

Same class names, constructor arguments, parameter names / shapes (``MinkowskiConvolution.kernel [K, Cin, Cout]``,
``MinkowskiBatchNorm.bn.*``) so that the reference's ``pre_encoder.* / up_block_*.* / out_block_0.*`` checkpoint keys load.
MinkowskiEngine is NOT under /root/reference (un-vendored): semantics follow its published operator and documentation —
  * kernel offsets of a hypercubic region: odd sizes centred (-1, 0, 1), even sizes 0 .. k-1, in units of the INPUT tensor
    stride; kernel index = ix + k * (iy + k * iz) (first spatial dimension fastest);
  * a strided convolution writes the sites floor(c / s_out) * s_out of its input sites (tensor stride multiplied);
  * a transposed convolution with stride 2 divides the tensor stride; ``MinkowskiConvolutionTranspose`` writes the sites
    that already exist at that stride in the coordinate manager, ``MinkowskiGenerativeConvolutionTranspose`` generates
    every child site;
  * kernels other than the cube (``RegionType``, ``KernelGenerator``: cross, custom, dilation), the pooling layers and
    ``MinkowskiInstanceNorm`` serve the reference's module library (models/modules/, here ``vdetr_amd.modules``): DESIGN 6.10 says
    which of their conventions (the cross's offset order, ``MinkowskiAvgUnpooling``) are this package's own;
  * ``a + b`` / ``a - b`` of tensors on DIFFERENT key sets (the skip add behind a generative convolution) live on the union of the
    sites, a side without a site counting as zero; ``MinkowskiUnion`` folds ``+``; ``MinkowskiPruning`` keeps the rows of a bool
    mask in order (this package's own statement);
  * duplicated input coordinates keep one feature row (here: the first in input order) under the default
    ``SparseTensorQuantizationMode.RANDOM_SUBSAMPLE``; UNWEIGHTED_AVERAGE / UNWEIGHTED_SUM / MAX_POOL fold the rows of a site in
    ascending input order; sites are held in key order, which is also the row order of ``sparse_quantize``;
  * ``MinkowskiInterpolation`` / ``features_at_coordinates`` / ``SparseTensor.interpolate`` read a tensor of any stride at float
    coordinates: trilinear over the 2^3 sites around a point, a site's feature AT its integer coordinate, absent sites as zero
    without renormalisation (this package's own statement);
  * ``MinkowskiGlobal*Pooling`` write one row per scene of the batch on the origin map (keys (b, 0, 0, 0), ``tensor_stride`` 0; a scene
    without a site keeps a zero row), ``MinkowskiBroadcast*`` bring such rows back to the sites, ``MinkowskiLinear`` and the pointwise
    layers take either kind of tensor (this package's own statement);
  * ``expand_coordinates=True`` in a convolution's or pooling's constructor writes every site the kernel reaches from an input site
    (exactly the sites whose row of the kernel map is not empty); ``forward(x, coordinates)`` writes the sites the caller gives, a
    SparseTensor's, a key tensor's or an integer [M, 4] list's, in key order with ``inverse_mapping`` back to the list (DESIGN 6.19:
    this package's own statement).
The ORDER of the sites of a MinkowskiEngine tensor is an implementation detail of its hash map; here it is ascending
(batch, x, y, z).  Parity against the MinkowskiEngine binary is unpinned; ``oracle/sparse_oracle.py`` pins the arithmetic
against torch's dense convolutions.
"""
import enum
import math
import threading

import numpy as np
import torch
import torch.nn as nn

from . import heads as HD
from . import sparse_ops as S

# Inference (``heads.inference``: eval mode, autograd off): a convolution -> BatchNorm -> activation site is TWO launches, the
# pair GEMM and a gather-sum that finishes the row (sparse_ops.gather_sum_bn_act), instead of GEMM, gather-sum,
# (bias add,) BatchNorm pass(, skip add).  ``INFER_FUSED = False`` keeps the composition (A/B runs, parity tests).
INFER_FUSED = True
LAST_PATHS = []  # "fused" / "composition" per convolution -> BatchNorm site of the last forward (cleared by MinkResNet.forward / backbone_forward)


def clear_last_paths():
    if not _geometry_only():  # (a loader thread's geometry pass runs beside the training thread's forward)
        del LAST_PATHS[:]


def _record_path(path):
    if len(LAST_PATHS) >= 4096:  # (sites driven in a loop without either forward above: keep the record bounded)
        del LAST_PATHS[:]
    LAST_PATHS.append(path)


def _conv_bn_fusable(module, feats, plan=None, cout=None, bn=None):
    """The gate of the fused inference form, asked twice per site: by the convolution (``plan``, ``cout``: may its pair products
    stay un-summed?) and by the BatchNorm that receives them (``bn``: can it finish them in the fused launch?).  Everything
    else — training, autograd, SyncBatchNorm / no running statistics, CPU tensors, the plan / im2col modes — takes the
    composition of launches, unchanged."""
    if not (INFER_FUSED and HD.inference(module)) or _geometry_only():
        return False
    if plan is not None:
        if not (isinstance(plan, S.PairPlan) and feats.is_cuda and feats.dtype == torch.float32 and feats.is_contiguous()):
            return False
        width = cout + (-cout) % 16
        if cout % 4 or max(feats.numel(), plan.K * plan.nout, plan.nout * width, plan.P * width) >= 2 ** 31:
            return False
    if bn is not None:
        if type(bn) is not nn.BatchNorm1d or bn.running_mean is None or bn.running_var is None:
            return False
        if not all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)):
            return False
    return True


# Geometry-only pass (ModelVDETR.prepare_geometry): convolutions build their sites / kernel maps / pair lists and hand on an
# UNINITIALISED feature table of the right shape; every other layer is the identity.  Nothing is computed on features.
# The switch is per THREAD: a loader thread prepares the next scene while the training thread runs the model.
_tls = threading.local()


def _geometry_only():
    return getattr(_tls, "geometry_only", False)


class geometry_only:
    def __enter__(self):
        self._prev, _tls.geometry_only = _geometry_only(), True

    def __exit__(self, *exc):
        _tls.geometry_only = self._prev


def _region_offsets(kernel_size):
    r = range(-(kernel_size // 2), kernel_size // 2 + 1) if kernel_size % 2 else range(kernel_size)
    return [(x, y, z) for z in r for y in r for x in r]  # x fastest


class RegionType(enum.Enum):
    """ME.RegionType: the shape of a kernel's neighbourhood"""
    HYPER_CUBE = 0
    HYPER_CROSS = 1
    CUSTOM = 2


def _triple(value, name):
    if isinstance(value, (int, np.integer)):
        return (int(value),) * 3
    value = tuple(int(v) for v in value)
    if len(value) != 3:
        raise NotImplementedError(f"{name} {value}: three spatial dimensions only")
    return value


def _axis_range(k):
    return range(-(k // 2), k // 2 + 1) if k % 2 else range(k)


class KernelGenerator:
    """ME.KernelGenerator for three spatial dimensions: the offsets of a kernel, in a FIXED order (``kernel[k]`` of a checkpoint
    belongs to ``offsets[k]``), in units of dilation x tensor stride:
      HYPER_CUBE   ``_region_offsets`` per axis, x fastest: an odd size k covers -(k//2) .. k//2, an even size 0 .. k-1;
      HYPER_CROSS  odd sizes only: the centre, then for axis x, y, z and distance d = 1 .. k//2: -d, then +d (volume
                   1 + sum(k_a - 1); this order is this package's own, MinkowskiEngine's is not pinned: DESIGN 6.10);
      CUSTOM       ``region_offsets`` [K, 3] as given.
    ``stride > 1`` together with ``dilation > 1`` raises ValueError."""

    def __init__(self, kernel_size=-1, stride=1, dilation=1, is_transpose=False, region_type=RegionType.HYPER_CUBE,
                 region_offsets=None, expand_coordinates=False, axis_types=None, dimension=-1):
        if dimension != 3:
            raise NotImplementedError(f"KernelGenerator: dimension {dimension} (three spatial dimensions only)")
        if axis_types is not None:
            axis_types = list(axis_types)
            if len(axis_types) != 3 or any(a != axis_types[0] for a in axis_types):
                raise NotImplementedError("KernelGenerator: mixed axis_types (one region type for all three axes only)")
            region_type = axis_types[0]
        self.region_type = RegionType(region_type) if not isinstance(region_type, RegionType) else region_type
        self.kernel_size, self.kernel_stride = _triple(kernel_size, "kernel_size"), _triple(stride, "stride")
        self.kernel_dilation = _triple(dilation, "dilation")
        self.is_transpose, self.expand_coordinates, self.axis_types, self.dimension = is_transpose, expand_coordinates, axis_types, 3
        if max(self.kernel_stride) > 1 and max(self.kernel_dilation) > 1:
            raise ValueError(f"KernelGenerator: stride {self.kernel_stride} together with dilation {self.kernel_dilation}")
        if min(self.kernel_stride) < 1 or min(self.kernel_dilation) < 1:
            raise ValueError("KernelGenerator: stride and dilation must be positive")
        ks = self.kernel_size
        if self.region_type is RegionType.CUSTOM:
            if region_offsets is None:
                raise ValueError("KernelGenerator: RegionType.CUSTOM needs region_offsets [K, 3]")
            rows = region_offsets.tolist() if hasattr(region_offsets, "tolist") else region_offsets
            self.offsets = [tuple(int(v) for v in row) for row in rows]
            if not self.offsets or any(len(o) != 3 for o in self.offsets):
                raise ValueError("KernelGenerator: region_offsets must be [K, 3] with K >= 1")
        elif min(ks) < 1:
            raise ValueError(f"KernelGenerator: kernel_size {ks} must be positive")
        elif self.region_type is RegionType.HYPER_CUBE:
            self.offsets = [(x, y, z) for z in _axis_range(ks[2]) for y in _axis_range(ks[1]) for x in _axis_range(ks[0])]
        else:
            if any(k % 2 == 0 for k in ks):
                raise ValueError(f"KernelGenerator: a HYPER_CROSS region needs odd sizes, not {ks}")
            self.offsets = [(0, 0, 0)]
            for axis in range(3):
                for d in range(1, ks[axis] // 2 + 1):
                    for sign in (-1, 1):
                        self.offsets.append(tuple(sign * d if a == axis else 0 for a in range(3)))
        self.kernel_volume = len(self.offsets)

    def scaled_offsets(self):
        """the offsets times the dilation, per axis: what a kernel map multiplies by the tensor stride"""
        d = self.kernel_dilation
        return tuple((x * d[0], y * d[1], z * d[2]) for x, y, z in self.offsets)


class _Offsets(tuple):
    """offsets already in the canonical form (a tuple of int 3-tuples), hashed once: what the layers hand to the coordinate manager
    at every forward (equal to, and hashing like, the plain tuple of the same offsets)"""

    def __new__(cls, offsets):
        self = super().__new__(cls, offsets)
        self._hash = tuple.__hash__(self)
        return self

    def __hash__(self):
        return self._hash


def _kernel_offsets(kernel):
    """what ``CoordinateManager.kernel_map`` / ``generated`` accept as a kernel -> its offsets as a tuple of 3-tuples: a
    KernelGenerator, a cube's size (an int or one size per axis), or the offsets themselves"""
    if isinstance(kernel, _Offsets):
        return kernel
    if isinstance(kernel, KernelGenerator):
        return kernel.scaled_offsets()
    if isinstance(kernel, (int, np.integer)):
        return tuple(_region_offsets(int(kernel)))
    kernel = tuple(kernel)
    if kernel and isinstance(kernel[0], (tuple, list)):
        return tuple(tuple(int(v) for v in o) for o in kernel)
    return KernelGenerator(kernel, dimension=3).scaled_offsets()


class SparseTensorQuantizationMode(enum.Enum):
    """ME.SparseTensorQuantizationMode: what becomes of the feature rows of points that share a voxel"""
    RANDOM_SUBSAMPLE = 0            # one row per site: here the first in input order
    UNWEIGHTED_AVERAGE = 1
    UNWEIGHTED_SUM = 2
    NO_QUANTIZATION = 3             # not built
    MAX_POOL = 4
    SPLAT_LINEAR_INTERPOLATION = 5  # not built


_VOXEL_MODE = {SparseTensorQuantizationMode.RANDOM_SUBSAMPLE: "first", SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE: "average",
               SparseTensorQuantizationMode.UNWEIGHTED_SUM: "sum", SparseTensorQuantizationMode.MAX_POOL: "max"}


def _quantization_mode(mode):
    """a SparseTensorQuantizationMode, or its name in either case ("unweighted_average": args.quantization_mode) -> the member;
    the two modes that are not built raise NotImplementedError"""
    if isinstance(mode, str):
        try:
            mode = SparseTensorQuantizationMode[mode.upper()]
        except KeyError:
            raise ValueError(f"quantization_mode {mode!r}: one of {[m.name.lower() for m in SparseTensorQuantizationMode]}") from None
    mode = SparseTensorQuantizationMode(mode)
    if mode not in _VOXEL_MODE:
        raise NotImplementedError(f"SparseTensorQuantizationMode.{mode.name} is not built: RANDOM_SUBSAMPLE, UNWEIGHTED_AVERAGE, "
                                  "UNWEIGHTED_SUM and MAX_POOL are")
    return mode


def _quantized_features(features, cm, mode):
    """the feature rows of the sites that ``cm.insert_points`` / ``insert_cloud`` made of the points behind ``features``"""
    if mode is SparseTensorQuantizationMode.RANDOM_SUBSAMPLE:
        return features[cm.unique_index]  # one row per site, in site (key) order
    if cm.voxel_map is None:
        S.L.require_gpu(features, "features")
    return S.voxel_reduce(features.contiguous(), cm.voxel_map, _VOXEL_MODE[mode])


class CoordinateManager:
    """Sites per tensor stride + cached kernel maps of one batch (geometry only: no gradients flow through it)."""

    def __init__(self, device):
        self.device = device
        self.keys = {}    # tensor_stride -> canonical sorted int64 keys of that stride
        self.maps = {}    # (in key set, out key set, strides, kernel offsets, transposed) -> (nbr [K,Nout], inv [K,Nin], plan)
        self.num_scenes = None  # batch size: read once, with the coordinate range, when the points are inserted
        self.voxel_map = None   # sparse_ops.VoxelMap of the inserted points (device tensors)

    def _take_voxel_map(self, vmap):
        self.voxel_map = vmap
        self.num_scenes = vmap.num_scenes
        self.keys[1], self.unique_index, self.inverse_mapping = vmap.sites, vmap.first, vmap.inverse

    def insert_cloud(self, points, offsets, voxel_size):
        """packed raw points [N, >= 3] fp32 on the device and their B + 1 scene offsets -> the sites of tensor stride 1, as
        ``insert_points`` of ``batch_sparse_collate`` of the scenes' ``p[:, :3] / voxel_size`` makes them (sparse_ops.voxel_map)"""
        self._take_voxel_map(S.voxel_map(points, offsets, voxel_size))

    def insert_points(self, coordinates):
        """raw integer coordinates [N,4] -> the sites of tensor stride 1 (+ ``unique_index``: the input row kept per site:
        the first occurrence in input order; MinkowskiEngine: RANDOM_SUBSAMPLE; ``inverse_mapping``: the site row of every input
        row).  Device tensors: sparse_ops.voxel_map_coords, one host read.  CPU tensors (geometry passes of the CPU tests):
        the tensor expressions the device path is tested against."""
        if coordinates.is_cuda and not coordinates.is_floating_point():
            return self._take_voxel_map(S.voxel_map_coords(coordinates))
        keys_in = S.pack_keys(coordinates)
        # (pack_keys has just read the coordinate range back: the one place where the scene count may be read as well)
        self.num_scenes = int(coordinates[:, 0].max()) + 1 if coordinates.shape[0] else 0
        keys, inverse = torch.unique(keys_in, return_inverse=True)
        first = torch.full((keys.shape[0],), keys_in.shape[0], dtype=torch.int64, device=keys.device)
        first.scatter_reduce_(0, inverse, torch.arange(keys_in.shape[0], device=keys.device), reduce="amin")
        self.keys[1] = keys
        self.unique_index = first
        self.inverse_mapping = inverse.to(torch.int32)

    @staticmethod
    def _strided_keys(keys, new_ts):
        c = S.unpack_keys(keys).to(torch.int64)
        c[:, 1:] = torch.div(c[:, 1:], new_ts, rounding_mode="floor") * new_ts
        return torch.unique(S.pack_keys(c, check=False))

    def strided(self, keys, ts, new_ts):
        """sites of a strided convolution's output.  The sites derived from the canonical set of stride `ts` become the
        canonical set of stride `new_ts` (what later transposed convolutions / skip connections land on)."""
        if keys is self.keys.get(ts):
            if new_ts not in self.keys:
                self.keys[new_ts] = self._strided_keys(keys, new_ts)
            return self.keys[new_ts]
        return self._strided_keys(keys, new_ts)

    def generated(self, keys, new_ts, kernel_size):
        """children of every site (generative transposed convolution): a NEW, non-canonical key set at stride `new_ts`.
        ``kernel_size``: anything ``_kernel_offsets`` takes.  Cached per (key set, stride, offsets), so that the forward pass
        after a ``prepare_geometry`` meets the key tensors its maps were built for."""
        region = _kernel_offsets(kernel_size)
        cache = self.__dict__.setdefault("_generated", {})
        key = (keys.data_ptr(), new_ts, region)
        if key not in cache:
            c = S.unpack_keys(keys).to(torch.int64)
            off = torch.tensor(region, dtype=torch.int64, device=c.device) * new_ts
            child = c[:, None, :].repeat(1, off.shape[0], 1)
            child[:, :, 1:] += off[None]
            cache[key] = (torch.unique(S.pack_keys(child.reshape(-1, 4))), keys)  # the parent key tensor is kept alive
        return cache[key][0]

    def expanded(self, keys, ts, out_ts, kernel_size, transposed):
        """the sites of an expanding layer (``expand_coordinates=True``): every site u of the output lattice whose row of
        the kernel map is not empty.  Not transposed (stride 1): u = v - offset * ts over the input sites v — the MINUS of the map's
        u + offset * ts = v; transposed: u = v + offset * out_ts, the children of ``generated``.  One candidates launch, the sort and
        the sites pass of ``sparse_ops.region_keys``, one host read.  A NEW, non-canonical key set, never written into ``self.keys``;
        cached per (key set, strides, offsets, transposed) like the generated ones."""
        region = _kernel_offsets(kernel_size)
        cache = self.__dict__.setdefault("_expanded", {})
        key = (keys.data_ptr(), ts, out_ts, region, transposed)
        if key not in cache:
            reg = torch.tensor(region, dtype=torch.int32)
            offsets = (reg * out_ts if transposed else -reg * ts).to(keys.device)
            cache[key] = (S.region_keys(keys, offsets), keys)  # the parent key tensor is kept alive
        return cache[key][0]

    def targets(self, coordinates):
        """(keys, inverse) of ``sparse_ops.target_keys`` for caller-chosen output sites [M, 4] (``forward(x, coordinates)``), cached
        per coordinate tensor and its version, bounded like the interpolation maps: it is geometry, and its size is read back once"""
        cache = self.__dict__.setdefault("_targets", {})
        key = (coordinates.data_ptr(), tuple(coordinates.shape), coordinates.dtype, coordinates._version)
        if key not in cache:
            if len(cache) >= 64:  # (coordinate tensors made anew for every call: keep the record bounded)
                cache.clear()
            cache[key] = S.target_keys(coordinates) + (coordinates,)  # the tensor is kept alive
        return cache[key][:2]

    def union_map(self, a_keys, b_keys):
        """(u, row_a, row_b, src_a, src_b) of ``sparse_ops.union_map`` for two key sets of one stride: the sites of
        ``a + b`` on different coordinate maps.  Cached per pair of key tensors: it is geometry, and its size is read back once."""
        cache = self.__dict__.setdefault("_union_maps", {})
        key = (a_keys.data_ptr(), b_keys.data_ptr())
        if key not in cache:
            cache[key] = S.union_map(a_keys, b_keys) + (a_keys, b_keys)  # key tensors kept alive
        return cache[key][:5]

    def kernel_map(self, in_keys, out_keys, in_ts, out_ts, kernel_size, transposed):
        """(nbr, inv, plan) of a kernel (``_kernel_offsets``: a cube's size, a KernelGenerator or the offsets) between two key
        sets.  Cached on the OFFSETS: a cube and a cross of one size do not share a plan, a pooling and a convolution of one
        geometry do."""
        region = _kernel_offsets(kernel_size)
        key = (in_keys.data_ptr(), out_keys.data_ptr(), in_ts, out_ts, region, transposed)
        if key not in self.maps:
            reg = torch.tensor(region, dtype=torch.int32)
            # convolution: output site u reads u + offset * in_stride; transposed: the output (fine) site v = u + offset *
            # out_stride of the input (coarse) site u reads v - offset * out_stride
            offsets = (reg * in_ts if not transposed else -reg * out_ts).to(self.device)
            nbr = S.kernel_map(in_keys, out_keys, offsets)
            pairs = not S._IM2COL and S._MODE == "pairs"
            inv = None if pairs else S.inverse_map(nbr, in_keys.shape[0])  # (the pair lists carry their own inverse: islot)
            plan = None if S._IM2COL else (S.PairPlan if pairs else S.ConvPlan)(nbr, in_keys.shape[0])
            self.maps[key] = (nbr, inv, plan, in_keys, out_keys)  # key tensors kept alive
        return self.maps[key][:3]

    def pool_map(self, in_keys, out_keys, in_ts, out_ts, kernel_size, transposed):
        """(nbr, inv) of ``kernel_map`` for a pooling: the same cached map, with the inverse map that the pair path of the
        convolutions does not keep built on first use"""
        nbr, inv, _ = self.kernel_map(in_keys, out_keys, in_ts, out_ts, kernel_size, transposed)
        if inv is None:
            cache = self.__dict__.setdefault("_pool_inverse", {})
            key = (nbr.data_ptr(), in_keys.shape[0])
            if key not in cache:
                cache[key] = (S.inverse_map(nbr, in_keys.shape[0]), nbr)
            inv = cache[key][0]
        return nbr, inv

    def scene_segments(self, keys):
        """(seg [nseg + 1] int32 on the device, nseg): scene s of a key set is the rows seg[s] .. seg[s+1].  Cached per key set;
        computed on the device.  nseg is the count read when the points were inserted (a manager filled by hand reads it here,
        once)."""
        cache = self.__dict__.setdefault("_scene_segments", {})
        key = keys.data_ptr()
        if key not in cache:
            if self.num_scenes is None:
                self.num_scenes = int(S.key_batch(keys[-1])) + 1 if keys.numel() else 0
            cache[key] = (S.scene_segments(keys, self.num_scenes), keys)
        return cache[key][0], self.num_scenes

    def origin_keys(self):
        """the keys of the origin map: one site (b, 0, 0, 0) per scene 0 .. num_scenes - 1, in order — where a global pooling
        writes its rows (``tensor_stride`` 0 marks them).  Built on the device once the scene count is known."""
        assert self.num_scenes is not None, "origin_keys: the scene count is not known yet (scene_segments reads it)"
        if 0 not in self.keys:
            self.keys[0] = S.origin_keys(self.num_scenes, self.device)
        return self.keys[0]

    def scene_counts(self, keys):
        """sites per batch element of a key set, as a host list.  Cached per key set: it is geometry, and reading it back is a
        host synchronisation that must not sit between the backbone's forward launches and what follows them (measured: the
        host then waits for the whole forward pass, 12 ms per step at 40k points, before it can enqueue the decoder)."""
        cache = self.__dict__.setdefault("_scene_counts", {})
        key = keys.data_ptr()
        if key not in cache:
            b = S.key_batch(keys)
            nb = int(b.max()) + 1 if b.numel() else 0
            # (a key set from which MinkowskiPruning took a whole scene still has one entry per scene of the batch)
            nb = max(nb, self.num_scenes or 0)
            cache[key] =(torch.bincount(b, minlength=nb).tolist(), keys)  # the key tensor is kept alive with its entry
        return cache[key][0]

    def device_tensors(self):
        """every device tensor this manager holds, directly or through its cached plans (sites, kernel maps, pair lists,
        tile tables ...)"""
        seen, stack, out = set(), [self], []
        while stack:
            o = stack.pop()
            if id(o) in seen:
                continue
            seen.add(id(o))
            if torch.is_tensor(o):
                if o.is_cuda:
                    out.append(o)
            elif isinstance(o, dict):
                stack.extend(o.values())
            elif isinstance(o, (list, tuple, set)):
                stack.extend(o)
            elif hasattr(o, "__dict__") and not isinstance(o, (type, torch.nn.Module)):
                stack.extend(vars(o).values())
        return out

    def use_on(self, stream=None):
        """Tell the caching allocator that `stream` (default: the current one) reads this manager's tensors.  A manager
        built by ``prepare_geometry`` on a loader stream is consumed by forward and backward kernels of the training
        stream; without this, dropping the manager lets the allocator hand its blocks to the loader stream's next scene
        while those kernels are still queued.  Idempotent per stream; plans added later are picked up on the next call."""
        stream = stream or torch.cuda.current_stream()
        if torch.cuda.is_current_stream_capturing():
            return self
        # keyed by storage + stream (views of one buffer are one allocator block), and the memo HOLDS a tensor of every
        # recorded storage: while it does, the address cannot be handed to a new allocation that would then be skipped
        # and have its block recycled under the training stream's kernels
        done = self.__dict__.setdefault("_recorded", {})
        for t in self.device_tensors():
            key = (t.untyped_storage().data_ptr(), stream.cuda_stream)
            if key not in done:
                t.record_stream(stream)
                done[key] = t
        return self

    def finalize(self):
        """wait for the pair counts of every plan built so far (one synchronisation for the whole scene)"""
        for entry in self.maps.values():
            if hasattr(entry[2], "finalize"):
                entry[2].finalize()
        return self


class _PendingConv:
    """The pair products y [P, Cout padded to 16] of a convolution (None: the layer has no pair) with the rest of its forward
    still to run: the gather-sum over ``slot`` [K, Nout], the cut to ``channels`` and the ``bias`` add."""
    __slots__ = ("y", "slot", "channels", "bias")

    def __init__(self, y, slot, channels, bias):
        self.y, self.slot, self.channels, self.bias = y, slot, channels, bias

    def materialise(self):
        """what MinkowskiConvolution.forward computes without the hand-over, op for op"""
        width = self.channels + (-self.channels) % 16
        if self.y is None:
            f = torch.zeros((self.slot.shape[1], width), dtype=torch.float32, device=self.slot.device)
        else:
            f = S.gather_sum(self.y, self.slot, flat=True)
        if width != self.channels:
            f = f[:, :self.channels]
        return f if self.bias is None else f + self.bias


class SparseTensor:
    """features [N, C] on the sites ``coordinates`` [N, 4] = (batch, x, y, z) (MinkowskiEngine's SparseTensor)."""

    def __init__(self, features, coordinates=None, tensor_stride=1, coordinate_manager=None, keys=None,
                 quantization_mode=SparseTensorQuantizationMode.RANDOM_SUBSAMPLE):
        self.quantization_mode = _quantization_mode(quantization_mode)
        self.unique_index = self.inverse_mapping = None
        if coordinate_manager is None:
            assert coordinates is not None and tensor_stride == 1
            coordinate_manager = CoordinateManager(features.device)
            coordinate_manager.insert_points(coordinates)
            features = _quantized_features(features, coordinate_manager, self.quantization_mode)
            self.unique_index, self.inverse_mapping = coordinate_manager.unique_index, coordinate_manager.inverse_mapping
        self._F, self._pending = features, None
        self.tensor_stride = tensor_stride
        self.coordinate_manager = coordinate_manager
        self.keys = keys if keys is not None else coordinate_manager.keys[tensor_stride]

    @classmethod
    def pending(cls, conv, tensor_stride, coordinate_manager, keys):
        """the output of a convolution under inference whose gather-sum has not run: ``conv`` (_PendingConv) is finished by the
        MinkowskiBatchNorm that receives this tensor, or summed by whatever else reads ``.F``"""
        out = cls(None, tensor_stride=tensor_stride, coordinate_manager=coordinate_manager, keys=keys)
        out._pending = conv
        return out

    @property
    def F(self):
        if self._pending is not None:
            self._F, self._pending = self._pending.materialise(), None
        return self._F

    @F.setter
    def F(self, features):
        self._F, self._pending = features, None

    @property
    def C(self):
        return S.unpack_keys(self.keys)

    @property
    def device(self):
        return self.keys.device if self._pending is not None else self._F.device

    def _like(self, features):
        return SparseTensor(features, tensor_stride=self.tensor_stride, coordinate_manager=self.coordinate_manager, keys=self.keys)

    def _same_map(self, other):
        return self.keys is other.keys or torch.equal(self.keys, other.keys)

    def _on_union(self, other, sign):
        """self + sign * other on DIFFERENT key sets: the result lives on the union of the two, in key order; a side without a
        site contributes zero.  Geometry-only: the union map is built and cached, the table is uninitialised."""
        cm, ts = self.coordinate_manager, self.tensor_stride
        if other.coordinate_manager is not cm:
            raise ValueError(f"sparse tensors of different coordinate managers: {cm!r} and {other.coordinate_manager!r}")
        if other.tensor_stride != ts:
            raise ValueError(f"sparse tensors of different tensor strides: {ts} and {other.tensor_stride}")
        ca, cb = self.F.shape[1], other.F.shape[1]
        if ca != cb:
            raise ValueError(f"sparse tensors of different channel counts: {ca} and {cb}")
        u, row_a, row_b, src_a, src_b = cm.union_map(self.keys, other.keys)
        if _geometry_only():
            f = self.F.new_empty((u.shape[0], ca))
        else:
            f = S.union_add(self.F.contiguous(), other.F.contiguous(), row_a, row_b, src_a, src_b, sign)
        return SparseTensor(f, tensor_stride=ts, coordinate_manager=cm, keys=u)

    def __add__(self, other):
        if not self._same_map(other):
            return self._on_union(other, 1)
        return self if _geometry_only() else self._like(self.F + other.F)

    def __sub__(self, other):
        if not self._same_map(other):
            return self._on_union(other, -1)
        return self if _geometry_only() else self._like(self.F - other.F)

    def slice(self, field):
        """ME.SparseTensor.slice: this tensor's features on the points of ``field`` (a TensorField whose ``sparse()`` made this
        tensor's sites) -> a TensorField with F = self.F[field.inverse_mapping].  One gather launch; its backward is the sum of
        the point gradients of every site in ascending input-row order."""
        if not isinstance(field, TensorField):
            raise ValueError(f"slice: a TensorField is expected, not {type(field).__name__}")
        if field.coordinate_manager is not self.coordinate_manager or field._vmap is None:
            raise ValueError("slice: the field must be the one whose sparse() built this tensor's coordinate manager")
        if self.tensor_stride != 1 or self.keys is not self.coordinate_manager.keys[1]:
            raise ValueError("slice: only a tensor on the field's own sites (tensor stride 1) can be sliced")
        return field._like(S.voxel_slice(self.F.contiguous(), field._vmap))

    def cat_slice(self, field):
        """ME.SparseTensor.cat_slice: ``slice(field)`` with the field's own features behind it, F = cat((self.F[inverse], field.F),
        1) — the site features first: that column order is this package's definition.  Preconditions and errors of ``slice``."""
        sliced = self.slice(field)
        return field._like(torch.cat((sliced.F, field.F), 1))

    def _interp_map(self, tfield):
        """the InterpMap of this tensor's keys at ``tfield`` [N, 4] fp32 (batch, x, y, z), cached in the coordinate manager per
        (key set, stride, coordinate tensor and its version): it is geometry, built once by a geometry-only pass"""
        cache = self.coordinate_manager.__dict__.setdefault("_interp_maps", {})
        key = (self.keys.data_ptr(), self.tensor_stride, tfield.data_ptr(), tuple(tfield.shape), tfield._version)
        if key not in cache:
            if len(cache) >= 64:  # (query tensors made anew for every call: keep the record bounded)
                cache.clear()
            cache[key] = (S.interp_map(self.keys, self.tensor_stride, tfield), self.keys, tfield)  # the tensors are kept alive
        return cache[key][0]

    def features_at_coordinates(self, query_coordinates):
        """ME.SparseTensor.features_at_coordinates: [N, C] = this tensor's features interpolated trilinearly at
        ``query_coordinates`` [N, 4] fp32 (batch, x, y, z) in units of the finest voxel, at any tensor stride (a
        site's feature sits at its integer coordinate; corners without a site count as zero, without renormalisation).
        Gradients reach the features, not the coordinates."""
        return MinkowskiInterpolation()(self, query_coordinates)

    def interpolate(self, field):
        """ME.SparseTensor.interpolate: ``features_at_coordinates`` at the float coordinates of ``field`` -> a TensorField on
        them.  Only this tensor's keys are used: any tensor stride, the field's own coordinate manager or another."""
        if not isinstance(field, TensorField):
            raise ValueError(f"interpolate: a TensorField is expected, not {type(field).__name__}")
        return field._like(self.features_at_coordinates(field.float_coordinates))

    def decomposed(self):
        """per batch element: (coordinates [n,3] int32, features [n,C]) — key order keeps the scenes contiguous"""
        counts = self.coordinate_manager.scene_counts(self.keys)
        coords, out, s = self.C, [], 0
        for n in counts:
            out.append((coords[s:s + n, 1:], self.F[s:s + n]))
            s += n
        return out


class TensorField:
    """ME.TensorField(features [N, C], coordinates [N, 4] = (batch, x, y, z)): features on POINTS, several of which may share a
    voxel.  ``sparse()`` quantises them into a SparseTensor (``quantization_mode``; ME's default for a field is the average) and
    keeps the inverse map, so that ``SparseTensor.slice(field)`` / ``cat_slice(field)`` bring site features back to the points.
    ``C`` holds float coordinates floored to int32; ``float_coordinates`` keeps them as given ([N, 4] fp32; integer coordinates
    converted), and ``SparseTensor.interpolate(field)`` reads a tensor of any stride there trilinearly (``MinkowskiInterpolation``).
    The SPLAT_LINEAR_INTERPOLATION and NO_QUANTIZATION modes and a gradient to the coordinates are not built."""

    def __init__(self, features, coordinates, quantization_mode=SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE):
        self.quantization_mode = _quantization_mode(quantization_mode)
        S.L.require_gpu(features, "features")
        S.L.require_gpu(coordinates, "coordinates")
        if coordinates.dim() != 2 or coordinates.shape[1] != 4 or coordinates.shape[0] != features.shape[0]:
            raise ValueError(f"TensorField: coordinates must be [{features.shape[0]}, 4] (batch, x, y, z), got {tuple(coordinates.shape)}")
        self._given = coordinates
        if coordinates.is_floating_point():
            coordinates = torch.floor(coordinates).to(torch.int32)
        self.F, self.C = features, coordinates
        self.coordinate_manager = self._vmap = self._float = None

    @property
    def float_coordinates(self):
        """the coordinates as given, [N, 4] contiguous fp32 (integer coordinates interpolate at themselves); made on first use"""
        if self._float is None:
            self._float = self._given.detach().to(torch.float32).contiguous()
        return self._float

    def _like(self, features):
        """a field of other features on this field's points: same coordinates (``C`` is shared), manager and voxel map"""
        out = TensorField(features, self.C, quantization_mode=self.quantization_mode)
        out._given, out._float = self._given, self._float
        out.coordinate_manager, out._vmap = self.coordinate_manager, self._vmap
        return out

    @property
    def inverse_mapping(self):
        if self._vmap is None:
            raise RuntimeError("TensorField.inverse_mapping: call sparse() first")
        return self._vmap.inverse

    def sparse(self, quantization_mode=None):
        """the SparseTensor of this field's voxels (rows in key order); the field remembers the map for ``slice``"""
        mode = self.quantization_mode if quantization_mode is None else _quantization_mode(quantization_mode)
        x = SparseTensor(self.F, coordinates=self.C, quantization_mode=mode)
        self.coordinate_manager, self._vmap = x.coordinate_manager, x.coordinate_manager.voxel_map
        return x


def sparse_quantize(coordinates, features=None, labels=None, ignore_label=-100, return_index=False, return_inverse=False,
                    return_maps_only=False, quantization_size=None):
    """ME.utils.sparse_quantize on the device: coordinates [N, 3] (or [N, 4] with a leading batch column) -> one row per voxel,
    floor(coordinates / quantization_size) (a float or one per axis).  Returns, in MinkowskiEngine's order: the voxel coordinates
    int32 [M, 3 or 4]; ``features[index]`` if features are given; the voxel labels if labels are given (the label all points of
    the voxel share, ``ignore_label`` where they differ); ``index`` [M] int64 (the lowest input row of each voxel) with
    ``return_index``; ``inverse`` [N] int64 (the voxel row of every input row) with ``return_inverse``.  ``return_maps_only``:
    only index (and inverse).  The rows are in ascending (batch, x, y, z) order — MinkowskiEngine's order is its hash map's and
    unspecified.  Device tensors in, device tensors out; one host read of eight bytes."""
    S.L.require_gpu(coordinates, "coordinates")
    if coordinates.dim() != 2 or coordinates.shape[1] not in (3, 4):
        raise ValueError(f"sparse_quantize: coordinates must be [N, 3] or [N, 4] (batch first), got {tuple(coordinates.shape)}")
    n, batched = coordinates.shape[0], coordinates.shape[1] == 4
    for name, t in (("features", features), ("labels", labels)):
        if t is not None:
            S.L.require_gpu(t, name)
            if t.shape[0] != n:
                raise ValueError(f"sparse_quantize: {name} has {t.shape[0]} rows, coordinates {n}")
    scalar = isinstance(quantization_size, (int, float, np.integer, np.floating))
    if quantization_size is not None and not scalar:
        quantization_size = [float(q) for q in quantization_size]
        if len(quantization_size) != 3:
            raise ValueError("sparse_quantize: quantization_size must be a number or one per axis (3)")
    if scalar and not batched and coordinates.dtype == torch.float32:
        points = coordinates if coordinates.stride(1) == 1 else coordinates.contiguous()
        vmap = S.voxel_map(points, [0, n], float(quantization_size))  # the keys launch floors p / size itself
    else:
        c = coordinates
        if quantization_size is not None:
            q = quantization_size if scalar else torch.tensor(quantization_size, dtype=torch.float32, device=c.device)
            xyz = torch.floor(c[:, -3:].to(torch.float32) / q).to(torch.int32)
            c = torch.cat((c[:, :1].to(torch.int32), xyz), 1) if batched else xyz
        elif c.is_floating_point():
            c = torch.floor(c).to(torch.int32)
        if not batched:
            c = torch.cat((torch.zeros((n, 1), dtype=c.dtype, device=c.device), c), 1)
        vmap = S.voxel_map_coords(c)
    index, inverse = vmap.first, vmap.inverse.to(torch.int64)
    if return_maps_only:
        return (index, inverse) if return_inverse else index
    sites = S.unpack_keys(vmap.sites)
    out = [sites if batched else sites[:, 1:]]
    if features is not None:
        out.append(features[index])
    if labels is not None:
        out.append(S.voxel_labels(labels, vmap, ignore_label))
    if return_index:
        out.append(index)
    if return_inverse:
        out.append(inverse)
    return out[0] if len(out) == 1 else tuple(out)


def _refuse_origin(module, x):
    """a tensor on the origin map (``tensor_stride == 0``: one row per scene, the result of a global pooling) has no lattice for a
    kernel to walk"""
    if x.tensor_stride == 0:
        raise ValueError(f"{type(module).__name__}: the input is an origin tensor (tensor_stride 0, one row per scene, "
                         f"{x.keys.shape[0]} rows): convolutions and local poolings need a tensor on sites; use MinkowskiLinear")


def _expanding(module, expand_coordinates, stride):
    """the ``expand_coordinates`` keyword of a layer's constructor -> bool.  The expansion of a strided, non-transposed layer is
    not built: its candidates v - offset * ts mostly lie off the output lattice and need a filter."""
    if expand_coordinates and not module.transposed and stride > 1:
        raise NotImplementedError(f"{type(module).__name__}: expand_coordinates=True with stride {stride} is not built (the "
                                  "expansion of a non-transposed layer exists at stride 1 only; the transposed layers expand at "
                                  "any stride)")
    return bool(expand_coordinates)


def _given_sites(module, x, out_ts, coordinates):
    """``forward(x, coordinates)``: the output sites the caller chose -> (keys, inverse).  A SparseTensor of the same coordinate
    manager at the layer's output stride: its keys as they are.  A 1-D int64 tensor on the device: sorted unique keys, unchecked.
    An integer [M, 4] tensor on the device: (batch, x, y, z) through ``cm.targets`` — rows in key order, duplicates merged,
    ``inverse`` [M] int32 the row of every given coordinate (it becomes ``out.inverse_mapping``); the coordinates are taken as given,
    nothing ties them to the output lattice.  Everything else is a ValueError that names what was given."""
    name, cm = type(module).__name__, x.coordinate_manager
    if module.expand_coordinates:
        raise ValueError(f"{name}: coordinates together with expand_coordinates=True (the layer chooses its sites or the caller does)")
    if isinstance(coordinates, SparseTensor):
        if coordinates.coordinate_manager is not cm:
            raise ValueError(f"{name}: coordinates is a SparseTensor of a different coordinate manager ({coordinates.coordinate_manager!r}, "
                             f"the input's is {cm!r})")
        if coordinates.tensor_stride != out_ts:
            raise ValueError(f"{name}: coordinates has tensor stride {coordinates.tensor_stride}, the layer's output stride is {out_ts}")
        return coordinates.keys, None
    if not torch.is_tensor(coordinates):
        raise ValueError(f"{name}: coordinates must be a SparseTensor, a key tensor or an integer [M, 4] tensor, not "
                         f"{type(coordinates).__name__}")
    given = f"{tuple(coordinates.shape)} {coordinates.dtype} on {coordinates.device}"
    if not coordinates.is_cuda or coordinates.device != x.keys.device:
        raise ValueError(f"{name}: coordinates must be on the input's device {x.keys.device} (it is {given})")
    if coordinates.dtype == torch.int64 and coordinates.dim() == 1:
        return coordinates, None
    integer = coordinates.dtype in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8)
    if not integer or coordinates.dim() != 2 or coordinates.shape[1] != 4:
        raise ValueError(f"{name}: coordinates must be integer [M, 4] (batch, x, y, z) or int64 keys [M] (it is {given})")
    return cm.targets(coordinates)


def _site_tensor(features, out_ts, cm, keys, inverse):
    """the output of a layer; ``inverse`` (coordinates given as a list): the row of every given coordinate, ``out.F[out.inverse_mapping
    .long()]`` is in the caller's order"""
    out = features if isinstance(features, SparseTensor) else SparseTensor(features, tensor_stride=out_ts, coordinate_manager=cm, keys=keys)
    out.inverse_mapping = inverse
    return out


class MinkowskiConvolution(nn.Module):
    """ME.MinkowskiConvolution(in, out, kernel_size, stride=1, dilation=1, bias=False, kernel_generator=None,
    expand_coordinates=False, dimension=3).
    ``kernel_size`` / ``dilation``: an int or one value per axis; ``kernel_generator`` (KernelGenerator) replaces both and picks
    the region (cube, cross, custom).  ``kernel`` is [volume, in, out] in the generator's offset order.
    Output sites: the input's at stride 1, ``cm.strided`` above it; the transposed form lands on the canonical sites of its output
    stride.  ``expand_coordinates=True`` writes every site the kernel reaches from an input site instead — exactly the sites whose
    row of the kernel map is not empty: u = v - offset * ts at stride 1 (the minus matters for even cubes and custom regions),
    u = v + offset * out_ts transposed (the sites and, with the same kernel, the bits of MinkowskiGenerativeConvolutionTranspose).
    Not built: the expansion of a non-transposed layer above stride 1 (NotImplementedError at construction).
    ``forward(x, coordinates)`` writes the sites the caller gives (``_given_sites``: a SparseTensor, keys, or integer [M, 4]
    coordinates); a target that no input reaches is a zero row (plus bias)."""
    transposed, generative = False, False

    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False, kernel_generator=None,
                 expand_coordinates=False, dimension=3):
        super().__init__()
        assert dimension == 3
        if kernel_generator is None:
            kernel_generator = KernelGenerator(kernel_size, stride, dilation, is_transpose=self.transposed,
                                               expand_coordinates=bool(expand_coordinates), dimension=dimension)
        else:
            ks, dl = kernel_generator.kernel_size, kernel_generator.kernel_dilation
            kernel_size = ks[0] if len(set(ks)) == 1 else ks  # (a cubic size stays an int)
            dilation = dl[0] if len(set(dl)) == 1 else dl
        if isinstance(stride, (tuple, list)):
            if any(s != stride[0] for s in stride):
                raise NotImplementedError(f"stride {stride}: one stride for all three axes only")
            stride = int(stride[0])
        if stride > 1 and max(kernel_generator.kernel_dilation) > 1:
            raise ValueError(f"stride {stride} together with dilation {kernel_generator.kernel_dilation}")
        self.in_channels, self.out_channels, self.kernel_size, self.stride = in_channels, out_channels, kernel_size, stride
        self.dilation, self.kernel_generator = dilation, kernel_generator
        self.expand_coordinates = _expanding(self, expand_coordinates, stride)
        self._offsets = _Offsets(kernel_generator.scaled_offsets())
        kv = kernel_generator.kernel_volume
        # MinkowskiEngine keeps a plain [in, out] matrix only for the 1x1x1 stride-1 case
        shape = (in_channels, out_channels) if (kv == 1 and stride == 1) else (kv, in_channels, out_channels)
        self.kernel = nn.Parameter(torch.empty(shape))
        self.bias = nn.Parameter(torch.zeros(1, out_channels)) if bias else None
        stdv = 1.0 / math.sqrt((out_channels if self.transposed else in_channels) * kv)
        with torch.no_grad():
            self.kernel.uniform_(-stdv, stdv)

    def _out_stride(self, ts):
        if not self.transposed:
            return ts * self.stride
        assert ts % self.stride == 0, "transposed convolution below tensor stride 1"
        return ts // self.stride

    def forward(self, x, coordinates=None):
        cm, ts = x.coordinate_manager, x.tensor_stride
        _refuse_origin(self, x)
        out_ts = self._out_stride(ts)
        w = self.kernel if self.kernel.dim() == 3 else self.kernel[None]
        inverse = None
        if coordinates is not None:
            out_keys, inverse = _given_sites(self, x, out_ts, coordinates)
        elif self.generative:
            out_keys = cm.generated(x.keys, out_ts, self._offsets)
        elif self.expand_coordinates:
            out_keys = cm.expanded(x.keys, ts, out_ts, self._offsets, self.transposed)
        elif self.transposed:
            assert out_ts in cm.keys, "MinkowskiConvolutionTranspose needs existing sites at the output stride"
            out_keys = cm.keys[out_ts]
        else:
            out_keys = x.keys if out_ts == ts else cm.strided(x.keys, ts, out_ts)
        nbr, inv, plan = cm.kernel_map(x.keys, out_keys, ts, out_ts, self._offsets, self.transposed)
        if _geometry_only():
            if hasattr(plan, "request_wgrad"):  # the weight-gradient chunk table of this layer's width: built with the geometry
                plan.request_wgrad(w.shape[1], w.shape[2])
            return _site_tensor(x.F.new_empty((out_keys.shape[0], self.out_channels)), out_ts, cm, out_keys, inverse)
        if _conv_bn_fusable(self, x.F, plan=plan, cout=self.out_channels):
            return _site_tensor(SparseTensor.pending(_PendingConv(S.pair_products(x.F, w, plan), plan.slot, self.out_channels, self.bias),
                                                     out_ts, cm, out_keys), out_ts, cm, out_keys, inverse)
        f = S.sparse_conv(x.F, w, nbr, inv, plan)
        if self.bias is not None:
            f = f + self.bias
        return _site_tensor(f, out_ts, cm, out_keys, inverse)


class MinkowskiConvolutionTranspose(MinkowskiConvolution):
    """ME.MinkowskiConvolutionTranspose: onto the canonical sites of the output stride; with ``expand_coordinates=True`` onto the
    children u = v + offset * out_ts of every input site (any stride the class accepts), the key set and bits of
    MinkowskiGenerativeConvolutionTranspose; ``forward(x, coordinates)`` onto given sites, e.g. a pruned tensor's."""
    transposed = True


class MinkowskiGenerativeConvolutionTranspose(MinkowskiConvolution):
    """ME.MinkowskiGenerativeConvolutionTranspose: every child site, through ``CoordinateManager.generated`` (an ATen composition;
    profiles/expand_bench.txt holds both sides for the day it moves onto ``expanded``)."""
    transposed, generative = True, True


class MinkowskiChannelwiseConvolution(nn.Module):
    """ME.MinkowskiChannelwiseConvolution(in_channels, kernel_size=-1, stride=1, dilation=1, bias=False, kernel_generator=None,
    dimension=3): the depthwise convolution.  ``kernel`` is [volume, in_channels] in the generator's offset order (one weight per
    offset and channel, no mixing across channels), ``bias`` [1, in_channels]; y[u] = sum over the neighbours that exist of
    kernel[k] * x[nbr[k][u]] (+ bias).  Output sites and map are those of a MinkowskiConvolution / pooling of the same generator and
    stride: the coordinate manager's cached map, shared with them.  One HIP launch forward, one for the input gradient, two for the
    kernel / bias gradients (``sparse_ops.channelwise_conv``).
    Not built: a transposed channelwise convolution (MinkowskiEngine has none), dimension 4, double backward, and a fused
    convolution -> BatchNorm -> activation inference form (a following MinkowskiBatchNorm runs its own launch).
    ``expand_coordinates=True`` (stride 1 only: NotImplementedError above it) and ``forward(x, coordinates)`` choose the output sites
    as in MinkowskiConvolution."""
    transposed = False

    def __init__(self, in_channels, kernel_size=-1, stride=1, dilation=1, bias=False, kernel_generator=None,
                 expand_coordinates=False, dimension=3):
        super().__init__()
        assert dimension == 3
        if kernel_generator is None:
            kernel_generator = KernelGenerator(kernel_size, stride, dilation, is_transpose=False,
                                               expand_coordinates=bool(expand_coordinates), dimension=dimension)
        else:
            ks, dl = kernel_generator.kernel_size, kernel_generator.kernel_dilation
            kernel_size = ks[0] if len(set(ks)) == 1 else ks  # (a cubic size stays an int)
            dilation = dl[0] if len(set(dl)) == 1 else dl
        if isinstance(stride, (tuple, list)):
            if any(s != stride[0] for s in stride):
                raise NotImplementedError(f"stride {stride}: one stride for all three axes only")
            stride = int(stride[0])
        if stride > 1 and max(kernel_generator.kernel_dilation) > 1:
            raise ValueError(f"stride {stride} together with dilation {kernel_generator.kernel_dilation}")
        self.in_channels, self.out_channels, self.kernel_size, self.stride = in_channels, in_channels, kernel_size, stride
        self.dilation, self.kernel_generator = dilation, kernel_generator
        self.expand_coordinates = _expanding(self, expand_coordinates, stride)
        self._offsets = _Offsets(kernel_generator.scaled_offsets())
        kv = kernel_generator.kernel_volume
        self.kernel = nn.Parameter(torch.empty(kv, in_channels))
        self.bias = nn.Parameter(torch.zeros(1, in_channels)) if bias else None
        stdv = 1.0 / math.sqrt(in_channels * kv)
        with torch.no_grad():
            self.kernel.uniform_(-stdv, stdv)

    def forward(self, x, coordinates=None):
        cm, ts = x.coordinate_manager, x.tensor_stride
        _refuse_origin(self, x)
        out_ts = ts * self.stride
        inverse = None
        if coordinates is not None:
            out_keys, inverse = _given_sites(self, x, out_ts, coordinates)
        elif self.expand_coordinates:
            out_keys = cm.expanded(x.keys, ts, out_ts, self._offsets, False)
        else:
            out_keys = x.keys if out_ts == ts else cm.strided(x.keys, ts, out_ts)
        nbr, inv = cm.pool_map(x.keys, out_keys, ts, out_ts, self._offsets, False)
        if _geometry_only():
            return _site_tensor(x.F.new_empty((out_keys.shape[0], self.in_channels)), out_ts, cm, out_keys, inverse)
        f = S.channelwise_conv(x.F.contiguous(), self.kernel, nbr, inv, self.bias)
        return _site_tensor(f, out_ts, cm, out_keys, inverse)


class MinkowskiBatchNorm(nn.Module):
    """BatchNorm1d over the feature rows of all sites of the batch (ME.MinkowskiBatchNorm: parameters under ``.bn``)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        self.bn = nn.BatchNorm1d(num_features, eps=eps, momentum=momentum, affine=affine,
                                 track_running_stats=track_running_stats)

    fused_act = None  # "elu" / "relu": the activation module that follows in an nn.Sequential is folded into this layer

    def forward(self, x, act=None, residual=None, post_add=None):
        """act(bn(x) + residual) (+ post_add: a skip tensor added behind the activation, ``post_add + out``)"""
        if _geometry_only():
            return x
        act = act or self.fused_act
        conv = x._pending
        if conv is not None and _conv_bn_fusable(self, None, bn=self.bn):
            if post_add is not None:
                assert x.keys is post_add.keys or torch.equal(x.keys, post_add.keys), "sparse tensors on different coordinate maps"
            out = x._like(S.gather_sum_bn_act(conv.y, conv.slot, self.bn, act, None if residual is None else residual.F,
                                              None if post_add is None else post_add.F, conv.bias, conv.channels))
            _record_path("fused")
        else:
            out = x._like(S.bn_act(x.F, self.bn, act, None if residual is None else residual.F))
            if post_add is not None:
                out = post_add + out
            _record_path("composition")
        out.applied_act = act
        return out


class MinkowskiInstanceNorm(nn.Module):
    """per batch element, per channel normalisation over the element's sites, with affine parameters"""

    def __init__(self, num_features, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(1, num_features))
        self.bias = nn.Parameter(torch.zeros(1, num_features))
        self.eps = eps

    def forward(self, x):
        if _geometry_only():
            return x
        seg, nseg = x.coordinate_manager.scene_segments(x.keys)  # geometry: cached per key set, on the device
        return x._like(S.instance_norm(x.F.contiguous(), seg, nseg, self.weight, self.bias, self.eps))


class _MinkowskiPooling(nn.Module):
    """Pooling over a kernel region: the output sites are those of a convolution of the same kernel and stride (the same sites
    at stride 1, ``cm.strided`` above it), the map is the coordinate manager's, shared with such a convolution.
    ``expand_coordinates=True``: every site the kernel reaches from an input site (non-transposed at stride 1 only, NotImplementedError
    above it; the transposed poolings at any stride); ``forward(x, coordinates)``: the sites the caller gives, a target without a
    neighbour holding what ``sparse_pool`` writes for an empty row (0 for sum and avg).  Both as in MinkowskiConvolution; DESIGN 6.19."""
    mode, transposed = None, False

    def __init__(self, kernel_size, stride=1, dilation=1, kernel_generator=None, expand_coordinates=False, dimension=3):
        super().__init__()
        assert dimension == 3
        if kernel_generator is None:
            kernel_generator = KernelGenerator(kernel_size, stride, dilation, is_transpose=self.transposed,
                                               expand_coordinates=bool(expand_coordinates), dimension=dimension)
        if isinstance(stride, (tuple, list)):
            if any(s != stride[0] for s in stride):
                raise NotImplementedError(f"stride {stride}: one stride for all three axes only")
            stride = int(stride[0])
        if stride > 1 and max(kernel_generator.kernel_dilation) > 1:
            raise ValueError(f"stride {stride} together with dilation {kernel_generator.kernel_dilation}")
        self.kernel_size, self.stride, self.dilation, self.kernel_generator = kernel_size, stride, dilation, kernel_generator
        self.expand_coordinates = _expanding(self, expand_coordinates, stride)
        self._offsets = _Offsets(kernel_generator.scaled_offsets())

    def _sites(self, x, coordinates=None):
        """(output stride, output keys, the inverse map of coordinates given as a list or None)"""
        cm, ts = x.coordinate_manager, x.tensor_stride
        if not self.transposed:
            out_ts = ts * self.stride
        else:
            assert ts % self.stride == 0, "transposed pooling below tensor stride 1"
            out_ts = ts // self.stride
        if coordinates is not None:
            return (out_ts,) + tuple(_given_sites(self, x, out_ts, coordinates))
        if self.expand_coordinates:
            return out_ts, cm.expanded(x.keys, ts, out_ts, self._offsets, self.transposed), None
        if not self.transposed:
            return out_ts, (x.keys if out_ts == ts else cm.strided(x.keys, ts, out_ts)), None
        assert out_ts in cm.keys, f"{type(self).__name__} needs existing sites at the output stride"
        return out_ts, cm.keys[out_ts], None

    def forward(self, x, coordinates=None):
        cm, ts = x.coordinate_manager, x.tensor_stride
        _refuse_origin(self, x)
        out_ts, out_keys, inverse = self._sites(x, coordinates)
        if _geometry_only():
            cm.kernel_map(x.keys, out_keys, ts, out_ts, self._offsets, self.transposed)
            return _site_tensor(x.F.new_empty((out_keys.shape[0], x.F.shape[1])), out_ts, cm, out_keys, inverse)
        nbr, inv = cm.pool_map(x.keys, out_keys, ts, out_ts, self._offsets, self.transposed)
        return _site_tensor(S.sparse_pool(x.F.contiguous(), nbr, inv, self.mode), out_ts, cm, out_keys, inverse)


class MinkowskiSumPooling(_MinkowskiPooling):
    """ME.MinkowskiSumPooling: the sum over the neighbours that exist"""
    mode = "sum"


class MinkowskiAvgPooling(_MinkowskiPooling):
    """ME.MinkowskiAvgPooling: that sum divided by the number of neighbours that exist (not by the kernel volume)"""
    mode = "avg"


class MinkowskiMaxPooling(_MinkowskiPooling):
    """ME.MinkowskiMaxPooling: per channel the maximum over the neighbours that exist (ties: the lowest kernel index)"""
    mode = "max"


class MinkowskiPoolingTranspose(_MinkowskiPooling):
    """ME.MinkowskiPoolingTranspose: the sum over the transposed map onto the existing sites of the output stride, exactly where
    MinkowskiConvolutionTranspose lands"""
    mode, transposed = "sum", True


class MinkowskiAvgUnpooling(_MinkowskiPooling):
    """MinkowskiPoolingTranspose with every output row divided by the number of input rows that reach it.  (The reference's
    ``avg_unpool`` names a class MinkowskiEngine's master no longer has: this definition is this package's own)"""
    mode, transposed = "avg", True


class MinkowskiUnion(nn.Module):
    """ME.MinkowskiUnion: the sum of two or more sparse tensors of one coordinate manager and tensor stride on the union of their
    sites — the left fold of ``+``."""

    def forward(self, *inputs):
        if len(inputs) < 2:
            raise ValueError(f"MinkowskiUnion: {len(inputs)} input (two or more sparse tensors)")
        out = inputs[0]
        for x in inputs[1:]:
            out = out + x
        return out


class MinkowskiPruning(nn.Module):
    """ME.MinkowskiPruning: keep the rows of ``x`` whose ``mask`` entry is true, in order, at the same tensor stride and with the
    same coordinate manager, on a new non-canonical key set (like the generated ones).  ``mask``: bool [N] on x's device, in
    ``x.F``'s row order.  Backward: a kept row receives its gradient, a dropped one an exact zero.  The mask is DATA: under
    ``geometry_only`` the module passes x through, and the maps of the layers behind a pruning are built in the real forward."""

    def forward(self, x, mask):
        if _geometry_only():
            return x
        n = x.keys.shape[0]
        if not torch.is_tensor(mask) or mask.dtype != torch.bool:
            raise ValueError(f"MinkowskiPruning: the mask must be a bool tensor, not {getattr(mask, 'dtype', type(mask))}")
        if mask.dim() != 1 or mask.shape[0] != n:
            raise ValueError(f"MinkowskiPruning: a mask of shape {tuple(mask.shape)} for {n} rows")
        if mask.device != x.keys.device:
            raise ValueError(f"MinkowskiPruning: the mask is on {mask.device}, the tensor on {x.keys.device}")
        kept, pos, keys = S.prune_map(mask.contiguous(), x.keys)
        return SparseTensor(S.take_rows(x.F.contiguous(), kept, back=pos), tensor_stride=x.tensor_stride,
                            coordinate_manager=x.coordinate_manager, keys=keys)


class MinkowskiInterpolation(nn.Module):
    """ME.MinkowskiInterpolation: ``forward(input, tfield)`` -> [N, C], the features of the SparseTensor ``input`` (any integer
    tensor stride) interpolated trilinearly at ``tfield`` [N, 4] fp32 (batch, x, y, z) in units of the finest voxel.  A site's
    feature sits at its integer coordinate; the 2^3 sites around a point weigh in by the usual products, the ones that do not
    exist count as zero and the rest is NOT renormalised (this package's own statement).  With ``return_kernel_map``
    / ``return_weights`` the result is the list [out, (in_map, out_map)?, weights?] of the pairs that exist in ascending (point,
    corner) order: in_map = site rows, out_map = field rows (int32), weights fp32 — compacted with one host read; the plain
    call reads nothing back.  Gradients reach the features only.  Under ``geometry_only`` the map is built and cached, the
    table is uninitialised."""

    def __init__(self, return_kernel_map=False, return_weights=False):
        super().__init__()
        self.return_kernel_map, self.return_weights = bool(return_kernel_map), bool(return_weights)

    def forward(self, input, tfield):
        if not isinstance(input, SparseTensor):
            raise ValueError(f"MinkowskiInterpolation: a SparseTensor is expected, not {type(input).__name__}")
        if not torch.is_tensor(tfield) or tfield.dim() != 2 or tfield.shape[1] != 4 or tfield.dtype != torch.float32:
            raise ValueError("MinkowskiInterpolation: tfield must be a [N, 4] float32 tensor (batch, x, y, z), got "
                             f"{tuple(tfield.shape) if torch.is_tensor(tfield) else type(tfield).__name__}"
                             f"{' ' + str(tfield.dtype) if torch.is_tensor(tfield) else ''}")
        if tfield.device != input.keys.device:
            raise ValueError(f"MinkowskiInterpolation: tfield is on {tfield.device}, the tensor on {input.keys.device}")
        imap = input._interp_map(tfield.detach().contiguous())
        if _geometry_only():
            out = input.F.new_empty((tfield.shape[0], input.F.shape[1]))
        else:
            out = S.interpolate(input.F.contiguous(), imap)
        if not (self.return_kernel_map or self.return_weights):
            return out
        at = torch.nonzero(imap.nbr.view(-1) >= 0).view(-1)  # ascending n * 8 + k (the one host read: the pair count is data)
        result = [out]
        if self.return_kernel_map:
            result.append((imap.nbr.view(-1)[at], (at >> 3).to(torch.int32)))
        if self.return_weights:
            result.append(imap.w.view(-1)[at])
        return result


class _Pointwise(nn.Module):
    kind = None

    def forward(self, x):
        if _geometry_only():
            return x
        if getattr(x, "applied_act", None) == self.kind:  # already applied by the fused BatchNorm in front (fuse_activations)
            return x._like(x.F)
        return x._like(self.fn(x.F))


class MinkowskiReLU(_Pointwise):
    kind = "relu"

    def __init__(self, inplace=False):
        super().__init__()
        self.fn = nn.ReLU()


class MinkowskiELU(_Pointwise):
    kind = "elu"

    def __init__(self, alpha=1.0, inplace=False):
        super().__init__()
        self.fn = nn.ELU(alpha)


class MinkowskiSigmoid(_Pointwise):
    kind = "sigmoid"

    def __init__(self):
        super().__init__()
        self.fn = nn.Sigmoid()


class MinkowskiLinear(nn.Module):
    """ME.MinkowskiLinear(in_features, out_features, bias=True): a linear map of the feature rows of any SparseTensor, the
    origin one included; parameters under ``.linear`` (state-dict keys ``linear.weight`` / ``linear.bias``)."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.linear = nn.Linear(in_features, out_features, bias=bias)

    def forward(self, x):
        if _geometry_only():
            return x._like(x.F.new_empty((x.F.shape[0], self.linear.out_features)))
        return x._like(self.linear(x.F))


class MinkowskiGlobalPooling(nn.Module):
    """ME.MinkowskiGlobalPooling (the average, ME's default) and its sum / max forms: a SparseTensor of the same coordinate
    manager on the ORIGIN map — one row per scene 0 .. ``cm.num_scenes - 1`` in order, keys (b, 0, 0, 0), ``tensor_stride`` 0 as
    the marker.  A scene absent from the input's key set (a MinkowskiPruning took it) keeps its row: zeros, no gradient.  avg is
    the float32 sum times 1 / n; max follows np.max / np.argmax.  These definitions are this package's own.  Two
    launches forward, one backward, no host read.  Under ``geometry_only`` the segment table is built and cached and the output
    table is uninitialised."""
    mode = "avg"

    def forward(self, x):
        if not isinstance(x, SparseTensor):
            raise ValueError(f"{type(self).__name__}: a SparseTensor is expected, not {type(x).__name__}")
        if x.tensor_stride == 0:
            raise ValueError(f"{type(self).__name__}: the input is already an origin tensor (tensor_stride 0)")
        cm = x.coordinate_manager
        seg, nseg = cm.scene_segments(x.keys)  # geometry: cached per key set, on the device
        if _geometry_only():
            f = x.F.new_empty((nseg, x.F.shape[1]))
        else:
            f = S.global_pool(x.F.contiguous(), seg, nseg, self.mode)
        return SparseTensor(f, tensor_stride=0, coordinate_manager=cm, keys=cm.origin_keys())


class MinkowskiGlobalSumPooling(MinkowskiGlobalPooling):
    mode = "sum"


class MinkowskiGlobalAvgPooling(MinkowskiGlobalPooling):
    mode = "avg"


class MinkowskiGlobalMaxPooling(MinkowskiGlobalPooling):
    mode = "max"


class MinkowskiBroadcast(nn.Module):
    """ME.MinkowskiBroadcast*: ``forward(x, x_glob)`` combines every row of ``x`` with its scene's row of the origin tensor
    ``x_glob`` (a global pooling's result, possibly through MinkowskiLinear / pointwise layers).  The result lives on x's keys and
    stride.  One launch forward; the backward's sweep for dx leaves the partials of the origin tensor's gradient, a fold per scene
    adds them.  Under ``geometry_only`` x passes through (concatenation: an uninitialised table of the right width)."""
    mode = None

    def forward(self, x, x_glob):
        name = type(self).__name__
        if self.mode is None:
            raise NotImplementedError("MinkowskiBroadcast is the base: use MinkowskiBroadcastAddition / Multiplication / Concatenation")
        if not isinstance(x, SparseTensor) or not isinstance(x_glob, SparseTensor):
            raise ValueError(f"{name}: two SparseTensors are expected, not {type(x).__name__} and {type(x_glob).__name__}")
        cm = x.coordinate_manager
        if x_glob.coordinate_manager is not cm or x_glob.tensor_stride != 0:
            raise ValueError(f"{name}: x_glob must be an origin tensor (tensor_stride 0) of x's coordinate manager; it has "
                             f"tensor_stride {x_glob.tensor_stride} and manager {x_glob.coordinate_manager!r}, x has {cm!r}")
        seg, nseg = cm.scene_segments(x.keys)
        cx, (rows, cg) = x.F.shape[1], x_glob.F.shape
        if rows != nseg:
            raise ValueError(f"{name}: x_glob has {rows} rows, the coordinate manager {nseg} scenes")
        if self.mode != "cat" and cg != cx:
            raise ValueError(f"{name}: x has {cx} channels and x_glob {cg}")
        if _geometry_only():
            return x if self.mode != "cat" else x._like(x.F.new_empty((x.F.shape[0], cx + cg)))
        return x._like(S.broadcast(x.F.contiguous(), x_glob.F.contiguous(), seg, nseg, self.mode))


class MinkowskiBroadcastAddition(MinkowskiBroadcast):
    mode = "add"


class MinkowskiBroadcastMultiplication(MinkowskiBroadcast):
    mode = "mul"


class MinkowskiBroadcastConcatenation(MinkowskiBroadcast):
    mode = "cat"


class BasicBlock(nn.Module):
    """MinkowskiEngine.modules.resnet_block.BasicBlock (used by models/mink_resnet.py:5,22-23)."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, bn_momentum=0.1, dimension=-1):
        super().__init__()
        assert dimension > 0
        self.conv1 = MinkowskiConvolution(inplanes, planes, kernel_size=3, stride=stride, dilation=dilation, dimension=dimension)
        self.norm1 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.conv2 = MinkowskiConvolution(planes, planes, kernel_size=3, stride=1, dilation=dilation, dimension=dimension)
        self.norm2 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.relu = MinkowskiReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        residual = x if self.downsample is None else self.downsample(x)
        out = self.norm1(self.conv1(x), act="relu")
        return self.norm2(self.conv2(out), act="relu", residual=residual)  # relu(bn(conv) + residual) in one pass


class Bottleneck(nn.Module):
    """MinkowskiEngine.modules.resnet_block.Bottleneck (depth 50 / 101 / 152)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, bn_momentum=0.1, dimension=-1):
        super().__init__()
        assert dimension > 0
        self.conv1 = MinkowskiConvolution(inplanes, planes, kernel_size=1, dimension=dimension)
        self.norm1 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.conv2 = MinkowskiConvolution(planes, planes, kernel_size=3, stride=stride, dilation=dilation, dimension=dimension)
        self.norm2 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.conv3 = MinkowskiConvolution(planes, planes * self.expansion, kernel_size=1, dimension=dimension)
        self.norm3 = MinkowskiBatchNorm(planes * self.expansion, momentum=bn_momentum)
        self.relu = MinkowskiReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        residual = x if self.downsample is None else self.downsample(x)
        out = self.norm1(self.conv1(x), act="relu")
        out = self.norm2(self.conv2(out), act="relu")
        return self.norm3(self.conv3(out), act="relu", residual=residual)


def fuse_activations(module):
    """In every nn.Sequential, fold a MinkowskiReLU / MinkowskiELU (alpha 1) that directly follows a MinkowskiBatchNorm into
    that layer's fused kernel (the activation module stays in place — state-dict indices are unchanged — and passes
    tensors that already carry its activation through)."""
    for m in module.modules():
        if isinstance(m, nn.Sequential):
            mods = list(m)
            for a, b in zip(mods, mods[1:]):
                if isinstance(a, MinkowskiBatchNorm) and isinstance(b, _Pointwise) and (b.kind == "relu" or (b.kind == "elu" and b.fn.alpha == 1.0)):
                    a.fused_act = b.kind
    return module


def sequential_add(block, x, skip):
    """``skip + block(x)`` for an nn.Sequential that ends BatchNorm -> folded activation (``fuse_activations``).  Under inference
    the add is the ``post_add`` of the block's last fused launch; everywhere else it is exactly ``skip + block(x)``.  A block
    whose output sites differ from the skip's (a generative up block) still runs its last launch fused, without ``post_add``,
    and the add is the union add of ``skip + ...``."""
    mods = list(block) if isinstance(block, nn.Sequential) else []
    tail = mods[-2] if len(mods) >= 2 else None
    if not (INFER_FUSED and HD.inference(block)) or _geometry_only() or not isinstance(tail, MinkowskiBatchNorm) \
            or not isinstance(mods[-1], _Pointwise) or tail.fused_act != mods[-1].kind:
        return skip + block(x)
    for m in mods[:-2]:
        x = m(x)
    if not x._same_map(skip):
        return skip + mods[-1](tail(x))  # tail records its own launch in LAST_PATHS
    return mods[-1](tail(x, post_add=skip))


def kaiming_normal_(tensor, a=0, mode="fan_in", nonlinearity="leaky_relu"):
    """ME.utils.kaiming_normal_ on a [K, Cin, Cout] kernel: fan_in = K * Cin, fan_out = K * Cout."""
    if tensor.dim() == 3:
        fan = tensor.shape[0] * (tensor.shape[1] if mode == "fan_in" else tensor.shape[2])
    else:
        fan = tensor.shape[0] if mode == "fan_in" else tensor.shape[1]
    std = nn.init.calculate_gain(nonlinearity, a) / math.sqrt(fan)
    with torch.no_grad():
        return tensor.normal_(0, std)


def batch_sparse_collate(data):
    """ME.utils.batch_sparse_collate([(coords_i [n_i,3] float or int, feats_i [n_i,C]), ...]) -> (coordinates [N,4] int32 with
    the batch index in column 0, features [N,C]).  Float coordinates are floored (model_vdetr.py:252-259 passes p / voxel_size)."""
    coords, feats = [], []
    for b, (c, f) in enumerate(data):
        c = torch.floor(c) if c.is_floating_point() else c
        c = c.to(torch.int32)
        coords.append(torch.cat((torch.full((c.shape[0], 1), b, dtype=torch.int32, device=c.device), c), dim=1))
        feats.append(f)
    return torch.cat(coords), torch.cat(feats)
