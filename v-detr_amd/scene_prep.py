"""A loaded scan -> the model's ``inputs`` and the criterion's ``targets`` on the device (reference
datasets/scannet.py:510-626, ``ScannetDetectionDataset.__getitem__`` after the files are read).

The loader hands over raw arrays: the packed clouds of a batch, their boxes and the per-scene augmentation parameters
(``draw_augment_params`` draws them from ``np.random`` exactly as the reference consumes it, so a seed gives the reference's
own augmentation; ``AugmentParams.identity`` is the evaluation split).  ``prepare_scenes`` then flips, rotates, translates and
scales clouds and boxes, takes ``point_cloud_dims_min/max`` and builds the ``gt_*`` tensors in two launches on the current
stream (csrc/scene_prep.hip), with no host round trip.  ``crop_and_sample`` is the step before it in the training split, the
cuboid crop and the sampling (scannet.py:476-498, csrc/cuboid.hip): it replays the random stream attempt by attempt and returns
the ``choices`` that ``prepare_scenes`` takes.  Before the crop come the per-point steps of scannet.py:436-464 (DESIGN.md 6.5,
csrc/color_aug.hip): ``draw_color_augment`` + ``augment_colors`` are the four ``--use_color`` augmentations, ``append_height`` is
``use_height``; after ``prepare_scenes`` comes ``draw_sunrgbd_color`` + ``sunrgbd_color_augment`` (``--coloraug_sunrgbd``,
:544-560).  One generator per scene, used in that order, is left where the reference leaves ``np.random``, so a raw
``_vert.npy`` array goes to the device once.  ``vertex_normals`` + ``with_normals`` are ``--use_normals`` (scannet.py:394-420 and
:457-458, DESIGN.md 6.6, csrc/normals.hip): the area-weighted vertex normals of the scan's mesh become columns 6:9 of a
``use_color`` cloud.  The call order is ``augment_colors`` -> normals -> ``append_height`` -> ``crop_and_sample`` ->
``prepare_scenes`` -> ``sunrgbd_color_augment``; flips and the rotation touch columns 0:3 only, so the normals are not turned,
as in the reference.  Normals depend on the raw mesh alone and draw nothing from the generator, so a caller may compute them
once per scan and keep them (no such cache is built here).  File reading (the ``.ply``, the split lists) and ``use_superpoint``
stay with the loader.  No CPU path.
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L

TARGET_KEYS = ("gt_box_corners", "gt_box_centers", "gt_box_centers_normalized", "gt_angle_class_label", "gt_angle_residual_label",
               "gt_box_sem_cls_label", "gt_box_present", "gt_box_sizes", "gt_box_sizes_normalized", "gt_box_sizes_residual_label",
               "gt_box_angles")


@dataclass
class AugmentParams:
    """Per-scene parameters of scannet.py:516-541: flips (bool [B]), rot_angle [B], trans [B,3], scale [B] (float64)."""
    flip_x: np.ndarray
    flip_y: np.ndarray
    rot_angle: np.ndarray
    trans: np.ndarray
    scale: np.ndarray

    @classmethod
    def identity(cls, B):
        """augment=False: nothing is flipped, turned, moved or scaled"""
        return cls(np.zeros(B, bool), np.zeros(B, bool), np.zeros(B), np.zeros((B, 3)), np.ones(B))

    def __len__(self):
        return len(self.rot_angle)

    def table(self):
        """[B, 8] float64 rows (flip_x, flip_y, cos, sin, trans xyz, scale): what the kernels read"""
        angle = np.asarray(self.rot_angle, np.float64)
        return np.ascontiguousarray(np.concatenate(
            [np.asarray(self.flip_x, np.float64)[:, None], np.asarray(self.flip_y, np.float64)[:, None], np.cos(angle)[:, None],
             np.sin(angle)[:, None], np.asarray(self.trans, np.float64).reshape(-1, 3), np.asarray(self.scale, np.float64)[:, None]], 1))


def draw_augment_params(B, rot_ratio, trans_ratio, scale_ratio, random=np.random):
    """Draws B scenes' parameters from ``random`` (``np.random`` or a ``RandomState``) scene by scene in the order of
    scannet.py:516-540: two flips, the angle, then the translation only if trans_ratio > 0 and the scale only if
    scale_ratio > 0 — a ratio of 0 leaves the stream where the reference leaves it."""
    p = AugmentParams.identity(B)
    for b in range(B):
        p.flip_x[b] = random.random() > 0.5
        p.flip_y[b] = random.random() > 0.5
        p.rot_angle[b] = ((random.random() * np.pi / 18) - np.pi / 36) * rot_ratio / 5.0
        if trans_ratio > 0.0:
            p.trans[b] = (random.random(size=3) - 0.5) * trans_ratio / 0.5
        if scale_ratio > 0.0:
            p.scale[b] = 1 + (random.random() - 0.5) * scale_ratio / 0.5
    return p


def nyu40_to_class(nyu40_ids, dataset_config):
    """The last column of a scan's ``_bbox.npy`` -> class indices, on the host (scannet.py:607-610)."""
    table = dataset_config.nyu40id2class
    return np.array([table[int(x)] for x in np.asarray(nyu40_ids).reshape(-1)], np.int64).reshape(np.shape(nyu40_ids))


def _host_i32(a, name):
    if torch.is_tensor(a):
        a = a.cpu().numpy()   # a device tensor costs one synchronisation here: pass offsets as the loader has them, on the host
    a = np.ascontiguousarray(np.asarray(a), dtype=np.int64)
    if a.ndim != 1 or len(a) < 1:
        raise ValueError(f"{name} must hold B + 1 row offsets")
    return a


def _packed_scenes(points, offsets, min_width, what, *, name="points", strided=False, gpu=True):
    """The one place that holds a packed float32 [N, columns] tensor against its B + 1 host offsets -> (offsets int64, rows per
    scene).  ``name``: "points" or "vertices", the wording of the messages; ``strided``: the rows may be strided (unit column
    stride); ``gpu=False`` leaves ``require_gpu`` to the caller, after its own host checks."""
    if gpu:
        L.require_gpu(points, name)
    L.require_float(points, name)
    off_name = "offsets" if name == "points" else "vert_offsets"
    off = _host_i32(offsets, off_name)
    if points.dim() != 2 or points.shape[1] < min_width or (strided and (points.stride(1) != 1 or points.stride(0) < min_width)):
        layout = " with unit column stride" if strided else ""
        raise ValueError(f"{what}: {name} must be [N, {min_width} or more columns]{layout}, got {tuple(points.shape)}")
    N = points.shape[0]
    if off[0] != 0 or off[-1] != N or N >= 2 ** 31:
        raise ValueError(f"{off_name} run from {off[0]} to {off[-1]}, {name} has {N} rows")
    sizes = np.diff(off)
    if (sizes <= 0).any():
        raise ValueError(f"scene {int(np.argmax(sizes <= 0))} has no {name}")
    return off, sizes


def _box_tables(boxes, box_counts, box_classes, B, dtypes=(torch.float32,)):
    """boxes [B,G,6] of one of ``dtypes``, box_counts [B], box_classes [B,G] on the device -> the three detached and contiguous,
    counts and classes as int64"""
    for t, name in ((boxes, "boxes"), (box_counts, "box_counts"), (box_classes, "box_classes")):
        L.require_gpu(t, name)
    if boxes.dtype not in dtypes:
        raise RuntimeError("boxes must be a float tensor" if len(dtypes) == 1 else "boxes must be a float or double tensor")
    if boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[2] != 6:
        raise ValueError(f"boxes must be [{B}, G, 6], got {tuple(boxes.shape)}")
    if tuple(box_counts.shape) != (B,) or tuple(box_classes.shape) != (B, boxes.shape[1]):
        raise ValueError("box_counts [B] and box_classes [B,G] must describe the B scenes of offsets")
    return boxes.detach().contiguous(), box_counts.detach().to(torch.int64).contiguous(), box_classes.detach().to(torch.int64).contiguous()


def _upload_offsets(off, dev):
    """-> (the offsets as int32 on the host, their device copy, the host array's address for the C ABI); the caller keeps the
    first alive while the address is in use"""
    off32 = np.ascontiguousarray(off, dtype=np.int32)
    return off32, torch.from_numpy(off32).to(dev, non_blocking=True), off32.ctypes.data_as(ctypes.c_void_p)


def prepare_scenes(points, offsets, boxes, box_counts, box_classes, params, dataset_config, *, choices=None, color_mean=None,
                   max_num_obj=None):
    """points [N,3+C] f32 (packed scenes), offsets [B+1] (host array / CPU tensor; a device tensor is read back once), boxes
    [B,G,6] f32 centre + size, box_counts [B], box_classes [B,G] int64 class indices (``nyu40_to_class``), params
    ``AugmentParams`` -> dict of device tensors: ``point_clouds`` (list of [n_i,3+C] views of one packed tensor),
    ``point_cloud_dims_min/max`` [B,3] and the eleven ``gt_*`` tensors [B,MAX_NUM_OBJ,...] of scannet.py:591-626.

    ``choices`` [B,num_points] int32/int64: output row j of scene b is the scene's row choices[b,j] (pc_util.random_sampling's
    ``pc[choices]``, repeats allowed) and the bounds cover the kept rows; a host array is range-checked here, a device tensor
    cannot be without a synchronisation (the kernel turns an index outside the scene into a row of NaN).  ``color_mean``: None
    leaves columns 3:6, negative is ``(rgb - MEAN_COLOR_RGB) / 256.0``, otherwise ``rgb / 255.0 - 0.5`` (scannet.py:453-456)."""
    off, sizes = _packed_scenes(points, offsets, 3, "prepare_scenes")
    dev = points.device
    B = len(off) - 1
    boxes, counts, classes = _box_tables(boxes, box_counts, box_classes, B)
    N, W = points.shape
    G = boxes.shape[1]
    M = int(dataset_config.max_num_obj if max_num_obj is None else max_num_obj)
    if G > M:
        raise ValueError(f"{G} box slots > max_num_obj {M}")
    if len(params) != B:
        raise ValueError(f"params describe {len(params)} scenes, offsets {B}")
    mode = L.VDETR_COLOR_KEEP if color_mean is None else L.VDETR_COLOR_MEAN if color_mean < 0 else L.VDETR_COLOR_UNIT
    if mode != L.VDETR_COLOR_KEEP and W < 6:
        raise ValueError(f"color_mean needs rgb in columns 3:6, points has {W} columns")

    num_points = 0
    if choices is not None:
        if not torch.is_tensor(choices):
            choices = torch.from_numpy(np.ascontiguousarray(choices))
        if choices.dim() != 2 or choices.shape[0] != B or choices.shape[1] < 1 or choices.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"choices must be int32 / int64 [{B}, num_points]")
        if not choices.is_cuda:
            c = choices.numpy()
            if (c < 0).any() or (c >= sizes[:, None]).any():
                raise ValueError("choices hold a row outside their scene")
            choices = choices.to(dev, non_blocking=True)
        choices = choices.contiguous()
        num_points = choices.shape[1]
    keep_rows = [num_points] * B if num_points else sizes.tolist()
    rows = int(sum(keep_rows))

    points = points.detach().contiguous()
    off32, off_dev, host = _upload_offsets(off, dev)
    table = torch.from_numpy(params.table()).to(dev, non_blocking=True)
    mean = torch.from_numpy(np.ascontiguousarray(dataset_config.mean_size_arr, dtype=np.float64)).to(dev, non_blocking=True)

    f32 = dict(dtype=torch.float32, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    out = torch.empty((rows, W), **f32)
    ret = {"point_cloud_dims_min": torch.empty((B, 3), **f32), "point_cloud_dims_max": torch.empty((B, 3), **f32),
           "gt_box_corners": torch.empty((B, M, 8, 3), **f32), "gt_box_centers": torch.empty((B, M, 3), **f32),
           "gt_box_centers_normalized": torch.empty((B, M, 3), **f32), "gt_angle_class_label": torch.empty((B, M), **i64),
           "gt_angle_residual_label": torch.empty((B, M), **f32), "gt_box_sem_cls_label": torch.empty((B, M), **i64),
           "gt_box_present": torch.empty((B, M), **f32), "gt_box_sizes": torch.empty((B, M, 3), **f32),
           "gt_box_sizes_normalized": torch.empty((B, M, 3), **f32), "gt_box_sizes_residual_label": torch.empty((B, M, 3), **f32),
           "gt_box_angles": torch.empty((B, M), **f32)}
    ret["point_clouds"] = list(torch.split(out, keep_rows)) if B else []
    if B == 0:
        return ret

    d = L.ScenePrepDesc()
    d.B, d.C, d.G, d.max_obj, d.num_points, d.color_mode = B, W - 3, G, M, num_points, mode
    d.num_classes, d.choices_i64 = mean.shape[0], int(choices is not None and choices.dtype == torch.int64)
    d.points, d.offsets, d.params, d.mean_size = points.data_ptr(), off_dev.data_ptr(), table.data_ptr(), mean.data_ptr()
    d.choices = choices.data_ptr() if choices is not None else None
    d.boxes, d.box_counts, d.box_classes = boxes.data_ptr(), counts.data_ptr(), classes.data_ptr()
    d.out_points, d.dims_min, d.dims_max = out.data_ptr(), ret["point_cloud_dims_min"].data_ptr(), ret["point_cloud_dims_max"].data_ptr()
    for field, key in (("corners", "gt_box_corners"), ("centers", "gt_box_centers"), ("centers_norm", "gt_box_centers_normalized"),
                       ("sizes", "gt_box_sizes"), ("sizes_norm", "gt_box_sizes_normalized"),
                       ("size_residual", "gt_box_sizes_residual_label"), ("angle_class", "gt_angle_class_label"),
                       ("sem_cls", "gt_box_sem_cls_label"), ("angle_residual", "gt_angle_residual_label"),
                       ("angles", "gt_box_angles"), ("present", "gt_box_present")):
        setattr(d, field, ret[key].data_ptr())
    nbytes = L.lib().vdetr_scene_prep_workspace_bytes(host, B, num_points)
    ws = L.workspace(nbytes, dev)
    _launch_pair(d, host, ws, nbytes)
    return ret


def _launch_pair(d, host_offsets, ws, nbytes):
    """the two launches on the current stream (tools/scene_prep_bench.py times exactly this)"""
    lib, stream = L.lib(), L.stream_ptr()
    L.check(lib.vdetr_scene_prep_points_f32(ctypes.byref(d), host_offsets, L.ptr(ws), nbytes, stream), "scene_prep_points")
    L.check(lib.vdetr_scene_prep_targets_f32(ctypes.byref(d), host_offsets, L.ptr(ws), nbytes, stream), "scene_prep_targets")


# ---- the cuboid crop and the sampling after it (reference utils/random_cuboid.py, pc_util.random_sampling) -----------
@dataclass
class CuboidTrials:
    """One scene's attempts as random_cuboid.py:43-50 draws them: ``crop_range`` [T,3] float64, ``center`` [T] int64 (the row
    the crop is centred on; -1 where the aspect test failed and none was drawn), ``valid`` [T] bool, and ``states``: the
    generator's state just after each attempt."""
    crop_range: np.ndarray
    center: np.ndarray
    valid: np.ndarray
    states: list
    random: object

    def rewind(self, trial):
        """puts the generator to "just after attempt ``trial``"; -1 (the fallback) is after the last attempt"""
        self.random.set_state(self.states[trial])


def _aspect_ok(crop, aspect):
    """the smaller over the larger edge of the xy, xz or yz face reaches ``aspect`` (float64 quotients)"""
    pairs = crop[[[0, 1], [0, 2], [1, 2]]]
    return bool((pairs.min(1) / pairs.max(1) >= aspect).any())


def draw_cuboid_trials(n_points, random=np.random, *, aspect=0.8, min_crop=0.5, max_crop=1.0, max_trials=100):
    """Draws ``max_trials`` attempts for a scene of ``n_points`` rows from ``random`` (``np.random`` or a ``RandomState``): every
    attempt takes ``rand(3)``; one whose aspect test passes, which is decided here, also takes ``choice(n_points)``.  The
    reference stops at the attempt it accepts, which depends on the points: ``CuboidTrials.rewind`` puts the generator back
    there once the device has said which one it was.  Host only."""
    crop = np.zeros((max_trials, 3))
    center = np.full(max_trials, -1, np.int64)
    valid = np.zeros(max_trials, bool)
    states = []
    for t in range(max_trials):
        crop[t] = min_crop + random.rand(3) * (max_crop - min_crop)
        valid[t] = _aspect_ok(crop[t], aspect)
        if valid[t]:
            center[t] = random.choice(n_points)
        states.append(random.get_state())
    return CuboidTrials(crop, center, valid, states, random)


def crop_and_sample(points, offsets, boxes, box_counts, box_classes, randoms, num_points, *, min_points=30000, aspect=0.8,
                    min_crop=0.5, max_crop=1.0, max_trials=100, filter_boxes=None):
    """``RandomCuboid`` and ``random_sampling`` of the training split (scannet.py:476-498) for a packed batch.  points / offsets
    / box_counts / box_classes as in ``prepare_scenes``; boxes [B,G,6] float32 or float64 (the reference filters on the file's
    array); ``randoms``: B distinct legacy generators (``RandomState`` or the ``np.random`` module), one per scene; from a
    generator's state at the call this reproduces the reference's crop and sampling of that scene and leaves the generator
    where the reference leaves it.  ``filter_boxes`` host bool [B]: whether an attempt must keep a box centre (default
    ``box_counts > 0``; the reference's literal test is ``instance_bboxes.sum() > 0`` over all seven columns of the file).

    -> dict: ``choices`` int32 [B,num_points] on the device, rows of the original scene (for ``prepare_scenes(choices=...)`` and
    for the loader's per-point labels); ``boxes`` / ``box_counts`` / ``box_classes``: the kept boxes in their order, zero rows
    after them, shapes unchanged; ``trial`` host [B]: the accepted attempt or -1 for the fallback (scene and boxes unchanged);
    ``kept_points`` host [B]; ``kept_rows``: per scene a device view of the crop's rows, ascending.

    Six launches whatever B and the number of attempts (csrc/cuboid.hip) and ONE read-back of (trial, kept points, kept
    boxes) per scene, the call's only synchronisation.  It is inherent: ``np.random.choice(n_kept, num_points, replace=n_kept <
    num_points)`` consumes the stream differently for every ``n_kept``.  No CPU path."""
    off, sizes = _packed_scenes(points, offsets, 3, "crop_and_sample")
    dev = points.device
    B = len(off) - 1
    boxes, counts, classes = _box_tables(boxes, box_counts, box_classes, B, (torch.float32, torch.float64))
    N, W = points.shape
    G = boxes.shape[1]
    num_points, min_points, max_trials = int(num_points), int(min_points), int(max_trials)
    if num_points < 1:
        raise ValueError(f"num_points {num_points} < 1")
    if min_points < 1:
        raise ValueError(f"min_points {min_points} < 1 (an empty crop has no bounds)")
    if not 1 <= max_trials <= L.VDETR_CUBOID_MAX_TRIALS:
        raise ValueError(f"max_trials {max_trials} outside 1 .. {L.VDETR_CUBOID_MAX_TRIALS}")
    randoms = list(randoms)
    if len(randoms) != B:
        raise ValueError(f"{len(randoms)} generators for {B} scenes")
    if len({id(r) for r in randoms}) != B:
        raise ValueError("two scenes share a generator: a scene's draws would start where another scene's end, which depends on "
                         "its points (call scene by scene with B = 1 for one stream)")
    if filter_boxes is not None:
        filter_boxes = np.asarray(filter_boxes, bool)
        if filter_boxes.shape != (B,):
            raise ValueError(f"filter_boxes must be a host bool array [{B}]")

    points = points.detach().contiguous()
    ret = {"boxes": torch.empty_like(boxes), "box_counts": torch.empty_like(counts), "box_classes": torch.empty_like(classes),
           "choices": torch.empty((B, num_points), dtype=torch.int32, device=dev), "trial": np.zeros(B, np.int64),
           "kept_points": np.zeros(B, np.int64), "kept_rows": []}
    if B == 0:
        return ret

    # 1. host: every scene's attempts, one table
    trials = [draw_cuboid_trials(int(n), r, aspect=aspect, min_crop=min_crop, max_crop=max_crop, max_trials=max_trials)
              for n, r in zip(sizes, randoms)]
    table = np.zeros((B, max_trials + 1, L.VDETR_CUBOID_TRIAL))
    for b, t in enumerate(trials):
        table[b, :max_trials, :3], table[b, :max_trials, 3] = t.crop_range, t.center
    filter_dev = None
    if filter_boxes is None:
        filter_dev = (counts > 0).to(torch.float64)                    # stays on the device: no read-back for the default
    else:
        table[:, max_trials, 0] = filter_boxes
    table = torch.from_numpy(table).to(dev, non_blocking=True)
    if filter_dev is not None:
        table[:, max_trials, 0] = filter_dev
    off32, off_dev, host = _upload_offsets(off, dev)
    result = torch.empty((B, L.VDETR_CUBOID_RESULT), dtype=torch.int32, device=dev)
    kept_rows = torch.empty(N, dtype=torch.int32, device=dev)

    # 2. device: five launches
    d = L.CuboidDesc()
    d.B, d.W, d.G, d.T, d.min_points, d.boxes_f64, d.num_points = B, W, G, max_trials, min(min_points, 2 ** 31 - 1), int(
        boxes.dtype == torch.float64), num_points
    d.points, d.offsets, d.trials = points.data_ptr(), off_dev.data_ptr(), table.data_ptr()
    d.boxes, d.box_counts, d.box_classes = boxes.data_ptr(), counts.data_ptr(), classes.data_ptr()
    d.out_boxes, d.out_counts, d.out_classes = ret["boxes"].data_ptr(), ret["box_counts"].data_ptr(), ret["box_classes"].data_ptr()
    d.result, d.kept_rows, d.choices = result.data_ptr(), kept_rows.data_ptr(), ret["choices"].data_ptr()
    nbytes = L.lib().vdetr_cuboid_workspace_bytes(host, B, max_trials)
    ws = L.workspace(nbytes, dev)
    alive = (points, boxes, counts, classes, table, off_dev, result, kept_rows, ret)
    _launch_crop(d, host, ws, nbytes, alive)

    # 3. the one read-back
    res = result.cpu().numpy()
    ret["trial"], ret["kept_points"] = res[:, 0].astype(np.int64), res[:, 1].astype(np.int64)
    ret["kept_rows"] = [kept_rows[off[b]:off[b] + res[b, 1]] for b in range(B)]

    # 4. host: every generator to where the reference stopped drawing attempts, then the sample as random_sampling draws it
    drawn = np.empty((B, num_points), np.int32)
    for b, t in enumerate(trials):
        t.rewind(int(res[b, 0]))
        n_kept = int(res[b, 1])
        drawn[b] = t.random.choice(n_kept, num_points, replace=n_kept < num_points)

    # 5. device: choices[b, j] = kept_rows[b][drawn[b, j]]
    drawn_dev = torch.from_numpy(drawn).to(dev, non_blocking=True)
    d.drawn = drawn_dev.data_ptr()
    _launch_compose(d, host, alive + (drawn_dev,))
    return ret


def _launch_crop(d, host_offsets, ws, nbytes, alive):
    """the five launches on the current stream (tools/cuboid_bench.py times exactly these and holds on to ``alive``, the tensors
    the descriptor points into)"""
    L.check(L.lib().vdetr_cuboid_crop_f32(ctypes.byref(d), host_offsets, L.ptr(ws), nbytes, L.stream_ptr()), "cuboid_crop")


def _launch_compose(d, host_offsets, alive):
    L.check(L.lib().vdetr_cuboid_compose_i32(ctypes.byref(d), host_offsets, L.stream_ptr()), "cuboid_compose")


# ---- the colour augmentations, the height channel, the SUN RGB-D colour step (csrc/color_aug.hip) ----------------------
@dataclass
class ColorAugmentParams:
    """One scene's draws of scannet.py:436-451.  ``keep`` bool [N] (False: the row's colour is dropped) or None when
    ``color_drop`` is 0; ``blend`` the contrast's blend factor or None (gate not fired); ``noise`` float64 [N,3], already times
    ``std * 255``, or None; ``hue_val`` / ``sat_ratio`` or None."""
    n_points: int
    keep: object = None
    blend: object = None
    noise: object = None
    hue_val: object = None
    sat_ratio: object = None


def _hue_sat_fields(hue_sat):
    hue, sat, p = hue_sat.split("_") if isinstance(hue_sat, str) else hue_sat
    return float(hue), float(sat), float(p)


def draw_color_augment(n_points, random=np.random, *, color_drop=0.0, color_contrastp=0.0, color_jitterp=0.0, hue_sat="0_0_0",
                       jitter_std=0.005):
    """Draws one scene's colour parameters from ``random`` (``np.random`` or a ``RandomState``) as scannet.py:436-451 consumes
    the stream: ``random(N)`` only if color_drop > 0; the contrast's gate only if color_contrastp > 0 and its blend only if the
    gate fires; the jitter's gate, then ``randn(N, 3)`` only if it fires; the hue / saturation gate only if the last field of
    ``hue_sat`` ("hue_sat_p", the reference's option string, or the three numbers) is > 0, then the two draws only if it fires.
    The Gaussian stays on the host: the legacy generator's polar rejection loop runs log and sqrt in libm's float64, and only
    the same code gives the same bits.  Host only."""
    n = int(n_points)
    p = ColorAugmentParams(n)
    if color_drop > 0:
        p.keep = random.random(n) > color_drop
    if color_contrastp > 0 and random.random() < color_contrastp:
        p.blend = random.random()
    if color_jitterp > 0 and random.random() < color_jitterp:
        p.noise = random.randn(n, 3)
        p.noise *= jitter_std * 255
    hue_max, sat_max, hue_p = _hue_sat_fields(hue_sat)
    if hue_p > 0 and random.random() < hue_p:
        p.hue_val = (random.random() - 0.5) * 2 * hue_max
        p.sat_ratio = 1 + (random.random() - 0.5) * 2 * sat_max
    return p


@dataclass
class SunrgbdColorParams:
    """One scene's draws of scannet.py:546-558: ``brightness`` [3], ``shift`` [3], ``jitter`` [n] float64, ``keep`` bool [n]."""
    brightness: np.ndarray
    shift: np.ndarray
    jitter: np.ndarray
    keep: np.ndarray


def draw_sunrgbd_color(n_rows, random=np.random):
    """``random(3)``, ``random(3)``, ``random(n)``, ``random(n)`` put through the expressions of scannet.py:546-558; called after
    ``draw_augment_params`` for the same scene.  Host only."""
    n = int(n_rows)
    brightness = 1 + 0.4 * random.random(3) - 0.2
    shift = 0.1 * random.random(3) - 0.05
    jitter = 0.05 * random.random(n) - 0.025
    return SunrgbdColorParams(brightness, shift, jitter, random.random(n) > 0.3)


def _color_desc(points, out, off_dev):
    d = L.ColorAugDesc()
    d.B, d.W = len(off_dev) - 1, points.shape[1]
    d.points, d.offsets, d.out = points.data_ptr(), off_dev.data_ptr(), out.data_ptr()
    return d


def augment_colors(points, offsets, params):
    """The four ``--use_color`` augmentations (scannet.py:436-451) on a packed batch: points [N,3+C] f32 with rgb (0 .. 255) in
    columns 3:6, offsets [B+1] as in ``prepare_scenes``, params: B ``ColorAugmentParams`` (``draw_color_augment``) -> a new
    [N,3+C] tensor; columns 3:6 are augmented, every other column is copied, the input is left alone.  Three launches on the
    current stream whatever B and whichever gates fired; the result equals the reference's bit for bit.  No CPU path."""
    off, sizes = _packed_scenes(points, offsets, 6, "augment_colors")
    params = list(params)
    B = len(off) - 1
    if len(params) != B or any(p.n_points != n for p, n in zip(params, sizes)):
        raise ValueError(f"params must hold one ColorAugmentParams per scene, drawn for its row count ({B} scenes)")
    dev = points.device
    points = points.detach().contiguous()
    out = torch.empty_like(points)
    if B == 0:
        return out
    N = points.shape[0]
    table = np.zeros((B, L.VDETR_COLOR_AUG_PARAMS))
    table[:, 3] = -1
    noise, noise_rows = [], 0
    keep = np.ones(N, bool) if any(p.keep is not None for p in params) else None
    for b, p in enumerate(params):
        if p.keep is not None:
            table[b, 7] = 1
            keep[off[b]:off[b + 1]] = p.keep
        if p.blend is not None:
            table[b, :3] = 1, 1 - p.blend, p.blend
        if p.noise is not None:
            table[b, 3] = noise_rows
            noise.append(np.asarray(p.noise, np.float64).reshape(-1, 3))
            noise_rows += len(noise[-1])
        if p.hue_val is not None:
            table[b, 4:7] = 1, p.hue_val, p.sat_ratio
    off32, off_dev, host = _upload_offsets(off, dev)
    d = _color_desc(points, out, off_dev)
    table_dev = torch.from_numpy(table).to(dev, non_blocking=True)
    keep_dev = torch.from_numpy(keep.view(np.uint8)).to(dev, non_blocking=True) if keep is not None else None
    noise_dev = torch.from_numpy(np.ascontiguousarray(np.concatenate(noise))).to(dev, non_blocking=True) if noise else None
    d.params, d.noise_rows = table_dev.data_ptr(), noise_rows
    d.keep = keep_dev.data_ptr() if keep_dev is not None else None
    d.noise = noise_dev.data_ptr() if noise_dev is not None else None
    nbytes = L.lib().vdetr_color_aug_workspace_bytes(host, B)
    ws = L.workspace(nbytes, dev)
    _launch_colors(d, host, ws, nbytes, (points, out, off_dev, table_dev, keep_dev, noise_dev))
    return out


def _launch_colors(d, host_offsets, ws, nbytes, alive):
    """the three launches on the current stream (tools/color_aug_bench.py times exactly these)"""
    L.check(L.lib().vdetr_color_augment_f32(ctypes.byref(d), host_offsets, L.ptr(ws), nbytes, L.stream_ptr()), "color_augment")


def percentile_plan(n, percent=0.99):
    """What ``np.percentile(z, percent)`` (method "linear", numpy 2.2) takes from a float32 column of n values: the indices of the
    two order statistics and the float32 weight between them.  All of it is float32 arithmetic on n alone:
    q = float32(percent) / float32(100); the virtual index (n - 1) * q in float32; its floor and the floor + 1, both n - 1 once
    the virtual index reaches n - 1; the weight is the virtual index minus its floor."""
    q = np.float32(percent) / np.float32(100)
    virtual = np.float32(n - 1) * q
    lower = int(np.floor(virtual))
    upper = lower + 1
    if virtual >= n - 1:
        lower = upper = n - 1
    gamma = np.float32(np.float64(virtual) - (-1 if virtual >= n - 1 else lower))
    return lower, upper, gamma


def append_height(points, offsets):
    """``use_height`` (scannet.py:461-464) on a packed batch: -> [N,3+C+1], the last column ``z - np.percentile(z, 0.99)`` of the
    row's scene (a NaN in the column makes the floor NaN); it comes before ``crop_and_sample`` and then travels as an ordinary
    extra channel.  The two order statistics are found by a radix select, not a sort: nine launches whatever B and the data,
    two runs give the same bits.  No CPU path."""
    off, sizes = _packed_scenes(points, offsets, 3, "append_height")
    B = len(off) - 1
    dev = points.device
    points = points.detach().contiguous()
    out = torch.empty((points.shape[0], points.shape[1] + 1), dtype=torch.float32, device=dev)
    if B == 0:
        return out
    select = np.zeros((B, L.VDETR_HEIGHT_SELECT), np.int32)
    for b, n in enumerate(sizes):
        lower, upper, gamma = percentile_plan(int(n))
        select[b, :3] = lower, upper, np.array(gamma, np.float32).view(np.int32)
    off32, off_dev, host = _upload_offsets(off, dev)
    d = _color_desc(points, out, off_dev)
    select_dev = torch.from_numpy(select).to(dev, non_blocking=True)
    d.select = select_dev.data_ptr()
    nbytes = L.lib().vdetr_append_height_workspace_bytes(host, B)
    ws = L.workspace(nbytes, dev)
    _launch_height(d, host, ws, nbytes, (points, out, off_dev, select_dev))
    return out


def _launch_height(d, host_offsets, ws, nbytes, alive):
    L.check(L.lib().vdetr_append_height_f32(ctypes.byref(d), host_offsets, L.ptr(ws), nbytes, L.stream_ptr()), "append_height")


def sunrgbd_color_augment(point_clouds, offsets, params):
    """``--coloraug_sunrgbd`` (scannet.py:544-560), in place on the packed tensor behind ``prepare_scenes``' ``point_clouds`` (the
    list of views, or the packed [rows,3+C] tensor itself), whose colours are already normalised; offsets [B+1]: the scenes' rows
    in it; params: B ``SunrgbdColorParams`` (``draw_sunrgbd_color``).  One launch; returns ``point_clouds``.  No CPU path."""
    packed = point_clouds
    if not torch.is_tensor(point_clouds):
        views = list(point_clouds)
        if not views:
            return point_clouds
        packed = views[0]._base if views[0]._base is not None else views[0]
        L.require_gpu(packed, "point_clouds")
        at = packed.data_ptr()
        for v in views:
            if v.dim() != 2 or v.shape[1] != packed.shape[1] or not v.is_contiguous() or v.data_ptr() != at:
                raise ValueError("point_clouds must be consecutive row blocks of one packed tensor (prepare_scenes' list)")
            at += v.numel() * 4
    off, sizes = _packed_scenes(packed, offsets, 6, "sunrgbd_color_augment")
    if not packed.is_contiguous():
        raise ValueError("point_clouds must be contiguous: the step runs in place")
    params = list(params)
    B = len(off) - 1
    if len(params) != B or any(len(p.jitter) != n or len(p.keep) != n for p, n in zip(params, sizes)):
        raise ValueError(f"params must hold one SunrgbdColorParams per scene, drawn for its row count ({B} scenes)")
    if B == 0:
        return point_clouds
    dev = packed.device
    table = np.zeros((B, L.VDETR_COLOR_AUG_PARAMS))
    for b, p in enumerate(params):
        table[b, :3], table[b, 3:6] = p.brightness, p.shift
    off32, off_dev, host = _upload_offsets(off, dev)
    d = _color_desc(packed, packed, off_dev)
    table_dev = torch.from_numpy(table).to(dev, non_blocking=True)
    jitter_dev = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(p.jitter, np.float64) for p in params]))).to(dev, non_blocking=True)
    keep_dev = torch.from_numpy(np.concatenate([np.asarray(p.keep, bool) for p in params]).view(np.uint8)).to(dev, non_blocking=True)
    d.params, d.noise, d.keep, d.noise_rows = table_dev.data_ptr(), jitter_dev.data_ptr(), keep_dev.data_ptr(), packed.shape[0]
    _launch_sunrgbd(d, host, (packed, off_dev, table_dev, jitter_dev, keep_dev))
    return point_clouds


def _launch_sunrgbd(d, host_offsets, alive):
    L.check(L.lib().vdetr_sunrgbd_color_f32(ctypes.byref(d), host_offsets, L.stream_ptr()), "sunrgbd_color")


# ---- --use_normals: area-weighted vertex normals of the scan's mesh (csrc/normals.hip) ------------------------------
def vertex_normals(vertices, vert_offsets, faces, face_offsets, *, out=None):
    """``vertex_normal(coords, faces)`` of scannet.py:398-420 for a packed batch of meshes: vertices [N,3+] f32 (xyz first; any
    row stride, e.g. the seven columns ``read_plymesh`` returns), vert_offsets [B+1] as in ``prepare_scenes``, faces [F,3] int32 /
    int64 with indices local to their scene (a host array or a device tensor), face_offsets [B+1] (a scene without faces is
    legal) -> [N,3] f32 on the device, bit for bit the reference's serial loop: every vertex adds its incident faces' weights
    in ascending face index.  A vertex that no face names gets 0, 0, 0.  With ``out`` ([N,3] f32 on the device, rows strided at
    will, e.g. ``cloud9[:, 6:9]``) the normals are written there and ``out`` is returned; nothing else of its storage is touched.

    A host ``faces`` array is range-checked here; a device tensor cannot be without a synchronisation: the kernels turn a face
    with an index outside its scene into NaN normals for the face's in-range vertices and follow none of its indices.  Seven
    launches on the current stream whatever B, no synchronisation, two runs give the same bits.  No CPU path."""
    voff, sizes = _packed_scenes(vertices, vert_offsets, 3, "vertex_normals", name="vertices", strided=True, gpu=False)
    dev = vertices.device
    foff = _host_i32(face_offsets, "face_offsets")
    B, N = len(voff) - 1, vertices.shape[0]
    if len(foff) != B + 1:
        raise ValueError(f"face_offsets must hold {B + 1} offsets like vert_offsets, got {len(foff)}")
    if not torch.is_tensor(faces):
        faces = torch.from_numpy(np.ascontiguousarray(faces))
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"faces must be int32 / int64 [F, 3], got {faces.dtype} {tuple(faces.shape)}")
    F = faces.shape[0]
    if foff[0] != 0 or foff[-1] != F or (np.diff(foff) < 0).any() or 3 * F >= 2 ** 31:
        raise ValueError(f"face_offsets run from {foff[0]} to {foff[-1]} (they may not decrease), faces has {F} rows")
    if not faces.is_cuda:
        f = faces.numpy()
        if (f < 0).any() or (f >= np.repeat(sizes, np.diff(foff))[:, None]).any():
            raise ValueError("faces name a vertex outside their scene")
    L.require_gpu(vertices, "vertices")                                # after the host checks, which need no device
    if not faces.is_cuda:
        faces = faces.to(dev, non_blocking=True)
    faces = faces.detach().contiguous()
    vertices = vertices.detach()
    if out is None:
        out = torch.empty((N, 3), dtype=torch.float32, device=dev)
    else:
        L.require_gpu(out, "out")
        L.require_float(out, "out")
        if tuple(out.shape) != (N, 3) or (N and (out.stride(1) != 1 or out.stride(0) < 3)) or out.device != dev:
            raise ValueError(f"out must be a [{N}, 3] view with unit column stride on {dev}, got {tuple(out.shape)}")
    if B == 0:
        return out
    (voff32, voff_dev, vhost), (foff32, foff_dev, fhost) = _upload_offsets(voff, dev), _upload_offsets(foff, dev)
    d = L.NormalsDesc()
    d.B, d.vert_stride, d.out_stride, d.faces_i64 = B, vertices.stride(0), out.stride(0), int(faces.dtype == torch.int64)
    d.vertices, d.faces, d.out = vertices.data_ptr(), faces.data_ptr(), out.data_ptr()
    d.vert_offsets, d.face_offsets = voff_dev.data_ptr(), foff_dev.data_ptr()
    nbytes = L.lib().vdetr_vertex_normals_workspace_bytes(vhost, fhost, B)
    ws = L.workspace(nbytes, dev)
    _launch_normals(d, vhost, fhost, ws, nbytes, (vertices, faces, out, voff_dev, foff_dev, voff32, foff32))
    return out


def _launch_normals(d, vert_host, face_host, ws, nbytes, alive):
    """the seven launches on the current stream (tools/normals_bench.py times exactly these)"""
    L.check(L.lib().vdetr_vertex_normals_f32(ctypes.byref(d), vert_host, face_host, L.ptr(ws), nbytes, L.stream_ptr()), "vertex_normals")


def with_normals(points6, normals):
    """scannet.py:457-458: points6 [N,6] f32 (xyz, rgb: the reference appends normals under ``use_color`` only) and normals [N,3]
    -> the [N,9] cloud.  To skip this copy, allocate the [N,9] cloud first and pass ``cloud9[:, 6:9]`` as ``vertex_normals``' out."""
    if points6.dim() != 2 or points6.shape[1] != 6:
        raise ValueError(f"with_normals: points6 must be [N, 6] (normals are appended to a use_color cloud), got {tuple(points6.shape)}")
    if tuple(normals.shape) != (points6.shape[0], 3):
        raise ValueError(f"with_normals: normals must be [{points6.shape[0]}, 3], got {tuple(normals.shape)}")
    for t, name in ((points6, "points6"), (normals, "normals")):
        L.require_gpu(t, name)
        L.require_float(t, name)
    return torch.cat((points6, normals), 1)
