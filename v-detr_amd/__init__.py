"""vdetr_amd — MI355X (gfx950) native hot path of V-DETR.

Host side (this package): PyTorch-ROCm modules that keep the reference's module / operator API
(``models/vdetr_transformer.py``, ``models/helpers.py``, ``models/position_embedding.py``,
``third_party/pointnet2/pointnet2_utils.py``, the post-backbone part of ``models/model_vdetr.py``) and its
checkpoint key layout.  Device side: ``lib/libvdetr_hip.so`` (hand-written HIP kernels behind the C-ABI of
``include/vdetr_hip.h``), loaded through ctypes by ``_lib``.  There is no CPU fallback: every op raises when
its tensors are not on the GPU or when the HIP library is missing.
"""
__version__ = "0.1.0"

_SCENE_PREP = ("AugmentParams", "draw_augment_params", "prepare_scenes", "nyu40_to_class", "crop_and_sample", "draw_cuboid_trials",
               "CuboidTrials", "ColorAugmentParams", "draw_color_augment", "augment_colors", "append_height", "percentile_plan",
               "SunrgbdColorParams", "draw_sunrgbd_color", "sunrgbd_color_augment")
_SCAN_EXPORT = ("ScanTables", "scan_tables", "export_scans")
_OPTIM = ("ClipAdamW", "build_optimizer", "compute_learning_rate", "lr_table")


def __getattr__(name):
    # the scene preparation (scene_prep.py) is the package's loader-facing interface; resolved on first use so that importing the
    # package stays free of torch
    if name in _SCENE_PREP:
        from . import scene_prep
        return getattr(scene_prep, name)
    if name in _SCAN_EXPORT:  # the step in front of it: a raw scan to the loader's arrays (scan_export.py)
        from . import scan_export
        return getattr(scan_export, name)
    if name in _OPTIM:  # the training loop's optimizer (optim.py), the same way
        from . import optim
        return getattr(optim, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
