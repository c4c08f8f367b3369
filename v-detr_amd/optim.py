"""Gradient-norm clipping + AdamW on a ``dist.FlatParams`` buffer as one launch (csrc/optim.hip).

Reference: engine.py:105-107 (``clip_grad_norm_(model.parameters(), args.clip_gradient)`` then ``optimizer.step()``) with the
``torch.optim.AdamW`` of optimizer.py:6-26.  Host side of ``vdetr_adamw_clip_f32``: a ``torch.optim.Optimizer`` whose one parameter is
the flat buffer and whose state has torch's AdamW keys (``step``, ``exp_avg``, ``exp_avg_sq``: ``FlatParams.per_param_optimizer_state`` /
``load_per_param_optimizer_state`` and torch's own ``state_dict`` / ``load_state_dict`` keep working), so that a script built on the
reference's optimizer swaps one constructor.  The sum of squares behind the norm comes out of the gradient pack's launch
(``FlatParams.pack_grads``) where the flat gradient is final there, or out of one more launch where it was all-reduced afterwards.
With a learning-rate table (engine.py:24-56) and / or a no-decay mask (optimizer.py:11-15, ``--filter_biases_wd``) the launch is
``vdetr_adamw_sched_f32``: the rate of every step is read on the device, indexed by the device-resident step count, so that a
captured step follows the schedule.  ``step(skip=flag)`` is ``vdetr_adamw_guard_f32``: the same launch behind an int32 device word
(the training loop's non-finite-loss flag, engine.LossMeter): nonzero, and the launch touches nothing.  GPU only, fp32 only: there is
no CPU path.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L


def compute_learning_rate(args, curr_epoch_normalized):
    """The rate of engine.py:24-49 at ``curr_epoch_normalized`` = iteration / all iterations, in Python floats and in the
    reference's operation order (the value is compared with ``==``): linear warm-up from ``warm_lr`` to ``base_lr`` over
    ``warm_lr_epochs``, then a half cosine down to ``final_lr`` (``lr_scheduler == "cosine"``) or ``base_lr``, a tenth and a hundredth of
    it with the changes at the two epochs of ``step_epoch`` ("12_16")."""
    t = curr_epoch_normalized
    assert 0.0 <= t <= 1.0
    if args.warm_lr_epochs > 0 and t <= (args.warm_lr_epochs / args.max_epoch):
        return args.warm_lr + t * args.max_epoch * ((args.base_lr - args.warm_lr) / args.warm_lr_epochs)
    if args.lr_scheduler == "cosine":
        return args.final_lr + 0.5 * (args.base_lr - args.final_lr) * (1 + math.cos(math.pi * t))
    first, second = (int(e) for e in args.step_epoch.split("_"))
    if t < (first / args.max_epoch):
        return args.base_lr
    if t < (second / args.max_epoch):
        return args.base_lr / 10
    return args.base_lr / 100


def lr_table(args, iters_per_epoch):
    """Every iteration's rate of a whole run (engine.py:70-81: ``compute_learning_rate(args, curr_iter / max_iters)`` before
    iteration ``curr_iter``): float64 [max_epoch * iters_per_epoch], what ``ClipAdamW(lr_schedule=...)`` indexes by its step count."""
    max_iters = int(args.max_epoch) * int(iters_per_epoch)
    return np.array([compute_learning_rate(args, i / max_iters) for i in range(max_iters)], dtype=np.float64)


def build_optimizer(args, model, flat, iters_per_epoch=None):
    """optimizer.py:4-26 for the flat buffer: AdamW at ``args.base_lr`` / ``args.weight_decay`` behind ``clip_grad_norm_`` where
    ``args.clip_gradient > 0`` (engine.py:105-106), no decay for 1-D parameters and ``*.bias`` under ``args.filter_biases_wd``; with
    ``iters_per_epoch`` the schedule of engine.py:24-56 as well."""
    mask = flat.decay_mask(model.named_parameters()) if args.filter_biases_wd else None
    table = lr_table(args, iters_per_epoch) if iters_per_epoch is not None else None
    return ClipAdamW(flat, lr=args.base_lr, weight_decay=args.weight_decay, max_norm=args.clip_gradient if args.clip_gradient > 0 else None,
                     lr_schedule=table, decay_mask=mask)


class ClipAdamW(torch.optim.Optimizer):
    step_on_device = True  # (FlatParams.load_per_param_optimizer_state) state["step"] is read by the kernel

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None, norm_from_pack=True,
                 lr_schedule=None, decay_mask=None, lr_offset=0):
        """flat: dist.FlatParams.  max_norm: the ``clip_grad_norm_`` bound (None: no clipping).  norm_from_pack: the flat gradient is
        final when ``flat.pack_grads()`` returns (one rank); False: it changes afterwards (all-reduce) and the norm takes a launch.
        lr_schedule: one rate per step (``lr_table``): a 1-D float64 numpy array, uploaded once, or a 1-D float64 tensor on the
        buffer's device, used as it is; step k (from 0) runs at entry ``clamp(k + lr_offset, 0, len - 1)``, k being the
        device-resident ``state["step"]``: a captured ``step()`` follows the schedule, and so does a resumed one.  ``lr`` stays
        the rate without a schedule.  decay_mask: ``flat.decay_mask(...)``: the elements ``weight_decay`` applies to (None: all).
        A capture bakes in the POINTERS of the table and the mask and ``lr_offset``, like every other scalar: ``set_lr_offset``
        after a capture changes eager steps only."""
        if not (flat.data.is_cuda and flat.data.dtype == torch.float32):
            raise RuntimeError("ClipAdamW: an fp32 FlatParams buffer on the GPU (there is no CPU path)")
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError(f"ClipAdamW: lr {lr} betas {betas} eps {eps} weight_decay {weight_decay}")
        dev = flat.data.device
        table = self._checked_table(lr_schedule, dev)
        mask = self._checked_mask(decay_mask, flat.data.numel(), dev)
        super().__init__([flat.param], dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.flat = flat
        self.max_norm = None if max_norm is None else float(max_norm)
        self.norm_from_pack = bool(norm_from_pack)
        st = self.state[flat.param]
        st["step"] = torch.zeros((), dtype=torch.float32, device=dev)
        st["exp_avg"] = torch.zeros_like(flat.data)
        st["exp_avg_sq"] = torch.zeros_like(flat.data)
        self._ticket = torch.zeros(4, dtype=torch.int32, device=dev)
        self.grad_norm = torch.zeros((), dtype=torch.float32, device=dev)  # ||g|| of the last step (what clip_grad_norm_ returns)
        self._own_partials = None
        self.lr_schedule, self.decay_mask, self.lr_offset = table, mask, int(lr_offset)
        self.last_lr = torch.full((), float(lr), dtype=torch.float64, device=dev)  # the rate of the last scheduled / masked step
        if self.max_norm is not None and self.norm_from_pack:
            flat.want_sumsq = True  # pack_grads() leaves flat.sumsq from now on

    @staticmethod
    def _checked_table(table, dev):
        if table is None:
            return None
        if isinstance(table, np.ndarray):
            if table.dtype != np.float64 or table.ndim != 1:
                raise ValueError(f"ClipAdamW: lr_schedule must be 1-D float64, got {table.dtype} {table.shape}")
            host = torch.from_numpy(np.ascontiguousarray(table))
        elif torch.is_tensor(table):
            if table.dtype != torch.float64 or table.ndim != 1 or not table.is_contiguous():
                raise ValueError(f"ClipAdamW: lr_schedule must be contiguous 1-D float64, got {table.dtype} {tuple(table.shape)}")
            if table.device != dev:
                raise ValueError(f"ClipAdamW: an lr_schedule tensor must be on {dev} (it is on {table.device}); a numpy array is uploaded")
            host = table.cpu()
        else:
            raise ValueError("ClipAdamW: lr_schedule must be a numpy array or a tensor")
        if host.numel() == 0:
            raise ValueError("ClipAdamW: empty lr_schedule")
        if not bool((torch.isfinite(host) & (host >= 0)).all()):  # (the kernel cannot report an entry it does not like)
            raise ValueError("ClipAdamW: lr_schedule has a negative or non-finite entry")
        return table if torch.is_tensor(table) else host.to(dev)

    @staticmethod
    def _checked_mask(mask, n, dev):
        if mask is None:
            return None
        words = (n + 31) // 32
        if not (torch.is_tensor(mask) and mask.dtype in (torch.int32, torch.uint32) and mask.ndim == 1 and mask.is_contiguous()):
            raise ValueError("ClipAdamW: decay_mask must be a contiguous 1-D int32 / uint32 tensor (FlatParams.decay_mask)")
        if mask.numel() != words:
            raise ValueError(f"ClipAdamW: decay_mask has {mask.numel()} words, {n} elements take {words}")
        if mask.device != dev:
            raise ValueError(f"ClipAdamW: decay_mask must be on {dev} (it is on {mask.device})")
        return mask

    def set_lr_offset(self, k):
        """Entry ``step + k`` of the schedule from the next EAGER ``step()`` on (a captured one keeps the offset it was captured with)."""
        self.lr_offset = int(k)

    def _check_state(self):
        """``step`` as a float32 scalar on the buffer's device (the kernel reads and writes it: a checkpoint loaded with
        ``map_location="cpu"`` leaves it on the host), the moments as what the kernel updates."""
        flat = self.flat
        st = self.state[flat.param]
        missing = [k for k in ("step", "exp_avg", "exp_avg_sq") if k not in st]
        if missing:
            raise RuntimeError(f"ClipAdamW: the loaded state lacks {missing}")
        step = torch.as_tensor(st["step"])
        if step.numel() != 1:
            raise RuntimeError(f"ClipAdamW: state['step'] has {step.numel()} elements")
        st["step"] = step.detach().reshape(()).to(device=flat.data.device, dtype=torch.float32, copy=True)
        for k in ("exp_avg", "exp_avg_sq"):
            t = st[k]
            if not (torch.is_tensor(t) and t.device == flat.data.device and t.dtype == torch.float32 and t.is_contiguous()
                    and t.numel() == flat.data.numel()):
                raise RuntimeError(f"ClipAdamW: state[{k!r}] must be {flat.data.numel()} fp32 elements on {flat.data.device}, got "
                                   f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)} "
                                   "(a state saved under another FlatParams layout goes through load_per_param_optimizer_state)")

    def load_state_dict(self, state_dict):
        """torch's, then ``step`` back on the device: a checkpoint read with ``map_location="cpu"`` (utils/io.py:48-54) is fine."""
        super().load_state_dict(state_dict)
        self._check_state()

    @staticmethod
    def _checked_skip(skip, dev):
        if not (torch.is_tensor(skip) and skip.dtype == torch.int32):
            raise ValueError(f"ClipAdamW: skip must be an int32 tensor, got {getattr(skip, 'dtype', type(skip))}")
        if skip.numel() != 1:
            raise ValueError(f"ClipAdamW: skip has {skip.numel()} elements, the launch reads one word")
        if skip.device != dev:
            raise ValueError(f"ClipAdamW: skip must be on {dev} (it is on {skip.device})")
        return skip

    @torch.no_grad()
    def step(self, closure=None, skip=None):
        """One launch.  ``skip``: an int32 device scalar (``engine.LossMeter.bad_flag``) that the launch reads first
        (``vdetr_adamw_guard_f32``): nonzero leaves parameters, moments, step count, ``grad_norm`` and ``last_lr`` as they are; zero is
        the step without ``skip``, bit for bit.  None: the unguarded launches."""
        if closure is not None:
            raise RuntimeError("ClipAdamW: closures are not supported")
        flat, lib = self.flat, L.lib()
        if skip is not None:
            skip = self._checked_skip(skip, flat.data.device)
        g = self.param_groups[0]
        st = self.state[flat.param]
        if st["step"].device != flat.data.device:
            raise RuntimeError(f"ClipAdamW: state['step'] is on {st['step'].device}, the kernel reads it on {flat.data.device}")
        sched = self.lr_schedule is not None or self.decay_mask is not None
        d = L.AdamWGuardDesc() if skip is not None else L.AdamWSchedDesc() if sched else L.AdamWDesc()
        d.param, d.grad = flat.data.data_ptr(), flat.grad.data_ptr()
        d.exp_avg, d.exp_avg_sq = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
        d.n = flat.data.numel()
        d.step, d.ticket = st["step"].data_ptr(), self._ticket.data_ptr()
        d.sumsq, d.nsumsq = None, 0
        if self.max_norm is not None:
            part = getattr(flat, "sumsq", None) if self.norm_from_pack else None
            if part is None:  # the flat gradient as it is now
                n = flat.grad.numel()
                nb = lib.vdetr_sumsq_blocks(n)
                if self._own_partials is None:
                    self._own_partials = torch.empty(nb, dtype=torch.float32, device=flat.grad.device)
                part = self._own_partials
                L.check(lib.vdetr_sumsq_f32(flat.grad.data_ptr(), n, part.data_ptr(), nb, L.stream_ptr()), "sumsq")
            d.sumsq, d.nsumsq = part.data_ptr(), part.numel()
            d.max_norm, d.norm_eps = self.max_norm, 1e-6
            d.norm_out = self.grad_norm.data_ptr()
        d.lr, d.beta1, d.beta2 = float(g["lr"]), float(g["betas"][0]), float(g["betas"][1])
        d.eps, d.weight_decay = float(g["eps"]), float(g["weight_decay"])
        if not sched and skip is None:
            L.check(lib.vdetr_adamw_clip_f32(ctypes.byref(d), L.stream_ptr()), "adamw_clip")
            return None
        if self.lr_schedule is not None:
            d.lr_table, d.n_lr, d.lr_offset = self.lr_schedule.data_ptr(), self.lr_schedule.numel(), self.lr_offset
        if self.decay_mask is not None:
            d.decay_mask = self.decay_mask.data_ptr()
        d.lr_out = self.last_lr.data_ptr()
        if skip is not None:
            d.skip = skip.data_ptr()
            L.check(lib.vdetr_adamw_guard_f32(ctypes.byref(d), L.stream_ptr()), "adamw_guard")
            return None
        L.check(lib.vdetr_adamw_sched_f32(ctypes.byref(d), L.stream_ptr()), "adamw_sched")
        return None
