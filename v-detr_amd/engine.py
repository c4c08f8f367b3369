"""The reference's control plane (engine.py:24-193): ``train_one_epoch``, ``evaluate``, ``test_model`` (main.py:437-480: what
``--test_only`` runs on a checkpoint, with the S / M / L metrics of ``--test_size``) and the learning-rate helpers.  Both loops are eager; a captured (hipGraph) training step is NOT built here.

``evaluate`` is the reference's loop, statement for statement: batch to the model's device, ``model(inputs)`` on the three input
keys, the loss when a criterion is given, ``sigmoid`` for the focal-loss heads, ``all_gather_dict`` on outputs and batch, the
axis-aligned corners under ``--axis_align_test``, ``APCalculator.step_meter``, the progress line.  What differs is where the host
waits.  The reference reads the loss every batch (``loss_reduced.item()``) and ``step_meter`` copies seven tensors to the host; here
the last ten reduced losses stay device scalars until the loop has ended (``SmoothedValue(window_size=10).avg`` is their float32
mean) and the calculator is resident (``APCalculator(resident=True)``), so a batch's loop body reads nothing back
and the host can enqueue batch i+1 while the device finishes batch i.

``train_one_epoch`` (engine.py:59-122) has two forms, chosen by the optimizer.  With any ``torch.optim.Optimizer`` it is the
reference's loop as it stands, its two ``loss_reduced.item()`` reads per iteration included: the parity baseline, and what runs on
CPU tensors.  With ``optim.ClipAdamW`` it reads nothing back per iteration: the loss goes into a device-resident meter
(``LossMeter``, csrc/train_meter.hip) whose non-finite flag the optimizer's launch reads on the device
(``vdetr_adamw_guard_f32``), and the host copies the meter back only where the reference prints.
"""
import ctypes
import datetime
import logging
import math
import os
import sys
import time
from collections import deque
from types import SimpleNamespace

import torch

from . import _lib as L
from .ap_calculator import APCalculator
from .dist import all_gather_dict, all_reduce_average, barrier, batch_dict_to_cuda, is_primary, reduce_dict
from .optim import ClipAdamW, compute_learning_rate, lr_table  # noqa: F401  (engine.py:24-49; the table form ClipAdamW indexes)


def adjust_learning_rate(args, optimizer, curr_epoch):
    """engine.py:52-56"""
    curr_lr = compute_learning_rate(args, curr_epoch)
    for param_group in optimizer.param_groups:
        param_group["lr"] = curr_lr
    return curr_lr


def _window_stats(values):
    """``SmoothedValue``'s properties (utils/misc.py:71-91) of the deque ``values`` (Python floats, oldest first), by its own
    expressions; an empty deque reads as nan / None where the reference's ``median`` / ``max`` / ``value`` would raise."""
    if not values:
        return dict(avg=float("nan"), median=float("nan"), value=None, max=None)
    return dict(avg=torch.tensor(values, dtype=torch.float32).mean().item(), median=torch.tensor(values).median().item(),
                value=values[-1], max=max(values))


class LossMeter:
    """``SmoothedValue(window_size)`` plus the loop's ``math.isfinite`` check, resident on the device (csrc/train_meter.hip).
    ``update`` is one small launch and reads nothing back; ``read`` is ONE device-to-host copy of the 288-byte state block.
    ``bad_flag`` is the block's ``bad`` word as an int32 scalar: ``ClipAdamW.step(skip=meter.bad_flag)`` does nothing from the first
    non-finite loss on.  From then on the meter is frozen as well: later losses do not enter the window."""

    def __init__(self, window_size=10, device="cuda"):
        window_size = int(window_size)
        if not 1 <= window_size <= L.VDETR_LOSS_METER_MAX_WINDOW:
            raise ValueError(f"LossMeter: window_size {window_size} outside 1 .. {L.VDETR_LOSS_METER_MAX_WINDOW}")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"LossMeter: the state lives on the GPU (there is no CPU path), got {device}")
        host = L.LossMeterState(total=0.0, count=0, bad_iter=-1, bad=0, window=window_size)
        self.window_size = window_size
        self.state = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(device)
        off = L.LossMeterState.bad.offset
        self.bad_flag = self.state[off:off + 4].view(torch.int32).reshape(())
        self.reads = 0

    def update(self, loss, curr_iter):
        """enqueue: the loss (a one-element tensor on the meter's device) enters the window, or raises the flag at ``curr_iter``"""
        if not (torch.is_tensor(loss) and loss.numel() == 1 and loss.device == self.state.device):
            raise ValueError(f"LossMeter.update: a one-element tensor on {self.state.device}, got "
                             f"{tuple(getattr(loss, 'shape', ()))} on {getattr(loss, 'device', type(loss))}")
        loss = loss.detach()
        if loss.dtype != torch.float32:
            loss = loss.to(torch.float32)
        d = L.LossMeterDesc(loss=loss.data_ptr(), state=self.state.data_ptr(), iter=int(curr_iter))
        L.check(L.lib().vdetr_loss_meter_update_f32(ctypes.byref(d), L.stream_ptr()), "loss_meter_update")

    def read(self):
        """The one copy: a snapshot with ``SmoothedValue``'s ``avg``, ``median``, ``global_avg``, ``value``, ``max``, ``count``,
        ``total`` (equal to the reference's with ``==``) and the flag, ``bad`` / ``bad_iter``.  Waits for the stream."""
        self.reads += 1
        st = L.LossMeterState.from_buffer_copy(self.state.cpu().numpy().tobytes())
        return snapshot(st.total, st.count, st.bad, st.bad_iter, st.window, list(st.ring))


def snapshot(total, count, bad, bad_iter, window, ring):
    """the fields of ``LossMeter.read()`` from the words of a state block (``ring``: its floats as Python floats)"""
    n = min(count, window)
    start = count % window if count > window else 0
    values = [ring[(start + i) % window] for i in range(n)]      # the deque, oldest first
    return SimpleNamespace(count=count, total=total, global_avg=total / count if count else float("nan"), bad=bad, bad_iter=bad_iter,
                           **_window_stats(values))


class _HostLossWindow:
    """the window of the reference form of the loop: Python floats on the host, read through ``_window_stats``"""

    def __init__(self, window_size=10):
        self.deque = deque(maxlen=window_size)

    def update(self, value):
        self.deque.append(value)

    @property
    def avg(self):
        return _window_stats(list(self.deque))["avg"]


def _stop_on_bad_loss():
    """engine.py:100-102"""
    logging.info("Loss in not finite. Training will be stopped.")
    sys.exit(1)


def _check_sync_free(args, optimizer, reducer):
    """what the ClipAdamW form of ``train_one_epoch`` cannot honour is refused before the first batch"""
    want = float(args.clip_gradient) if args.clip_gradient and args.clip_gradient > 0 else None
    have = float(optimizer.max_norm) if optimizer.max_norm else None
    if want != have:
        raise ValueError(f"train_one_epoch: args.clip_gradient {args.clip_gradient} but the optimizer clips at max_norm "
                         f"{optimizer.max_norm}: with ClipAdamW the clipping is the optimizer's own (optim.build_optimizer)")
    if reducer is not None:
        if reducer.bucket_views:
            raise ValueError("train_one_epoch: a hooked GradientReducer (bucket_views=True) reduces inside backward; this loop "
                             "packs after the flush: build the reducer with bucket_views=False, flat=optimizer.flat")
        if reducer.flat is not optimizer.flat:
            raise ValueError("train_one_epoch: the reducer must pack into the optimizer's flat buffer (flat=optimizer.flat)")


def train_one_epoch(args, curr_epoch, model, optimizer, criterion, dataset_config, dataset_loader, reducer=None):
    """engine.py:59-122, same positional arguments -> ``(None, curr_iter, curr_lr, loss_avg.avg, loss_dict_reduced)``.

    Common to both forms, as the reference has them: the iteration count, ``model.train()``, a barrier before the loop and after
    every iteration, ``adjust_learning_rate`` before every iteration, the batch to the model's device, the three input keys, the
    criterion, the loss averaged over the ranks (a detached copy: the loss that is back-propagated is the rank's own), the log line
    on the primary rank every ``args.log_every`` iterations.  ``args.use_superpoint`` is refused.

    Any ``torch.optim.Optimizer``: the reference's loop, with its reads of the loss every iteration, ``sys.exit(1)`` on a
    non-finite one, ``clip_grad_norm_`` under ``args.clip_gradient`` and ``optimizer.step()``.  Works on CPU tensors.

    ``optim.ClipAdamW``: no read per iteration.  Zero the gradients (``reducer.zero_grad()`` or ``p.grad = None``), forward, loss,
    ``LossMeter.update``, backward, ``runtime.flush_weight_grads()`` under ``runtime.defer_weight_grads``, the pack
    (``reducer.pack_and_reduce()`` for a non-hooked reducer, else ``optimizer.flat.pack_grads()``), ``optimizer.step(skip=flag)``.
    Clipping is the optimizer's ``max_norm`` and must agree with ``args.clip_gradient``.  Every rank reads the meter where the
    reference prints (``curr_iter % args.log_every == 0``) and once after the loop; a raised flag at a read logs the reference's
    message and calls ``sys.exit(1)`` (the reduced loss is the same on every rank, so all ranks leave together).  On that exit the
    parameters, the moments and the step count are those before the bad iteration, which is what the reference guarantees: the
    flag has switched every later optimizer launch off on the device.  BatchNorm running statistics, dropout streams and the
    loader have moved on by fewer than ``log_every`` iterations (the reference has likewise run the bad iteration's forward)."""
    if getattr(args, "use_superpoint", False):
        raise NotImplementedError("train_one_epoch: args.use_superpoint is not built (README: superpoints are out of scope)")
    sync_free = isinstance(optimizer, ClipAdamW)
    if sync_free:
        _check_sync_free(args, optimizer, reducer)
    elif reducer is not None:
        raise ValueError("train_one_epoch: `reducer` belongs to the ClipAdamW form; the reference form steps the optimizer it is given")
    ap_calculator = None

    curr_iter = curr_epoch * len(dataset_loader)
    max_iters = args.max_epoch * len(dataset_loader)
    net_device = next(model.parameters()).device
    many_ranks = torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1

    loss_avg = LossMeter(window_size=10, device=net_device) if sync_free else _HostLossWindow(window_size=10)
    if sync_free:
        from . import runtime

    model.train()
    barrier()

    for batch_idx, batch_data_label in enumerate(dataset_loader):
        curr_time = time.time()
        curr_lr = adjust_learning_rate(args, optimizer, curr_iter / max_iters)
        batch_data_label = batch_dict_to_cuda(batch_data_label, local_rank=net_device)

        # Forward pass
        if not sync_free:
            optimizer.zero_grad()
        elif reducer is not None:
            reducer.zero_grad()
        else:
            for p in optimizer.flat.params:
                p.grad = None
        inputs = {"point_clouds": batch_data_label["point_clouds"],
                  "point_cloud_dims_min": batch_data_label["point_cloud_dims_min"],
                  "point_cloud_dims_max": batch_data_label["point_cloud_dims_max"]}
        outputs = model(inputs)
        # Compute loss
        loss, loss_dict = criterion(outputs, batch_data_label)

        # (the reference sums `loss` itself in place, which does not reach its gradients; all_reduce_average here divides in place too)
        loss_reduced = all_reduce_average(loss.detach().clone() if many_ranks else loss.detach())
        loss_dict_reduced = reduce_dict(loss_dict)

        if sync_free:
            loss_avg.update(loss_reduced, curr_iter)
            loss.backward()
            if runtime.weight_grads_deferred():
                runtime.flush_weight_grads()
            if reducer is not None:
                reducer.pack_and_reduce()
            else:
                optimizer.flat.pack_grads()
            optimizer.step(skip=loss_avg.bad_flag)
            seen = loss_avg.read() if curr_iter % args.log_every == 0 else None   # every rank, where the reference prints
            if seen is not None and seen.bad:
                _stop_on_bad_loss()
        else:
            if not math.isfinite(loss_reduced.item()):
                _stop_on_bad_loss()
            loss.backward()
            if args.clip_gradient > 0:
                torch.nn.utils.clip_grad_norm_(model.parameters(), args.clip_gradient)
            optimizer.step()
            loss_avg.update(loss_reduced.item())
            seen = loss_avg

        # logging
        if is_primary() and curr_iter % args.log_every == 0:
            eta_seconds = (max_iters - curr_iter) * (time.time() - curr_time)
            eta_str = str(datetime.timedelta(seconds=int(eta_seconds)))
            print(f"Epoch [{curr_epoch}/{args.max_epoch}]; Iter [{curr_iter}/{max_iters}]; Loss {seen.avg:0.2f}; LR {curr_lr:0.2e}; ETA {eta_str}")

        curr_iter += 1
        barrier()

    if sync_free:
        seen = loss_avg.read()   # the read behind the return value
        if seen.bad:
            _stop_on_bad_loss()
        return ap_calculator, curr_iter, curr_lr, seen.avg, loss_dict_reduced
    return ap_calculator, curr_iter, curr_lr, loss_avg.avg, loss_dict_reduced


@torch.no_grad()
def evaluate(args, curr_epoch, model, criterion, dataset_config, dataset_loader, curr_train_iter):
    """engine.py:125-193, same arguments -> (ap_calculator, loss_avg, loss_dict_reduced).  ``loss_avg`` is the mean of the last
    ten reduced losses (0.0 without a criterion); ``loss_dict_reduced`` is the last batch's, None without a criterion.  The
    calculator is resident: measured per batch, its ``step_meter`` costs the host 0.14 ms against the host path's 1.88 ms
    (profiles/eval_resident_bench.txt)."""
    ap_calculator = APCalculator(dataset_config=dataset_config, ap_iou_thresh=[0.25, 0.5], class2type_map=dataset_config.class2type,
                                 no_nms=args.test_no_nms, args=args, resident=True)
    curr_iter = 0
    net_device = next(model.parameters()).device
    num_batches = len(dataset_loader)
    last_losses = deque(maxlen=10)     # SmoothedValue(window_size=10), as device scalars
    loss_dict_reduced = None
    model.eval()
    barrier()
    epoch_str = f"[{curr_epoch}/{args.max_epoch}]" if curr_epoch > 0 else ""

    for batch_idx, batch_data_label in enumerate(dataset_loader):
        batch_data_label = batch_dict_to_cuda(batch_data_label, local_rank=net_device)
        inputs = {"point_clouds": batch_data_label["point_clouds"],
                  "point_cloud_dims_min": batch_data_label["point_cloud_dims_min"],
                  "point_cloud_dims_max": batch_data_label["point_cloud_dims_max"]}
        outputs = model(inputs)

        if criterion is not None:
            loss, loss_dict = criterion(outputs, batch_data_label)
            loss_reduced = all_reduce_average(loss)
            loss_dict_reduced = reduce_dict(loss_dict)
            last_losses.append(loss_reduced.detach())
        else:
            loss_dict_reduced = None

        if args.cls_loss.split("_")[0] == "focalloss":
            outputs["outputs"]["sem_cls_prob"] = outputs["outputs"]["sem_cls_prob"].sigmoid()

        outputs["outputs"] = all_gather_dict(outputs["outputs"])
        batch_data_label = all_gather_dict(batch_data_label)
        if args.axis_align_test:
            outputs["outputs"]["box_corners"] = outputs["outputs"]["box_corners_axis_align"]

        ap_calculator.step_meter(outputs, batch_data_label)
        if is_primary() and curr_iter % args.log_every == 0:
            print(f"Evaluate {epoch_str}; Batch [{curr_iter}/{num_batches}]")
        curr_iter += 1
        barrier()

    # the one read of the losses: the float32 mean of the window, on the host as SmoothedValue.avg takes it
    loss_avg = torch.stack(list(last_losses)).to(torch.float32).cpu().mean().item() if last_losses else 0.0
    return ap_calculator, loss_avg, loss_dict_reduced


def test_model(args, model, model_no_ddp, criterion, dataset_config, dataloaders):
    """main.py:437-480, same arguments: the ``--test_only`` entry.  Loads ``args.test_ckpt`` (the layout of utils/io.py:23-29:
    model, optimizer, epoch, args, best_val_metrics) into ``model_no_ddp``, runs ``evaluate`` on ``dataloaders["test"]`` without
    a criterion and prints the metrics, and with ``args.test_size`` those of the S, M and L volume classes, which come from one
    device pass (``APCalculator.compute_metrics_by_size``).  -> {"": metrics, "S": ..., "M": ..., "L": ...} as
    printed (the reference returns None)."""
    if args.test_ckpt is None or not os.path.isfile(args.test_ckpt):
        print(f"Please specify a test checkpoint using --test_ckpt. Found invalid value {args.test_ckpt}")
        sys.exit(1)
    # the reference's checkpoints carry an argparse.Namespace and the numpy scalars of best_val_metrics: a full unpickle, as
    # the reference does it; a checkpoint is trusted like the code that reads it
    sd = torch.load(args.test_ckpt, map_location=torch.device("cpu"), weights_only=False)
    model_no_ddp.load_state_dict(sd["model"], strict=False)
    ap_calculator, _, _ = evaluate(args, -1, model, None, dataset_config, dataloaders["test"], 0)   # no loss, for speed
    ret = {"": ap_calculator.compute_metrics()}
    if getattr(args, "test_size", False):
        ret.update(ap_calculator.compute_metrics_by_size())
    for size, metrics in ret.items():
        if is_primary():
            print("==" * 10)
            print(f"Test model{' ' + size if size else ''}; Metrics {ap_calculator.metrics_to_str(metrics)}")
            print("==" * 10)
    return ret
