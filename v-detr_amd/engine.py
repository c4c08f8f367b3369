"""The evaluation half of the reference's control plane (engine.py:24-56, 125-193): ``evaluate`` — what ``--test_only`` runs on a
checkpoint — and the learning-rate helpers.  ``train_one_epoch`` is NOT built here.

``evaluate`` is the reference's loop, statement for statement: batch to the model's device, ``model(inputs)`` on the three input
keys, the loss when a criterion is given, ``sigmoid`` for the focal-loss heads, ``all_gather_dict`` on outputs and batch, the
axis-aligned corners under ``--axis_align_test``, ``APCalculator.step_meter``, the progress line.  What differs is where the host
waits.  The reference reads the loss every batch (``loss_reduced.item()``) and ``step_meter`` copies seven tensors to the host; here
the last ten reduced losses stay device scalars until the loop has ended (``SmoothedValue(window_size=10).avg`` is their float32
mean) and the calculator is resident (``APCalculator(resident=True)``), so a batch's loop body reads nothing back
and the host can enqueue batch i+1 while the device finishes batch i.
"""
from collections import deque

import torch

from .ap_calculator import APCalculator
from .dist import all_gather_dict, all_reduce_average, barrier, batch_dict_to_cuda, is_primary, reduce_dict
from .optim import compute_learning_rate, lr_table  # noqa: F401  (engine.py:24-49; the table form ClipAdamW indexes)


def adjust_learning_rate(args, optimizer, curr_epoch):
    """engine.py:52-56"""
    curr_lr = compute_learning_rate(args, curr_epoch)
    for param_group in optimizer.param_groups:
        param_group["lr"] = curr_lr
    return curr_lr


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
