"""What tools/make_train_epoch_golden.py records and the train_one_epoch tests read back (tests/golden/train_epoch.npz): the
settings engine.py:59-122 reads, the small model of optim_sched_cases.py behind the loop's inputs dict, an MSE stub criterion, and
the loader rebuilt from the recorded batches.  The model and the criterion are this project's own: the fixture holds numbers only."""
from argparse import Namespace

import torch

from optim_sched_cases import SCHEDULES, small_model

EPOCHS, BATCHES, BATCH_SIZE = 2, 5, 4
BAD_ITER = 3                      # the iteration whose target holds an inf in the second recorded run
WEIGHT_DECAY = 0.1
INPUT_KEYS = ["point_cloud_dims_max", "point_cloud_dims_min", "point_clouds"]


def settings(**over):
    """the cosine_warm schedule of optim_sched_cases.py (20 epochs: ten iterations of its warm-up) behind clip_gradient 0.1"""
    a = dict(SCHEDULES["cosine_warm"][0], clip_gradient=0.1, log_every=2, use_superpoint=False)
    a.update(over)
    return Namespace(**a)


class DictModel(torch.nn.Module):
    """``small_model()`` fed from ``inputs["point_clouds"]`` [B, 7]; refuses any other set of keys than the loop's three"""

    def __init__(self):
        super().__init__()
        self.net = small_model()

    def forward(self, inputs):
        assert sorted(inputs) == INPUT_KEYS, sorted(inputs)
        assert self.training
        return self.net(inputs["point_clouds"])


def mse_criterion(outputs, batch):
    loss = ((outputs - batch["target"]) ** 2).mean()
    return loss, {"loss_mse": loss.detach()}


def make_batches(seed=11):
    """(x [EPOCHS * BATCHES, B, 7], target [EPOCHS * BATCHES, B, 5]): what the tool records"""
    g = torch.Generator().manual_seed(seed)
    n = EPOCHS * BATCHES
    return torch.randn((n, BATCH_SIZE, 7), generator=g), torch.randn((n, BATCH_SIZE, 5), generator=g) * 2.0


def loader(x, target, epoch, bad_iter=None):
    """the epoch's batches as fresh dicts of CPU tensors (the loop moves them); ``bad_iter``: that batch's first target is +inf"""
    out = []
    for i in range(epoch * BATCHES, (epoch + 1) * BATCHES):
        t = torch.as_tensor(target[i]).clone()
        if bad_iter is not None and i == bad_iter:
            t[0, 0] = float("inf")
        xi = torch.as_tensor(x[i]).clone()
        out.append({"point_clouds": xi, "point_cloud_dims_min": xi.amin(0, keepdim=True), "point_cloud_dims_max": xi.amax(0, keepdim=True),
                    "target": t})
    return out


def load_params(model, arrays):
    """the recorded initial parameters (``param:<name>``) into ``model``"""
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.as_tensor(arrays[f"param:{name}"]))
    return model


def cut_eta(text):
    """printed lines without their last field (the ETA depends on the clock)"""
    return [line.split("; ETA ")[0] for line in text.splitlines()]


def real_scenes(ds):
    """the two synthetic batches of tests/test_gpu_engine_evaluate.py (B = 2 and B = 1: two walls of a room, six box slots of which
    four are present), with the box parameters the criterion reads beside the corners"""
    g = torch.Generator().manual_seed(3)
    loader = []
    for B in (2, 1):
        uu = torch.rand(B, 5000, 2, generator=g)
        cloud = torch.cat((torch.stack((uu[:, :2500, 0] * 4, uu[:, :2500, 1] * 3, torch.zeros(B, 2500)), -1),
                           torch.stack((uu[:, 2500:, 0] * 4, torch.zeros(B, 2500), uu[:, 2500:, 1] * 2.5), -1)), 1) + 1.0
        present = torch.zeros(B, 6)
        present[:, :4] = 1
        centers = (torch.rand(B, 6, 3, generator=g) * torch.tensor([4.0, 3.0, 2.5]) + 1) * present[..., None]
        sizes = (0.4 + torch.rand(B, 6, 3, generator=g)) * present[..., None]
        loader.append({"point_clouds": cloud, "point_cloud_dims_min": cloud.amin(1), "point_cloud_dims_max": cloud.amax(1),
                       "gt_box_corners": ds.box_parametrization_to_corners(centers, sizes, torch.zeros(B, 6)) * present[..., None, None],
                       "gt_box_centers": centers, "gt_box_sizes": sizes, "gt_box_angles": torch.zeros(B, 6),
                       "gt_box_sem_cls_label": torch.randint(0, ds.num_semcls, (B, 6), generator=g) * present.long(),
                       "gt_box_present": present, "gt_angle_class_label": torch.zeros(B, 6, dtype=torch.int64),
                       "gt_angle_residual_label": torch.zeros(B, 6)})
    return loader
