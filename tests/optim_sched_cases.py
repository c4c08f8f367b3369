"""What tools/make_lr_schedule_golden.py records and tests/test_optim_sched.py / test_gpu_optim_sched.py read back: the schedule
settings (the fields engine.py:24-49 reads) and the small model whose parameter names optimizer.py:4-26 sorts into its two groups."""
import torch

# name -> (settings, iterations per epoch).  "defaults": main.py:34-43,177-178 as they stand.
SCHEDULES = {
    "cosine_warm": (dict(base_lr=7e-4, warm_lr=1e-6, warm_lr_epochs=9, final_lr=1e-6, lr_scheduler="cosine", max_epoch=20, step_epoch=""), 7),
    "cosine_nowarm": (dict(base_lr=7e-4, warm_lr=1e-6, warm_lr_epochs=0, final_lr=1e-6, lr_scheduler="cosine", max_epoch=20, step_epoch=""), 7),
    "step": (dict(base_lr=7e-4, warm_lr=1e-6, warm_lr_epochs=9, final_lr=1e-6, lr_scheduler="step", max_epoch=20, step_epoch="12_16"), 7),
    "defaults": (None, 5),
}


class Scaled(torch.nn.Module):
    """a 2-D parameter under a name that ends in ``bias`` (exempt by name, not by shape)"""

    def __init__(self, rows, cols):
        super().__init__()
        self.table_bias = torch.nn.Parameter(torch.zeros(rows, cols))

    def forward(self, x):
        return x + self.table_bias.sum(0)


def small_model():
    """Linear with bias, LayerNorm, a bias-free Linear, and the 2-D ``*bias``: every branch of optimizer.py:11"""
    return torch.nn.Sequential(torch.nn.Linear(7, 9), torch.nn.LayerNorm(9), Scaled(3, 9), torch.nn.Linear(9, 5, bias=False))
