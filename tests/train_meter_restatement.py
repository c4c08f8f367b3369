"""The loss meter of csrc/train_meter.hip restated in numpy, word for word of its state block, and the fields the host derives from
the block (engine.LossMeter.read).  Independent of the library: tests hold it to the reference's recorded ``SmoothedValue``
(tests/golden/train_meter.npz) and then hold the kernel to it where the fixture has no case (other windows, non-finite losses)."""
import numpy as np
import torch

MAX_WINDOW = 64


class Meter:
    def __init__(self, window):
        self.total = np.float64(0.0)
        self.count = 0
        self.bad_iter = -1
        self.bad = 0
        self.window = int(window)
        self.ring = np.zeros(MAX_WINDOW, np.float32)

    def update(self, loss, it):
        if self.bad != 0:
            return
        if not 1 <= self.window <= MAX_WINDOW:
            self.bad = 2
            return
        x = np.float32(loss)
        if not np.isfinite(x):
            self.bad, self.bad_iter = 1, int(it)
            return
        self.ring[self.count % self.window] = x
        self.total = self.total + np.float64(x)
        self.count += 1

    def deque(self):
        """oldest first, as Python floats"""
        n = min(self.count, self.window)
        start = self.count % self.window if self.count > self.window else 0
        return [float(self.ring[(start + i) % self.window]) for i in range(n)]

    def fields(self):
        d = self.deque()
        out = dict(count=self.count, total=float(self.total), bad=self.bad, bad_iter=self.bad_iter)
        if d:
            out.update(avg=torch.tensor(d, dtype=torch.float32).mean().item(), median=torch.tensor(d).median().item(),
                       global_avg=float(self.total) / self.count, value=d[-1], max=max(d))
        return out


FIELDS = ("avg", "median", "global_avg", "value", "max", "count", "total")
