"""CPU tests (no GPU) of the fp64 rotated IoU / DIoU restatement (tests/rot_iou_restatement.py) that the diou / iou
criterion tests and tools/make_diou_golden.py stand on: area against a dense-grid count, closed forms, invariances and
autograd gradients against central differences."""
import math

import numpy as np
import torch

import rot_iou_restatement as R


def random_boxes(g, n, spread=1.0):
    c = (torch.rand((n, 3), generator=g, dtype=torch.float64) - 0.5) * 2 * spread + 5.0
    s = 0.2 + torch.rand((n, 3), generator=g, dtype=torch.float64) * 2.0
    a = (torch.rand((n, 1), generator=g, dtype=torch.float64) - 0.5) * 2 * math.pi
    return torch.cat((c, s, a), -1)


def grid_area(c1, c2, n=1000):
    """intersection area of two quads (4, 2) by counting the centres of an n x n grid over their common bounding box"""
    lo = torch.maximum(c1.min(0)[0], c2.min(0)[0])
    hi = torch.minimum(c1.max(0)[0], c2.max(0)[0])
    if (hi <= lo).any():
        return 0.0
    u = (torch.arange(n, dtype=torch.float64) + 0.5) / n
    xs, ys = lo[0] + u * (hi[0] - lo[0]), lo[1] + u * (hi[1] - lo[1])
    pts = torch.stack(torch.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)
    inside = R._inside(pts, c1, 0.0) & R._inside(pts, c2, 0.0)
    return float(inside.double().mean() * (hi - lo).prod())


def test_area_matches_a_dense_grid():
    g = torch.Generator().manual_seed(0)
    b1, b2 = random_boxes(g, 200, 0.8), random_boxes(g, 200, 0.8)
    k1, k2 = R.box2corners(b1[:, [0, 1, 3, 4, 6]]), R.box2corners(b2[:, [0, 1, 3, 4, 6]])
    got = R.intersection_area(k1, k2)
    want = torch.tensor([grid_area(k1[i], k2[i]) for i in range(200)], dtype=torch.float64)
    assert (want > 0).sum() > 100, "most pairs overlap"
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=1e-3 * float(want.max()) + 2e-3)


def test_axis_aligned_closed_form():
    g = torch.Generator().manual_seed(1)
    b1, b2 = random_boxes(g, 300), random_boxes(g, 300)
    b1[:, 6] = 0
    b2[:, 6] = 0
    ov = []
    for a in range(3):
        lo = torch.maximum(b1[:, a] - b1[:, 3 + a] / 2, b2[:, a] - b2[:, 3 + a] / 2)
        hi = torch.minimum(b1[:, a] + b1[:, 3 + a] / 2, b2[:, a] + b2[:, 3 + a] / 2)
        ov.append((hi - lo).clamp(min=0))
    inter = ov[0] * ov[1] * ov[2]
    union = b1[:, 3:6].prod(-1) + b2[:, 3:6].prod(-1) - inter
    np.testing.assert_allclose(R.rotated_iou_3d(b1, b2).numpy(), (inter / union).numpy(), rtol=1e-12, atol=1e-12)
    # DIoU of axis-aligned boxes: the enclosing box is the union of the extents; r2 over (x, y, w)
    ext = []
    for a in range(3):
        lo = torch.minimum(b1[:, a] - b1[:, 3 + a] / 2, b2[:, a] - b2[:, 3 + a] / 2)
        hi = torch.maximum(b1[:, a] + b1[:, 3 + a] / 2, b2[:, a] + b2[:, 3 + a] / 2)
        ext.append(hi - lo)
    c2 = ext[0] ** 2 + ext[1] ** 2 + ext[2] ** 2
    r2 = (b1[:, 0] - b2[:, 0]) ** 2 + (b1[:, 1] - b2[:, 1]) ** 2 + (b1[:, 3] - b2[:, 3]) ** 2
    np.testing.assert_allclose(R.rotated_iou_3d(b1, b2, diou=True).numpy(), (inter / union - r2 / c2).numpy(),
                               rtol=1e-12, atol=1e-12)


def test_identity_symmetry_and_rotation_invariance():
    g = torch.Generator().manual_seed(2)
    b1, b2 = random_boxes(g, 300, 0.7), random_boxes(g, 300, 0.7)
    np.testing.assert_allclose(R.rotated_iou_3d(b1, b1).numpy(), 1.0, atol=1e-12)
    np.testing.assert_allclose(R.rotated_iou_3d(b1, b1, diou=True).numpy(), 1.0, atol=1e-12)
    np.testing.assert_allclose(R.rotated_iou_3d(b1, b2).numpy(), R.rotated_iou_3d(b2, b1).numpy(), atol=1e-12)
    # turn both boxes and their centres about the z axis: the IoU does not change
    th = 0.7
    c, s = math.cos(th), math.sin(th)

    def turn(b):
        out = b.clone()
        out[:, 0] = c * b[:, 0] - s * b[:, 1]
        out[:, 1] = s * b[:, 0] + c * b[:, 1]
        out[:, 6] = b[:, 6] + th
        return out

    np.testing.assert_allclose(R.rotated_iou_3d(turn(b1), turn(b2)).numpy(), R.rotated_iou_3d(b1, b2).numpy(), atol=1e-10)


def test_diou_penalises_width_at_a_shared_centre():
    """The reference's r2 sums over (x, y, w) (criterion.py:33-34, 60): same centre, different w -> a non-zero penalty."""
    b1 = torch.tensor([[5.0, 4.0, 1.0, 2.0, 1.0, 1.0, 0.3]], dtype=torch.float64)
    b2 = b1.clone()
    b2[0, 3] = 1.5
    iou, diou = R.rotated_iou_3d(b1, b2), R.rotated_iou_3d(b1, b2, diou=True)
    assert float(iou - diou) > 1e-3
    assert abs(float(R.rotated_iou_3d(b1, b1, diou=True)) - 1.0) < 1e-12


def test_gradients_match_central_differences():
    g = torch.Generator().manual_seed(3)
    b1, b2 = random_boxes(g, 40, 0.6), random_boxes(g, 40, 0.6)
    for diou in (False, True):
        x = b1.clone().requires_grad_(True)
        q = R.rotated_iou_3d(x, b2, diou)
        (gr,) = torch.autograd.grad(q.sum(), x)
        h = 1e-6
        num = torch.zeros_like(b1)
        for k in range(7):
            e = torch.zeros_like(b1)
            e[:, k] = h
            num[:, k] = (R.rotated_iou_3d(b1 + e, b2, diou) - R.rotated_iou_3d(b1 - e, b2, diou)) / (2 * h)
        np.testing.assert_allclose(gr.numpy(), num.numpy(), rtol=1e-5, atol=1e-7)


def test_pairwise_backward_only_where_the_gradient_lands():
    g = torch.Generator().manual_seed(4)
    p, t = random_boxes(g, 12, 0.5).reshape(2, 6, 7), random_boxes(g, 8, 0.5).reshape(2, 4, 7)
    x = p.clone().requires_grad_(True)
    q = R.pairwise(x, t, True)
    w = torch.zeros_like(q)
    w[0, 1, 2], w[1, 5, 0], w[1, 5, 3] = 1.0, 2.0, -1.0
    (q * w).sum().backward()
    y = p.clone().requires_grad_(True)
    full = R.rotated_iou_3d(y[:, :, None].expand(2, 6, 4, 7), t[:, None].expand(2, 6, 4, 7), True)
    (full * w).sum().backward()
    np.testing.assert_allclose(q.detach().numpy(), full.detach().numpy(), atol=1e-14)
    np.testing.assert_allclose(x.grad.numpy(), y.grad.numpy(), atol=1e-14)
