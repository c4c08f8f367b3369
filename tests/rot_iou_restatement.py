"""TEST INFRASTRUCTURE ONLY: torch fp64 CPU restatement of the rotated 3-D IoU / DIoU that the reference's criterion.py
uses with ``--iou_type diou / iou`` (criterion.py:25-64 diff_diou_rotated_3d, 620-633), differentiable by autograd.

The reference takes three functions from mmcv-full 1.6.1 (mmcv/ops/diff_iou_rotated.py), which is not in this image.
They are restated here from their published semantics, so they are PARITY-UNPINNED (as points_in_boxes_all is in
oracle/criterion_oracle.py):
  * box2corners(box (..., 5) = x, y, w, h, alpha) -> (..., 4, 2): local corners (+-w/2, +-h/2) in the order (+,+), (-,+),
    (-,-), (+,-), multiplied by [[cos, sin], [-sin, cos]] (row vectors) and moved to (x, y);
  * oriented_box_intersection_2d(c1, c2) -> (area, vertices): the exact area of the intersection of two convex
    quadrilaterals.  mmcv collects the corners of each box inside the other and the edge crossings, orders them by angle
    around their mean and takes the shoelace area; the same construction is used here (mmcv's own tolerances at
    degenerate configurations are not reproduced);
  * diff_iou_rotated_3d(b1, b2) for boxes (x, y, z, w, h, l, alpha): footprint intersection x height overlap over the
    union of the volumes, no epsilon.
The reference's own diff_diou_rotated_3d (criterion.py:25-64) subtracts r2 / c2 with r2 summed over (x, y, w) -- its
box1[..., :3] is taken from the (x, y, w, h, alpha) slice -- and c2 the squared diagonal of the enclosing box of both
boxes' rotated footprint corners and z extents; restated in `rotated_iou_3d(..., diou=True)`.

`pair_terms_for(iou_type)` returns a drop-in for oracle.criterion_oracle.pair_terms: tests monkeypatch it over the
oracle's, and the oracle's cost, assignment and losses then run unchanged in that mode.
"""
import torch

_LX = (0.5, -0.5, -0.5, 0.5)
_LY = (0.5, 0.5, -0.5, -0.5)


def box2corners(box):
    """(..., 5) = (x, y, w, h, alpha) -> (..., 4, 2) footprint corners (see the module header)."""
    x, y, w, h, a = box.unbind(-1)
    lx = box.new_tensor(_LX) * w[..., None]
    ly = box.new_tensor(_LY) * h[..., None]
    s, c = torch.sin(a)[..., None], torch.cos(a)[..., None]
    return torch.stack((lx * c - ly * s + x[..., None], lx * s + ly * c + y[..., None]), -1)


def _cross(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def _inside(pts, quad, eps):
    """pts (..., K, 2) inside the counter-clockwise quad (..., 4, 2), boundary included (to eps)"""
    ok = torch.ones(pts.shape[:-1], dtype=torch.bool)
    for k in range(4):
        p, q = quad[..., k, None, :], quad[..., (k + 1) % 4, None, :]
        ok = ok & (_cross(q - p, pts - p) >= -eps)
    return ok


def intersection_area(c1, c2):
    """Exact area of the intersection of two convex counter-clockwise quadrilaterals c1, c2 (..., 4, 2) -> (...,)."""
    scale = (c1.detach().abs().amax((-1, -2)) + c2.detach().abs().amax((-1, -2)) + 1.0)[..., None]
    eps = 1e-12 * scale * scale
    verts = [c1, c2]
    valid = [_inside(c1, c2, eps), _inside(c2, c1, eps)]
    # crossings of edge i of c1 with edge j of c2
    p, d1 = c1, torch.roll(c1, -1, -2) - c1                        # (..., 4, 2)
    q, d2 = c2, torch.roll(c2, -1, -2) - c2
    p, d1 = p[..., :, None, :], d1[..., :, None, :]                # (..., 4, 1, 2)
    q, d2 = q[..., None, :, :], d2[..., None, :, :]                # (..., 1, 4, 2)
    den = _cross(d1, d2)
    ok = den.abs() > 1e-14 * (d1.detach().norm(dim=-1) * d2.detach().norm(dim=-1))
    safe = torch.where(ok, den, torch.ones_like(den))
    t = _cross(q - p, d2) / safe
    u = _cross(q - p, d1) / safe
    tol = 1e-12
    ok = ok & (t >= -tol) & (t <= 1 + tol) & (u >= -tol) & (u <= 1 + tol)
    x = p + t[..., None] * d1
    shp = x.shape[:-3]
    verts.append(x.reshape(shp + (16, 2)))
    valid.append(ok.reshape(shp + (16,)))
    v = torch.cat(verts, -2)                                       # (..., 24, 2)
    m = torch.cat(valid, -1)                                       # (..., 24)
    mf = m.to(v.dtype)[..., None]
    n = mf.sum(-2).clamp(min=1)
    mean = (v.detach() * mf).sum(-2) / n                           # (..., 2)
    rel = v.detach() - mean[..., None, :]
    ang = torch.atan2(rel[..., 1], rel[..., 0])
    ang = torch.where(m, ang, torch.full_like(ang, 10.0))          # invalid ones last
    order = torch.argsort(ang, -1)
    vs = torch.gather(v, -2, order[..., None].expand(v.shape))
    ms = torch.gather(m, -1, order)
    vs = torch.where(ms[..., None], vs, vs[..., :1, :])            # invalid -> copies of the first vertex (no area)
    return 0.5 * _cross(vs, torch.roll(vs, -1, -2)).sum(-1).abs()


def rotated_iou_3d(b1, b2, diou=False):
    """b1, b2 (..., 7) = (x, y, z, w, h, l, alpha) -> IoU (diou=False: mmcv diff_iou_rotated_3d) or the reference's DIoU."""
    f1, f2 = b1[..., [0, 1, 3, 4, 6]], b2[..., [0, 1, 3, 4, 6]]
    k1, k2 = box2corners(f1), box2corners(f2)
    area = intersection_area(k1, k2)
    top1, bot1 = b1[..., 2] + b1[..., 5] * 0.5, b1[..., 2] - b1[..., 5] * 0.5
    top2, bot2 = b2[..., 2] + b2[..., 5] * 0.5, b2[..., 2] - b2[..., 5] * 0.5
    zo = (torch.minimum(top1, top2) - torch.maximum(bot1, bot2)).clamp(min=0.0)
    inter = area * zo
    union = b1[..., 3] * b1[..., 4] * b1[..., 5] + b2[..., 3] * b2[..., 4] * b2[..., 5] - inter
    iou = inter / union
    if not diou:
        return iou
    # enclosing box: torch.max / min over the 4 corners (first extreme takes the gradient), elementwise max / min between
    # the boxes (a tie splits it)
    hi_x = torch.maximum(k1[..., 0].max(-1)[0], k2[..., 0].max(-1)[0])
    lo_x = torch.minimum(k1[..., 0].min(-1)[0], k2[..., 0].min(-1)[0])
    hi_y = torch.maximum(k1[..., 1].max(-1)[0], k2[..., 1].max(-1)[0])
    lo_y = torch.minimum(k1[..., 1].min(-1)[0], k2[..., 1].min(-1)[0])
    hi_z, lo_z = torch.maximum(top1, top2), torch.minimum(bot1, bot2)
    c2 = (lo_x - hi_x) ** 2 + (lo_y - hi_y) ** 2 + (lo_z - hi_z) ** 2
    r2 = ((f1[..., :3] - f2[..., :3]) ** 2).sum(-1)                # (x, y, w): the reference's slice
    return iou - r2 / c2


class _PairwiseIoU(torch.autograd.Function):
    """pred (B, P, 7) x gt (B, G, 7) -> (B, P, G) in fp64 without holding the whole pairwise graph: the forward runs in
    chunks without autograd, the backward re-runs autograd only on the pairs that receive a gradient (the matched ones,
    when the result is gathered by an assignment)."""

    CHUNK = 1 << 16

    @staticmethod
    def forward(ctx, pred, gt, diou):
        B, P, G = pred.shape[0], pred.shape[1], gt.shape[1]
        a = pred[:, :, None, :].expand(B, P, G, 7).reshape(-1, 7)
        b = gt[:, None, :, :].expand(B, P, G, 7).reshape(-1, 7)
        out = torch.cat([rotated_iou_3d(a[s:s + _PairwiseIoU.CHUNK], b[s:s + _PairwiseIoU.CHUNK], diou)
                         for s in range(0, a.shape[0], _PairwiseIoU.CHUNK)]) if a.shape[0] else a.new_zeros(0)
        ctx.save_for_backward(pred, gt)
        ctx.diou = diou
        return out.reshape(B, P, G)

    @staticmethod
    def backward(ctx, grad):
        pred, gt = ctx.saved_tensors
        B, P, G = grad.shape
        nz = grad.nonzero(as_tuple=True)
        d = torch.zeros_like(pred)
        if nz[0].numel():
            with torch.enable_grad():
                p = pred[nz[0], nz[1]].detach().requires_grad_(True)
                q = rotated_iou_3d(p, gt[nz[0], nz[2]].detach(), ctx.diou)
                (gp,) = torch.autograd.grad(q, p, grad[nz])
            d.index_put_((nz[0], nz[1]), gp, accumulate=True)
        return d, None, None


def pairwise(pred, gt, diou):
    """(B, P, 7) x (B, G, 7) -> (B, P, G) rotated IoU / DIoU in fp64 (differentiable w.r.t. pred)."""
    return _PairwiseIoU.apply(pred.double(), gt.double(), diou)


def pair_terms_for(iou_type):
    """Drop-in for oracle.criterion_oracle.pair_terms with iou_type "diou" / "iou" (criterion.py:620-637): the masked
    pairwise DIoU / IoU of (center_unnormalized, size_unnormalized, angle_continuous) against the ground truth, and the
    centre / size L1 matrices as the oracle computes them."""
    assert iou_type in ("diou", "iou")

    def pair_terms(o, t):
        pred = torch.cat((o["center_unnormalized"], o["size_unnormalized"], o["angle_continuous"][..., None]), -1)
        gt = torch.cat((t["gt_box_centers"], t["gt_box_sizes"], t["gt_box_angles"][..., None]), -1)
        q = pairwise(pred, gt, iou_type == "diou").to(pred.dtype)
        G = gt.shape[1]
        mask = (torch.arange(G)[None, None, :] < t["nactual_gt"][:, None, None]).to(q.dtype)
        q = q * mask
        pc, ps = o["pre_box_center_unnormalized"][:, :, None], o["pre_box_size_unnormalized"][:, :, None]
        want_c = (t["gt_box_centers"][:, None] - pc) / (ps + 1e-5)
        center = (o["center_reg"][:, :, None] - want_c).abs().sum(-1)
        want_s = torch.log((t["gt_box_sizes"][:, None] + 1e-5) / (ps + 1e-5))
        size = (o["size_reg"][:, :, None] - want_s).abs().sum(-1)
        return q, center, size

    return pair_terms
