"""GPU tests of the device criterion with ``iou_type`` "diou" / "iou" (csrc/rot_iou.h through criterion.hip's DIoU / IoU
instantiations): pairwise values, gradients, the reference fixtures, C2 shapes, the box decode's backward under this loss,
graph capture and the standalone matcher.  The yardstick is the fp64 restatement of tests/rot_iou_restatement.py (the
three mmcv functions) composed with the oracle (oracle/criterion_oracle.py) or with the reference's own criterion.py
(tests/golden/criterion_{diou,iou}_*.npz)."""
import math

import numpy as np
import pytest
import torch

import rot_iou_restatement as R
from oracle import criterion_oracle as CO
from test_oracle_criterion_rot import ROT_CASES, check_rot_against_golden, load_rot_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def crit_for(iou_type, **kw):
    from vdetr_amd.criterion import build_criterion, default_criterion_args
    return build_criterion(default_criterion_args(iou_type=iou_type, **kw), None)


def stage_from_boxes(pred, C=18, A=1, seed=0):
    """a stage dictionary around prediction boxes pred [B,P,7] (the other heads random)"""
    g = torch.Generator().manual_seed(seed)
    B, P = pred.shape[:2]
    pre_s = 0.3 + torch.rand((B, P, 3), generator=g)
    st = {"sem_cls_logits": torch.randn((B, P, C), generator=g) * 2 - 2, "objectness_prob": torch.rand((B, P), generator=g),
          "center_reg": torch.randn((B, P, 3), generator=g) * 0.3, "size_reg": torch.randn((B, P, 3), generator=g) * 0.3,
          "pre_box_center_unnormalized": pred[..., :3] + torch.randn((B, P, 3), generator=g) * 0.1,
          "pre_box_size_unnormalized": pre_s, "box_corners": torch.zeros((B, P, 8, 3)),
          "angle_logits": torch.randn((B, P, A), generator=g), "angle_residual_normalized": torch.randn((B, P, A), generator=g),
          "center_unnormalized": pred[..., :3].clone(), "size_unnormalized": pred[..., 3:6].clone(),
          "angle_continuous": pred[..., 6].clone()}
    st["sem_cls_prob"] = st["sem_cls_logits"]
    return st


def targets_from_boxes(gt, counts, C=18, seed=1):
    g = torch.Generator().manual_seed(seed)
    B, G = gt.shape[:2]
    present = torch.zeros((B, G))
    for b, n in enumerate(counts):
        present[b, :n] = 1
    return {"gt_box_corners": torch.zeros((B, G, 8, 3)), "gt_box_centers": gt[..., :3].clone(), "gt_box_sizes": gt[..., 3:6].clone(),
            "gt_box_angles": gt[..., 6].clone(), "gt_box_sem_cls_label": torch.randint(0, C, (B, G), generator=g),
            "gt_box_present": present, "gt_angle_class_label": torch.zeros((B, G), dtype=torch.int64),
            "gt_angle_residual_label": torch.zeros((B, G))}


def designed_pairs(seed=0, G=16, P=640):
    """ground truth [2,G,7] and predictions [2,P,7]: prediction p is built against box p % G in category (p // G) % 10.
    Scene 0 rotated (angles in [-pi, pi], some exactly +-pi), scene 1 axis-aligned (every angle 0)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(s, generator=g)  # noqa: E731
    gt = torch.cat((1 + r(2, G, 3) * torch.tensor([8.0, 6.0, 3.0]), 0.2 + r(2, G, 3) * 2.5, (r(2, G, 1) - 0.5) * 2 * math.pi), -1)
    gt[0, :3, 6] = torch.tensor([math.pi, -math.pi, 0.0])
    gt[1, :, 6] = 0.0
    pred = torch.empty(2, P, 7)
    for p in range(P):
        k, cat = p % G, (p // G) % 10
        for b in range(2):
            q = gt[b, k].clone()
            if cat == 0:    # generic
                q[:3] += torch.randn(3, generator=g) * 0.6
                q[3:6] = 0.2 + r(3) * 2.5
                q[6] = (r(1)[0] - 0.5) * 2 * math.pi
            elif cat == 1:  # nested
                q[3:6] *= 0.3 + 0.5 * r(3)
            elif cat == 2:  # partial
                q[:3] += (r(3) - 0.5) * q[3:6]
                q[6] += (r(1)[0] - 0.5) * 0.8
            elif cat == 3:  # identical
                pass
            elif cat == 4:  # disjoint
                q[:2] += 6.0 + r(2)
            elif cat == 5:  # shared centre
                q[3:6] = 0.2 + r(3) * 2.5
                q[6] = (r(1)[0] - 0.5) * 2 * math.pi
            elif cat == 6:  # edges touching: shifted along the box's own x axis by the sum of the half widths
                w2 = 0.3 + r(1)[0]
                d = 0.5 * (q[3] + w2)
                q[0] += d * math.cos(float(q[6]))
                q[1] += d * math.sin(float(q[6]))
                q[3] = w2
            elif cat == 7:  # thin: one edge 1e-3 next to 3 m ones
                q[3:6] = torch.tensor([3.0, 3.0, 3.0])
                q[3 + int(r(1)[0] * 3) % 3] = 1e-3
                q[:3] += torch.randn(3, generator=g) * 0.3
            elif cat == 8:  # the (x, y, w) quirk: same centre and angle, different w
                q[3] *= 0.5 + 0.3 * r(1)[0]
            else:           # angles at +-pi
                q[:3] += torch.randn(3, generator=g) * 0.3
                q[6] = math.pi if p % 2 else -math.pi
            if b == 1:
                q[6] = 0.0
            pred[b, p] = q
    return pred.float(), gt.float()


@pytest.mark.parametrize("iou_type", ["diou", "iou"])
def test_pairwise_values_against_restatement(iou_type):
    from vdetr_amd.criterion import pack_ground_truth
    pred, gt = designed_pairs()
    counts = (13, 16)  # scene 0: slots 13..15 are absent and must read exactly 0
    st = {k: v.to(DEV) for k, v in stage_from_boxes(pred).items()}
    tg = {k: v.to(DEV) for k, v in targets_from_boxes(gt, counts).items()}
    crit = crit_for(iou_type)
    records = pack_ground_truth(tg)
    nactual = torch.tensor(counts, dtype=torch.int64, device=DEV)
    _, giou_t = crit.matcher.cost(st, records, records.shape[1], nactual, want_giou=True)
    got = giou_t.transpose(1, 2).cpu().double()                                        # [B,P,G]
    want = R.pairwise(pred.double(), gt.double(), iou_type == "diou").detach()
    want[0, :, 13:] = 0
    assert got.numel() >= 10000
    assert torch.isfinite(got).all()
    assert torch.equal(got[0, :, 13:], torch.zeros_like(got[0, :, 13:]))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=2e-5)
    ident = torch.arange(pred.shape[1]) // 16 % 10 == 3
    k = torch.arange(pred.shape[1]) % 16
    np.testing.assert_allclose(got[1, ident, k[ident]].numpy(), 1.0, atol=1e-5)
    keep = ident & (k < 13)
    np.testing.assert_allclose(got[0, keep, k[keep]].numpy(), 1.0, atol=1e-5)
    if iou_type == "diou":  # same centre, different w: the r2 term of the reference is non-zero
        quirk = (torch.arange(pred.shape[1]) // 16 % 10 == 8) & (k < 13)
        iou = R.pairwise(pred.double(), gt.double(), False)
        assert (iou[0, quirk, k[quirk]] - got[0, quirk, k[quirk]]).min() > 1e-4


def _oracle_run(monkeypatch, iou_type, outputs_cpu, targets, **kw):
    monkeypatch.setattr(CO, "pair_terms", R.pair_terms_for(iou_type))
    loss, loss_dict, assigns = CO.set_criterion(outputs_cpu, targets, **kw)
    loss.backward()
    return loss, loss_dict, assigns


def _leaves(stage, dev, keys):
    return {k: (v.detach().to(dev).requires_grad_(k in keys)) for k, v in stage.items()}


@pytest.mark.parametrize("iou_type", ["diou", "iou"])
def test_box_parameter_gradients_against_restatement(iou_type, monkeypatch):
    """d loss / d (center, size, angle) of the decoded boxes against fp64 autograd of the restatement, generic rotated
    boxes (scene 0) and axis-aligned ones (scene 1: the enclosing box's corner ties decide the angle gradient)."""
    g = torch.Generator().manual_seed(11)
    B, P, G = 2, 96, 12
    gt = torch.cat((1 + torch.rand((B, G, 3), generator=g) * torch.tensor([8.0, 6.0, 3.0]), 0.3 + torch.rand((B, G, 3), generator=g) * 2,
                    (torch.rand((B, G, 1), generator=g) - 0.5) * 2.5), -1)
    pred = gt[:, torch.arange(P) % G].clone()
    pred[..., :3] += torch.randn((B, P, 3), generator=g) * 0.4
    pred[..., 3:6] *= 0.6 + 0.8 * torch.rand((B, P, 3), generator=g)
    pred[..., 6] += torch.randn((B, P), generator=g) * 0.3
    gt[1, :, 6], pred[1, :, 6] = 0.0, 0.0
    keys = ("center_unnormalized", "size_unnormalized", "angle_continuous", "sem_cls_logits", "center_reg", "size_reg")
    base = stage_from_boxes(pred)
    tg = targets_from_boxes(gt, (G, G - 3))
    st_d, st_c = _leaves(base, DEV, keys), _leaves(base, "cpu", keys)
    crit = crit_for(iou_type, repeat_num=1, is_bilable=False)
    loss, _ = crit({"outputs": st_d}, {k: v.to(DEV) for k, v in tg.items()})
    loss.backward()
    ref_loss, _, ref_assign = _oracle_run(monkeypatch, iou_type, {"outputs": st_c}, tg, repeat_num=1, is_bilable=False)
    inds, mask = crit.last_assignments()[0][0]
    ri, rm = ref_assign["outputs"]
    assert torch.equal(mask.cpu(), rm) and torch.equal(inds.cpu() * (rm > 0), ri * (rm > 0).long())
    assert rm.sum() > 0
    np.testing.assert_allclose(float(loss), float(ref_loss), rtol=1e-4)
    for k in ("center_unnormalized", "size_unnormalized", "angle_continuous"):
        np.testing.assert_allclose(st_d[k].grad.cpu().numpy(), st_c[k].grad.numpy(), rtol=1e-3, atol=1e-6, err_msg=k)
    assert np.abs(st_c["angle_continuous"].grad[1].numpy()).max() > 0, "axis-aligned pairs carry an angle gradient"
    assert st_d["box_corners"].grad is None


def test_identical_boxes_have_finite_gradients():
    pred, gt = designed_pairs(seed=3, G=8, P=8)
    pred[:, :, :] = gt  # every prediction equals its box
    keys = ("center_unnormalized", "size_unnormalized", "angle_continuous")
    st = _leaves(stage_from_boxes(pred), DEV, keys)
    crit = crit_for("diou", repeat_num=1, is_bilable=False)
    loss, loss_dict = crit({"outputs": st}, {k: v.to(DEV) for k, v in targets_from_boxes(gt, (8, 8)).items()})
    loss.backward()
    for k in keys:
        assert torch.isfinite(st[k].grad).all(), k
    assert float(loss_dict["loss_giou"]) < 1e-4  # DIoU 1 on every matched pair


@pytest.mark.parametrize("name", ROT_CASES)
def test_criterion_matches_reference_fixture(name):
    """loss, every loss_dict entry, assignments and gradients against criterion.py's own diou / iou run"""
    outputs, targets, z = load_rot_case(name, DEV)
    crit = crit_for(str(z["iou_type"]), repeat_num=int(z["repeat_num"]))
    loss, loss_dict = crit(outputs, targets)
    loss.backward()
    matches, _ = crit.last_assignments()
    nst = int(z["S"]) + 2
    by_stage = {nst - 1: matches[0], **{k: matches[k + 1] for k in range(nst - 1)}}
    check_rot_against_golden(z, outputs, loss, loss_dict, by_stage, rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize("iou_type,rotated", [("diou", False), ("diou", True), ("iou", False), ("iou", True)])
def test_criterion_full_size_against_oracle(iou_type, rotated, monkeypatch):
    """C2 shapes: a 4096-token first stage, 3 x 1024-query later stages, 64 slots with 41 present, repeat_num 5."""
    from oracle.make_golden import synthetic_stage, synthetic_targets
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    cfg = ScannetDatasetConfig()
    g = torch.Generator().manual_seed(7 + rotated)
    B = 1
    targets = synthetic_targets(g, cfg, B, 64, (41,), 18, rotated=rotated)
    near = targets["gt_box_centers"][:, :41]
    stages = [synthetic_stage(g, cfg, B, 4096, 1, rotated=rotated, near=near)] + [
        synthetic_stage(g, cfg, B, 1024, 18, rotated=rotated, near=near) for _ in range(3)]
    for st in stages:
        st["angle_continuous"] = (torch.rand((B, st["center_reg"].shape[1]), generator=g) - 0.5) * 2.0 if rotated \
            else torch.zeros((B, st["center_reg"].shape[1]))
    seed_xyz = torch.rand((B, 4096, 3), generator=g) * torch.tensor([8.0, 6.0, 3.0]) + 1
    point_logits = torch.randn((B, 4096, 18), generator=g) - 1
    keys = ("sem_cls_logits", "center_reg", "size_reg", "angle_continuous", "angle_logits", "angle_residual_normalized")

    def outputs_on(dev):
        st = []
        for s in stages:
            d = {k: v.detach().to(dev).requires_grad_(k in keys) for k, v in s.items()}
            d["center_unnormalized"] = d["center_reg"] * d["pre_box_size_unnormalized"] + d["pre_box_center_unnormalized"]
            d["size_unnormalized"] = torch.exp(d["size_reg"]) * d["pre_box_size_unnormalized"]
            d["sem_cls_prob"] = d["sem_cls_logits"]
            st.append(d)
        return {"outputs": st[-1], "aux_outputs": st[:-1], "seed_xyz": seed_xyz.to(dev),
                "enc_outputs": {"point_cls_logits": point_logits.to(dev).requires_grad_(True)}}

    og, oc = outputs_on(DEV), outputs_on("cpu")
    crit = crit_for(iou_type)
    loss, loss_dict = crit(og, {k: v.to(DEV) for k, v in targets.items()})
    loss.backward()
    ref_loss, ref_dict, ref_assign = _oracle_run(monkeypatch, iou_type, oc, targets)
    matches, _ = crit.last_assignments()
    ref_matches = [ref_assign["outputs"]] + [ref_assign[k] for k in range(3)]
    for (inds, mask), (ri, rm) in zip(matches, ref_matches):
        assert torch.equal(mask.cpu(), rm)
        # fp32 device vs fp64 oracle cost: a flipped near-tie would show here
        assert torch.equal(inds.cpu() * (rm > 0), ri * (rm > 0).long())
    np.testing.assert_allclose(float(loss.detach()), float(ref_loss.detach()), rtol=1e-3)
    for k, v in ref_dict.items():
        np.testing.assert_allclose(float(loss_dict[k].detach()), float(v.detach()), rtol=1e-3, atol=1e-6, err_msg=k)
    for sg, sc in zip(og["aux_outputs"] + [og["outputs"]], oc["aux_outputs"] + [oc["outputs"]]):
        for k in ("sem_cls_logits", "center_reg", "size_reg") + (("angle_continuous",) if rotated else ()):
            want = sc[k].grad if sc[k].grad is not None else torch.zeros_like(sc[k])
            np.testing.assert_allclose(sg[k].grad.cpu().numpy(), want.numpy(), rtol=1e-3, atol=1e-6, err_msg=k)


def test_decode_backward_under_the_diou_loss(monkeypatch):
    """box_decode.decode_boxes_joint on random head slabs, then the diou criterion: d loss / d y through the decode node's
    center_unnorm / size_unnorm / angle_cont inputs equals the one of the restatement's loss through the same node."""
    from vdetr_amd.box_decode import decode_boxes_joint
    B, N, A, C1 = 1, 256, 1, 18
    chans = (C1, 3, 3, A, A)
    g = torch.Generator().manual_seed(21)
    y0 = torch.randn(B, 5, max(chans) + 2, N, generator=g) * 0.5
    pre_c = (torch.rand(B, N, 3, generator=g) * 0.8 + 0.1).to(DEV)
    pre_s = (torch.rand(B, N, 3, generator=g) * 0.2 + 0.05).to(DEV)
    dims = [torch.zeros(B, 3, device=DEV), torch.tensor([[8.0, 6.0, 3.0]], device=DEV)]
    gt = torch.cat((torch.rand((B, 8, 3), generator=g) * torch.tensor([8.0, 6.0, 3.0]), 0.3 + torch.rand((B, 8, 3), generator=g),
                    torch.zeros((B, 8, 1))), -1)
    tg = targets_from_boxes(gt, (7,))
    grads = []
    for side in ("device", "restatement"):
        y = y0.to(DEV).requires_grad_(True)
        out = decode_boxes_joint(y, chans, pre_c, pre_s, dims, A, "focalloss_0.25")
        if side == "device":
            loss, _ = crit_for("diou", repeat_num=1, is_bilable=False)({"outputs": out}, {k: v.to(DEV) for k, v in tg.items()})
        else:
            oc = {k: v.cpu() for k, v in out.items() if torch.is_tensor(v)}
            monkeypatch.setattr(CO, "pair_terms", R.pair_terms_for("diou"))
            loss, _, _ = CO.set_criterion({"outputs": oc}, tg, repeat_num=1, is_bilable=False)
        loss.backward()
        grads.append(y.grad.cpu())
    assert grads[0][:, 1:3].abs().max() > 0
    np.testing.assert_allclose(grads[0].numpy(), grads[1].numpy(), rtol=1e-3, atol=2e-6)


def test_diou_criterion_captures_in_a_graph():
    """the whole diou criterion (gradients included) captured on one stream and replayed == an eager run.  As in bench.py's
    criterion leg, everything -- leaves, eager run, warm-up, capture -- lives on one side stream, and no autograd graph
    of an earlier run is kept alive into the capture."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        outputs, targets, z = load_rot_case("criterion_diou_rotated", DEV)
        stages = outputs["aux_outputs"] + [outputs["outputs"]]
        for st in stages:
            del st["center_unnormalized"], st["size_unnormalized"]
        crit = crit_for("diou", repeat_num=int(z["repeat_num"]))
        prep = crit.prepare_targets(targets)
        leaves = [st[k] for st in stages for k in ("center_reg", "size_reg", "angle_continuous")]

        def step():
            for t in leaves:
                t.grad = None
            for st in stages:  # the decoded boxes as the model would produce them, every step
                st["center_unnormalized"] = st["center_reg"] * st["pre_box_size_unnormalized"] + st["pre_box_center_unnormalized"]
                st["size_unnormalized"] = torch.exp(st["size_reg"]) * st["pre_box_size_unnormalized"]
            loss, loss_dict = crit(outputs, prep)
            loss.backward()
            for st in stages:
                del st["center_unnormalized"], st["size_unnormalized"]
            return loss.detach(), torch.stack([loss_dict["loss_giou"], loss_dict["loss_giou_0"]]), [t.grad for t in leaves]

        eager_loss, eager_giou, eager_grads = step()
        eager = (eager_loss.clone(), eager_giou.clone(), [g_.clone() for g_ in eager_grads])
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        loss, giou, cap_grads = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    # the loss sums end in float atomics (order-dependent last bits); the gradients are written per row
    torch.testing.assert_close(loss, eager[0], rtol=1e-6, atol=0)
    torch.testing.assert_close(giou, eager[1], rtol=1e-6, atol=0)
    assert float(eager[1].abs().sum()) > 0
    for a, b in zip(cap_grads, eager[2]):
        assert torch.equal(a, b)


def test_standalone_matcher_reads_iou_type():
    from vdetr_amd.criterion import Matcher, build_criterion, default_criterion_args
    outputs, targets, z = load_rot_case("criterion_diou_aligned", DEV)
    crit = crit_for("diou", repeat_num=1)
    crit(outputs, targets)
    inds, mask = crit.last_assignments()[0][0]
    args = default_criterion_args(iou_type="diou")
    m = Matcher(cls_loss=args.cls_loss, cost_class=args.matcher_cls_cost, cost_giou=args.matcher_giou_cost,
                cost_center=args.matcher_center_cost, cost_objectness=args.matcher_objectness_cost,
                cost_size=args.matcher_size_cost, args=args)
    got = m(outputs["outputs"], targets)
    assert torch.equal(got["proposal_matched_mask"], mask)
    assert torch.equal(got["per_prop_gt_inds"] * (mask > 0), inds * (mask > 0))
    with pytest.raises(ValueError, match="iou_type"):
        build_criterion(default_criterion_args(iou_type="ciou"), None)
