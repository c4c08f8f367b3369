"""GPU: engine.evaluate (the reference's engine.py:125-193) on stub models fed from the reference's APCalculator fixture, its loss
window, its two switches, and on a small real model against the hand-written loop over the host-path APCalculator."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _args(**over):
    a = dict(test_no_nms=False, no_3d_nms=False, nms_iou=0.25, empty_pt_thre=5, conf_thresh=0.0, rotated_nms=False, angle_nms=False,
             angle_conf=False, use_old_type_nms=False, no_cls_nms=False, no_per_class_proposal=False, use_cls_confidence_only=False,
             cls_loss="crossentropy", axis_align_test=False, log_every=10, max_epoch=1)
    a.update(over)
    return types.SimpleNamespace(**a)


def _fixture():
    from test_oracle_ap import NUM_SEMCLS
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "ap_calculator.npz"))
    ds = types.SimpleNamespace(num_semcls=NUM_SEMCLS, class2type={int(i): str(n) for i, n in zip(z["class_ids"], z["class_names"])})
    outs = [{k.split(":")[2]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"b{bi}:out:")} for bi in range(int(z["nbatch"]))]
    tgts = [{k.split(":")[2]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"b{bi}:tgt:")} for bi in range(int(z["nbatch"]))]
    return z, ds, outs, tgts


class _Stub(torch.nn.Module):
    """returns the recorded outputs in turn (on its own device), and remembers what it was given"""

    def __init__(self, outs):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.outs, self.calls, self.seen = outs, 0, []

    def forward(self, inputs):
        assert sorted(inputs) == ["point_cloud_dims_max", "point_cloud_dims_min", "point_clouds"]
        assert not self.training and not torch.is_grad_enabled()
        self.seen.append(inputs["point_clouds"].device.type)
        out = {k: v.to(self.anchor.device).clone() for k, v in self.outs[self.calls % len(self.outs)].items()}
        self.calls += 1
        return {"outputs": out}


def _loader(tgts):
    dims = lambda t: dict(t, point_cloud_dims_min=t["point_clouds"][..., :3].amin(1), point_cloud_dims_max=t["point_clouds"][..., :3].amax(1))  # noqa: E731
    return [dims(t) for t in tgts]


def test_evaluate_reproduces_the_recorded_metrics(capsys):
    from vdetr_amd import engine
    z, ds, outs, tgts = _fixture()
    model = _Stub(outs).to(DEV).train()
    calc, loss_avg, loss_dict = engine.evaluate(_args(), 0, model, None, ds, _loader(tgts), 0)
    assert model.calls == len(outs) and set(model.seen) == {"cuda"} and not model.training
    assert loss_avg == 0.0 and loss_dict is None
    assert calc.metrics_to_str(calc.compute_metrics()) == str(z["text"])
    assert calc.ap_iou_thresh == [0.25, 0.5] and calc.class2type_map is ds.class2type and calc.resident
    assert capsys.readouterr().out == "Evaluate ; Batch [0/3]\n"          # log_every 10: the first batch only, no epoch at 0
    assert engine.compute_learning_rate is __import__("vdetr_amd.optim", fromlist=["x"]).compute_learning_rate


def test_loss_average_is_the_mean_of_the_last_ten():
    from vdetr_amd import engine
    _, ds, outs, tgts = _fixture()
    losses = [0.5 + 0.37 * i * i for i in range(12)]
    state = {"n": 0}

    def criterion(outputs, batch):
        i = state["n"]
        state["n"] += 1
        return torch.tensor(losses[i], device=DEV), {"loss_sem_cls": torch.tensor(float(i), device=DEV)}

    loader = (_loader(tgts) * 4)[:12]
    calc, loss_avg, loss_dict = engine.evaluate(_args(log_every=1000), 3, _Stub(outs).to(DEV), criterion, ds, loader, 0)
    assert state["n"] == 12 and calc.scan_cnt == sum(t["gt_box_present"].shape[0] for t in loader)
    assert loss_avg == torch.tensor(losses[2:], dtype=torch.float32).mean().item()     # SmoothedValue(window_size=10).avg
    assert list(loss_dict) == ["loss_sem_cls"] and float(loss_dict["loss_sem_cls"]) == 11.0


def test_focal_loss_sigmoid_and_axis_aligned_corners(monkeypatch):
    from vdetr_amd import engine
    from vdetr_amd.ap_calculator import APCalculator
    _, ds, outs, tgts = _fixture()
    outs = [dict(o, box_corners_axis_align=o["box_corners"] + 7.0) for o in outs[:1]]
    got = []
    monkeypatch.setattr(APCalculator, "step_meter", lambda self, outputs, targets: got.append(outputs["outputs"]))
    engine.evaluate(_args(), 0, _Stub(outs).to(DEV), None, ds, _loader(tgts[:1]), 0)
    engine.evaluate(_args(cls_loss="focalloss_0.25", axis_align_test=True), 0, _Stub(outs).to(DEV), None, ds, _loader(tgts[:1]), 0)
    plain, switched = got
    assert torch.equal(plain["sem_cls_prob"].cpu(), outs[0]["sem_cls_prob"]) and torch.equal(plain["box_corners"].cpu(), outs[0]["box_corners"])
    assert torch.equal(switched["sem_cls_prob"], outs[0]["sem_cls_prob"].to(DEV).sigmoid())
    assert torch.equal(switched["box_corners"].cpu(), outs[0]["box_corners_axis_align"])


@pytest.fixture
def own_dropout_streams(monkeypatch):
    """Every attention module, residual block and BatchNorm site draws the salt of its dropout stream from a process-wide
    counter when it is built (vdetr_transformer._salt_counter, add_ln._salts, bn_act._salts).  A model built here would move
    those counters for every module that a LATER test of the same process builds and so change that test's dropout masks
    (tests/test_gpu_rowblock.py compares two summation orders in train mode at the edge of its tolerance).  The model of this
    test runs in eval mode, where no stream is read: it draws from counters of its own and the process's are left untouched."""
    import itertools
    from vdetr_amd import add_ln, bn_act, vdetr_transformer
    monkeypatch.setattr(vdetr_transformer, "_salt_counter", itertools.count(1 << 20))
    monkeypatch.setattr(add_ln, "_salts", itertools.count(0x5EED0001 + (1 << 20)))
    monkeypatch.setattr(bn_act, "_salts", itertools.count(0xB0A70001 + (1 << 20)))


def test_small_model_equals_the_hand_written_loop(own_dropout_streams):
    """a small ModelVDETR behind the sparse backbone, two tiny batches: evaluate == model -> sigmoid -> host-path step_meter"""
    from vdetr_amd import engine
    from vdetr_amd.ap_calculator import APCalculator
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    from vdetr_amd.model_vdetr import build_vdetr, default_args
    ds = ScannetDatasetConfig()
    torch.manual_seed(0)
    model = build_vdetr(default_args(dec_nlayers=2, nqueries=32, preenc_npoints=256), ds, "minkowski").to(DEV)
    g = torch.Generator().manual_seed(3)
    args = _args(cls_loss="focalloss_0.25", conf_thresh=0.0)
    loader = []
    for B in (2, 1):
        uu = torch.rand(B, 5000, 2, generator=g)
        cloud = torch.cat((torch.stack((uu[:, :2500, 0] * 4, uu[:, :2500, 1] * 3, torch.zeros(B, 2500)), -1),
                           torch.stack((uu[:, 2500:, 0] * 4, torch.zeros(B, 2500), uu[:, 2500:, 1] * 2.5), -1)), 1) + 1.0
        present = torch.zeros(B, 6)
        present[:, :4] = 1
        centers = torch.rand(B, 6, 3, generator=g) * torch.tensor([4.0, 3.0, 2.5]) + 1
        sizes = 0.4 + torch.rand(B, 6, 3, generator=g)
        loader.append({"point_clouds": cloud, "point_cloud_dims_min": cloud.amin(1), "point_cloud_dims_max": cloud.amax(1),
                       "gt_box_corners": ds.box_parametrization_to_corners(centers, sizes, torch.zeros(B, 6)) * present[..., None, None],
                       "gt_box_sem_cls_label": torch.randint(0, ds.num_semcls, (B, 6), generator=g) * present.long(),
                       "gt_box_present": present})
    calc, loss_avg, _ = engine.evaluate(args, 0, model, None, ds, [dict(b) for b in loader], 0)
    want = APCalculator(dataset_config=ds, ap_iou_thresh=[0.25, 0.5], class2type_map=ds.class2type, no_nms=False, args=args)
    model.eval()
    with torch.no_grad():
        for batch in loader:
            batch = {k: v.to(DEV) for k, v in batch.items()}
            out = model({k: batch[k] for k in ("point_clouds", "point_cloud_dims_min", "point_cloud_dims_max")})
            out["outputs"]["sem_cls_prob"] = out["outputs"]["sem_cls_prob"].sigmoid()
            want.step_meter(out, batch)
    got_m, want_m = calc.compute_metrics(), want.compute_metrics()
    assert calc.scan_cnt == want.scan_cnt == 3
    for thr in (0.25, 0.5):
        assert list(got_m[thr].keys()) == list(want_m[thr].keys())
        for key in want_m[thr]:   # AP: two summation orders of at most 12 + 1 terms; the float32 mAP may round the other way
            assert abs(float(got_m[thr][key]) - float(want_m[thr][key])) <= 13 * 2.0 ** -52 + (2.0 ** -23 if key == "mAP" else 0), (thr, key)
    assert calc.metrics_to_str(got_m) == want.metrics_to_str(want_m)
    assert loss_avg == 0.0
