"""GPU: engine.train_one_epoch with optim.ClipAdamW (the form that reads nothing back per iteration) against the sequence written
out here, against the reference's recorded run (tests/golden/train_epoch.npz), its reads counted; and on a small real model."""
import itertools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import train_epoch_cases as CASES
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _setup(z):
    from vdetr_amd.dist import FlatParams
    from vdetr_amd.optim import ClipAdamW
    args = CASES.settings()
    model = CASES.load_params(CASES.DictModel(), z).to(DEV)
    flat = FlatParams(list(model.parameters()))
    opt = ClipAdamW(flat, lr=args.base_lr, weight_decay=CASES.WEIGHT_DECAY, max_norm=args.clip_gradient)
    return args, model, flat, opt


def _state(opt):
    st = opt.state[opt.flat.param]
    return [opt.flat.data, st["exp_avg"], st["exp_avg_sq"], st["step"]]


@pytest.fixture(scope="module")
def fixture():
    return load_golden("train_epoch")


@pytest.fixture(scope="module")
def written_out(fixture):
    """zero, forward, loss, backward, pack_grads, step() -- ten times; the state after every iteration and every loss, computed
    once and left alone"""
    from vdetr_amd.engine import compute_learning_rate
    z = fixture
    args, model, flat, opt = _setup(z)
    model.train()
    states, losses, it = [], [], 0
    for epoch in range(CASES.EPOCHS):
        for batch in CASES.loader(z["x"], z["target"], epoch):
            batch = {k: v.to(DEV) for k, v in batch.items()}
            opt.param_groups[0]["lr"] = compute_learning_rate(args, it / (args.max_epoch * CASES.BATCHES))
            for p in flat.params:
                p.grad = None
            loss = ((model.net(batch["point_clouds"]) - batch["target"]) ** 2).mean()
            loss.backward()
            flat.pack_grads()
            opt.step()
            states.append([t.clone() for t in _state(opt)])
            losses.append(loss.detach().clone())
            it += 1
    return states, [float(x) for x in losses]


class _Spy:
    """counts what would make the host wait, outside LossMeter.read(): Tensor.item / .cpu / .tolist / .numpy, cuda.synchronize"""

    def __init__(self, monkeypatch):
        from vdetr_amd import engine
        self.outside, self.meters, inside = [], [], [0]
        spy = self

        class Meter(engine.LossMeter):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                spy.meters.append(self)

            def read(self):
                inside[0] += 1
                try:
                    return super().read()
                finally:
                    inside[0] -= 1

        monkeypatch.setattr(engine, "LossMeter", Meter)
        for owner, name in ((torch.Tensor, "item"), (torch.Tensor, "cpu"), (torch.Tensor, "tolist"), (torch.Tensor, "numpy"),
                            (torch.cuda, "synchronize")):
            real = getattr(owner, name)

            def counted(*a, _real=real, _name=name, **kw):
                if not inside[0]:
                    spy.outside.append(_name)
                return _real(*a, **kw)

            monkeypatch.setattr(owner, name, counted)


def _rel(a, b):
    return abs(a - b) / abs(b)


def test_sync_free_epochs_equal_the_written_out_sequence(fixture, written_out, monkeypatch, capsys):
    from vdetr_amd import engine
    z = fixture
    states, losses = written_out
    args, model, flat, opt = _setup(z)
    for epoch in range(CASES.EPOCHS):
        loader = CASES.loader(z["x"], z["target"], epoch)
        capsys.readouterr()
        with monkeypatch.context() as mp:
            spy = _Spy(mp)
            out = engine.train_one_epoch(args, epoch, model, opt, CASES.mse_criterion, None, loader)
        ap, curr_iter, curr_lr, loss_avg, loss_dict = out
        printed = CASES.cut_eta(capsys.readouterr().out)
        assert spy.outside == [], spy.outside                              # nothing read back beyond the meter's reads
        first = epoch * CASES.BATCHES
        logged = [i for i in range(first, first + CASES.BATCHES) if i % args.log_every == 0]
        assert len(spy.meters) == 1 and spy.meters[0].reads == len(logged) + 1
        if epoch == 0:
            assert spy.meters[0].reads == math.ceil(CASES.BATCHES / args.log_every) + 1
        assert ap is None and model.training
        assert curr_iter == int(z[f"epoch{epoch}:curr_iter"])
        assert curr_lr == float(z[f"epoch{epoch}:curr_lr"]) == opt.param_groups[0]["lr"]
        assert printed == list(z[f"epoch{epoch}:lines"])
        assert list(loss_dict) == ["loss_mse"] and float(loss_dict["loss_mse"]) == losses[curr_iter - 1]
        assert loss_avg == torch.tensor(losses[first:curr_iter], dtype=torch.float32).mean().item()
        assert _rel(loss_avg, float(z[f"epoch{epoch}:loss_avg"])) <= 1e-3   # another machine's CPU: the project's standing 1e-3
        for got, want in zip(_state(opt), states[curr_iter - 1]):
            assert torch.equal(got, want)
    assert float(opt.state[flat.param]["step"]) == 10.0 and int(opt._ticket[0]) == 0
    for name, p in model.named_parameters():
        want = z[f"epoch{CASES.EPOCHS - 1}:param:{name}"]
        assert np.abs(p.detach().cpu().numpy() - want).max() <= 1e-3 * np.abs(want).max(), name


def test_an_inf_loss_stops_at_the_next_read_with_the_state_before_it(fixture, written_out, monkeypatch, caplog):
    """inf at iteration 3, reads at 0, 2 and 4: SystemExit(1) at the read of iteration 4, the state that of three iterations"""
    from vdetr_amd import engine
    z = fixture
    states, _ = written_out
    args, model, flat, opt = _setup(z)
    spy = _Spy(monkeypatch)
    with caplog.at_level("INFO"), pytest.raises(SystemExit) as exit_info:
        engine.train_one_epoch(args, 0, model, opt, CASES.mse_criterion, None, CASES.loader(z["x"], z["target"], 0, bad_iter=CASES.BAD_ITER))
    assert exit_info.value.code == 1 and "Loss in not finite. Training will be stopped." in caplog.text
    assert spy.outside == [] and spy.meters[0].reads == 3
    snap = spy.meters[0].read()
    assert snap.bad == 1 and snap.bad_iter == CASES.BAD_ITER and snap.count == CASES.BAD_ITER
    for got, want in zip(_state(opt), states[CASES.BAD_ITER - 1]):
        assert torch.equal(got, want)
    assert float(opt.state[flat.param]["step"]) == 3.0 and int(opt._ticket[0]) == 0
    assert bool(torch.isfinite(flat.data).all())


def test_an_inactive_reducer_changes_no_bit(fixture, written_out):
    from vdetr_amd import engine
    from vdetr_amd.dist import GradientReducer
    z = fixture
    states, _ = written_out
    args, model, flat, opt = _setup(z)
    reducer = GradientReducer(list(model.parameters()), bucket_views=False, flat=flat)
    assert not reducer.active
    for epoch in range(CASES.EPOCHS):
        engine.train_one_epoch(args, epoch, model, opt, CASES.mse_criterion, None, CASES.loader(z["x"], z["target"], epoch), reducer=reducer)
    for got, want in zip(_state(opt), states[-1]):
        assert torch.equal(got, want)
    hooked = SimpleNamespace(bucket_views=True, flat=flat)
    with pytest.raises(ValueError, match="bucket_views"):
        engine.train_one_epoch(args, 0, model, opt, CASES.mse_criterion, None, CASES.loader(z["x"], z["target"], 0), reducer=hooked)
    with pytest.raises(ValueError, match="clip_gradient"):
        engine.train_one_epoch(CASES.settings(clip_gradient=0.2), 0, model, opt, CASES.mse_criterion, None, CASES.loader(z["x"], z["target"], 0))
    with pytest.raises(ValueError, match="clip_gradient"):
        engine.train_one_epoch(CASES.settings(clip_gradient=0.0), 0, model, opt, CASES.mse_criterion, None, CASES.loader(z["x"], z["target"], 0))
    for got, want in zip(_state(opt), states[-1]):                          # refused before the first batch
        assert torch.equal(got, want)


# ---- a small real model --------------------------------------------------------------------------------------------------------
@pytest.fixture
def own_dropout_streams(monkeypatch):
    """Every attention module, residual block and BatchNorm site draws the salt of its dropout stream from a process-wide counter
    when it is built (vdetr_transformer._salt_counter, add_ln._salts, bn_act._salts).  A model built here would move those
    counters for every module that a LATER test of the same process builds and so change that test's dropout masks.  The model of
    this test draws from counters of its own and the process's are left untouched."""
    from vdetr_amd import add_ln, bn_act, vdetr_transformer
    monkeypatch.setattr(vdetr_transformer, "_salt_counter", itertools.count(1 << 21))
    monkeypatch.setattr(add_ln, "_salts", itertools.count(0x5EED0001 + (1 << 21)))
    monkeypatch.setattr(bn_act, "_salts", itertools.count(0xB0A70001 + (1 << 21)))


@pytest.mark.parametrize("deferred", [True, False])
def test_small_real_model_trains_an_epoch(own_dropout_streams, deferred):
    """ModelVDETR behind the sparse backbone with the device criterion: one epoch of two iterations, with the weight gradients
    parked until after backward (runtime.defer_weight_grads) and without.  No bits against a second run: DESIGN.md 3 records how
    far two correct fp32 runs of this model drift apart."""
    from vdetr_amd import engine, runtime
    from vdetr_amd.criterion import build_criterion, default_criterion_args
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    from vdetr_amd.dist import FlatParams
    from vdetr_amd.model_vdetr import build_vdetr, default_args
    from vdetr_amd.optim import build_optimizer
    ds = ScannetDatasetConfig()
    torch.manual_seed(0)
    model = build_vdetr(default_args(dec_nlayers=2, nqueries=32, preenc_npoints=256), ds, "minkowski").to(DEV)
    criterion = build_criterion(default_criterion_args(), ds)
    args = CASES.settings(max_epoch=1, warm_lr_epochs=0, base_lr=7e-4, weight_decay=0.1, filter_biases_wd=True, log_every=10)
    flat = FlatParams(list(model.parameters()))
    opt = build_optimizer(args, model, flat)
    before = flat.data.clone()
    seen = []

    def wrapped(outputs, batch):
        loss, loss_dict = criterion(outputs, batch)
        seen.append((loss.detach().clone(), list(loss_dict)))
        return loss, loss_dict

    runtime.defer_weight_grads(deferred)
    try:
        assert runtime.weight_grads_deferred() == deferred
        ap, curr_iter, curr_lr, loss_avg, loss_dict = engine.train_one_epoch(args, 0, model, opt, wrapped, ds, CASES.real_scenes(ds))
    finally:
        runtime.defer_weight_grads(False)
    assert ap is None and curr_iter == 2 and len(seen) == 2
    assert curr_lr == engine.compute_learning_rate(args, 1 / 2) == opt.param_groups[0]["lr"]
    assert float(opt.state[flat.param]["step"]) == 2.0 and int(opt._ticket[0]) == 0
    assert bool(torch.isfinite(flat.data).all()) and not torch.equal(flat.data, before)
    for name, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), name
    assert loss_avg == torch.tensor([float(l) for l, _ in seen], dtype=torch.float32).mean().item() and math.isfinite(loss_avg)
    assert sorted(loss_dict) == sorted(seen[-1][1]) and len(loss_dict) > 0
