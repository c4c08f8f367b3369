"""engine.train_one_epoch in its reference form (any torch.optim.Optimizer; CPU tensors) against the reference's own
engine.train_one_epoch as tools/make_train_epoch_golden.py recorded it (tests/golden/train_epoch.npz), against the loop written out
here, and what the function refuses.  No GPU needed."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import train_epoch_cases as CASES
from conftest import load_golden


def _optimizer(model, args):
    return torch.optim.AdamW(model.parameters(), lr=args.base_lr, weight_decay=CASES.WEIGHT_DECAY)


def _fresh(z):
    return CASES.load_params(CASES.DictModel(), z)


def _written_out(z, args, epochs, bad_iter=None):
    """engine.py:59-122 for this model, as plain statements -> (model, [loss_avg per epoch])"""
    model = _fresh(z)
    opt = _optimizer(model, args)
    model.train()
    averages, it = [], 0
    for epoch in range(epochs):
        window = []
        for batch in CASES.loader(z["x"], z["target"], epoch, bad_iter):
            lr = args.warm_lr + (it / 100) * args.max_epoch * ((args.base_lr - args.warm_lr) / args.warm_lr_epochs)   # all ten are warm-up
            for group in opt.param_groups:
                group["lr"] = lr
            opt.zero_grad()
            loss = ((model.net(batch["point_clouds"]) - batch["target"]) ** 2).mean()
            if not math.isfinite(loss.item()):
                return model, averages
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), args.clip_gradient)
            opt.step()
            window.append(loss.item())
            it += 1
        averages.append(torch.tensor(window[-10:], dtype=torch.float32).mean().item())
    return model, averages


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_reference_form_reproduces_the_recorded_run(capsys):
    from vdetr_amd import engine
    z = load_golden("train_epoch")
    args = CASES.settings()
    model = _fresh(z)
    opt = _optimizer(model, args)
    twin, twin_avg = _written_out(z, args, CASES.EPOCHS)
    for epoch in range(CASES.EPOCHS):
        capsys.readouterr()
        ap, curr_iter, curr_lr, loss_avg, loss_dict = engine.train_one_epoch(args, epoch, model, opt, CASES.mse_criterion, None,
                                                                            CASES.loader(z["x"], z["target"], epoch))
        assert ap is None and model.training
        assert curr_iter == int(z[f"epoch{epoch}:curr_iter"]) == (epoch + 1) * CASES.BATCHES
        assert curr_lr == float(z[f"epoch{epoch}:curr_lr"]) == opt.param_groups[0]["lr"]
        assert CASES.cut_eta(capsys.readouterr().out) == list(z[f"epoch{epoch}:lines"])
        assert list(loss_dict) == ["loss_mse"]
        # the fixture was made on another CPU: the project's standing 1e-3 (relative to the largest entry)
        assert abs(loss_avg - float(z[f"epoch{epoch}:loss_avg"])) <= 1e-3 * abs(float(z[f"epoch{epoch}:loss_avg"]))
        assert _rel(loss_dict["loss_mse"], z[f"epoch{epoch}:loss_mse"]) <= 1e-3
        assert loss_avg == twin_avg[epoch]                                   # this process: bits
        for name, p in model.named_parameters():
            assert _rel(p.detach().numpy(), z[f"epoch{epoch}:param:{name}"]) <= 1e-3, name
    for (name, p), q in zip(model.named_parameters(), twin.parameters()):
        assert torch.equal(p, q), name
        # ten warm-up steps move a weight by about 7e-4, far inside 1e-3 of a weight of order one: the CHANGE is held as well.  Two
        # CPUs may round a parameter the other way once per step (2^-23 of its size each), beyond the 1e-3 of the change itself
        first, moved, want = z[f"param:{name}"], p.detach().numpy(), z[f"epoch{CASES.EPOCHS - 1}:param:{name}"]
        assert np.abs(want - first).max() > 1e-4, name
        slack = 10 * 2.0 ** -23 * max(np.abs(want).max(), 1e-3)
        assert np.all(np.abs((moved - first) - (want - first)) <= 1e-3 * np.abs(want - first) + slack), name


def test_a_non_finite_loss_exits_before_the_step(caplog):
    from vdetr_amd import engine
    z = load_golden("train_epoch")
    args = CASES.settings()
    bad_iter = int(z["bad_iter"])
    assert bad_iter == CASES.BAD_ITER == 3
    model = _fresh(z)
    with caplog.at_level("INFO"), pytest.raises(SystemExit) as exit_info:
        engine.train_one_epoch(args, 0, model, _optimizer(model, args), CASES.mse_criterion, None,
                               CASES.loader(z["x"], z["target"], 0, bad_iter=bad_iter))
    assert exit_info.value.code == 1 == int(z["bad:exit_code"])
    assert "Loss in not finite. Training will be stopped." in caplog.text
    twin, _ = _written_out(z, args, 1, bad_iter=bad_iter)               # returns at the bad loss: three completed iterations
    for (name, p), q in zip(model.named_parameters(), twin.parameters()):
        assert torch.equal(p, q), name
        assert _rel(p.detach().numpy(), z[f"bad:param:{name}"]) <= 1e-3, name
        assert not np.array_equal(p.detach().numpy(), z[f"param:{name}"]), name


def test_the_loss_that_is_reduced_is_a_detached_copy(monkeypatch):
    """what goes to all_reduce_average shares no graph with the loss that is back-propagated"""
    from vdetr_amd import engine
    z = load_golden("train_epoch")
    args = CASES.settings()
    seen = []
    monkeypatch.setattr(engine, "all_reduce_average", lambda t: seen.append(t) or t)
    model = _fresh(z)
    engine.train_one_epoch(args, 0, model, _optimizer(model, args), CASES.mse_criterion, None, CASES.loader(z["x"], z["target"], 0))
    assert len(seen) == CASES.BATCHES and all(not t.requires_grad and t.grad_fn is None for t in seen)


def test_refusals():
    from vdetr_amd import engine
    z = load_golden("train_epoch")
    model = _fresh(z)
    args = CASES.settings(use_superpoint=True)
    with pytest.raises(NotImplementedError, match="use_superpoint"):
        engine.train_one_epoch(args, 0, model, _optimizer(model, args), CASES.mse_criterion, None, CASES.loader(z["x"], z["target"], 0))
    args = CASES.settings()
    with pytest.raises(ValueError, match="reducer"):                      # a reducer belongs to the ClipAdamW form
        engine.train_one_epoch(args, 0, model, _optimizer(model, args), CASES.mse_criterion, None, CASES.loader(z["x"], z["target"], 0),
                               reducer=SimpleNamespace(bucket_views=False))
    # the ClipAdamW form's checks, on stand-ins (the optimizer itself has no CPU path): clipping on one side only, two bounds, a
    # hooked reducer, a reducer on another flat buffer
    flat = object()
    for clip, max_norm in ((0.1, None), (0.1, 0.0), (0.0, 0.1), (0, 0.5), (0.1, 0.2)):
        with pytest.raises(ValueError, match="clip_gradient"):
            engine._check_sync_free(CASES.settings(clip_gradient=clip), SimpleNamespace(max_norm=max_norm, flat=flat), None)
    for clip, max_norm in ((0.1, 0.1), (0.0, None), (0, 0.0), (-1.0, None)):
        engine._check_sync_free(CASES.settings(clip_gradient=clip), SimpleNamespace(max_norm=max_norm, flat=flat), None)
    opt = SimpleNamespace(max_norm=0.1, flat=flat)
    with pytest.raises(ValueError, match="bucket_views"):
        engine._check_sync_free(args, opt, SimpleNamespace(bucket_views=True, flat=flat))
    with pytest.raises(ValueError, match="flat"):
        engine._check_sync_free(args, opt, SimpleNamespace(bucket_views=False, flat=object()))
    engine._check_sync_free(args, opt, SimpleNamespace(bucket_views=False, flat=flat))
    with pytest.raises(ValueError, match="window_size"):
        engine.LossMeter(window_size=65)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.LossMeter(device="cpu")
