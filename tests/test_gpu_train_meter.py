"""GPU: the loss meter launch (vdetr_loss_meter_update_f32, engine.LossMeter) against the reference's recorded SmoothedValue
(tests/golden/train_meter.npz) and the numpy restatement, and the guarded AdamW launch (vdetr_adamw_guard_f32,
ClipAdamW.step(skip=...)) against the unguarded one, bit for bit."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from optim_sched_cases import small_model
from train_meter_restatement import FIELDS, Meter

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def losses():
    return load_golden("train_meter")["losses"]


def _same(snap, want):
    return all(getattr(snap, k) == want[k] for k in want)


def test_meter_equals_the_recorded_smoothed_value(losses):
    """the reads after updates 1, 9, 10, 11 and 25: a count below, at and above the window, the ring wrapped once and twice"""
    from vdetr_amd import engine
    z = load_golden("train_meter")
    meter = engine.LossMeter(window_size=10, device=DEV)
    assert meter.bad_flag.dtype == torch.int32 and meter.bad_flag.ndim == 0 and meter.bad_flag.data_ptr() == meter.state.data_ptr() + 24
    dev_losses = torch.from_numpy(losses).to(DEV)
    reads = 0
    for i in range(25):
        meter.update(dev_losses[i], i)
        if i + 1 in (1, 9, 10, 11, 25):
            snap = meter.read()
            reads += 1
            for k in FIELDS:
                assert getattr(snap, k) == z[k][i].item(), (i, k, getattr(snap, k), z[k][i])
            assert snap.bad == 0 and snap.bad_iter == -1
    assert meter.reads == reads == 5 and int(meter.bad_flag) == 0


@pytest.mark.parametrize("window", [1, 64])
def test_other_windows_equal_the_restatement(losses, window):
    from vdetr_amd import engine
    meter, want = engine.LossMeter(window_size=window, device=DEV), Meter(window)
    dev_losses = torch.from_numpy(np.concatenate([losses] * 3)).to(DEV)      # 75 updates: the 64-slot ring wraps as well
    for i in range(dev_losses.numel()):
        meter.update(dev_losses[i], i)
        want.update(float(dev_losses[i]), i)
        if i in (0, 1, 24, 62, 63, 64, 74):
            assert _same(meter.read(), want.fields()), (window, i)
    block = meter.state.cpu().numpy()
    assert np.array_equal(block[32:].view(np.float32), want.ring)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_loss_raises_the_flag_and_freezes_the_meter(losses, bad):
    from vdetr_amd import engine
    meter, want = engine.LossMeter(window_size=10, device=DEV), Meter(10)
    values = torch.from_numpy(losses[:13].copy()).to(DEV)
    values[7] = bad
    for i in range(7):
        meter.update(values[i], i)
        want.update(float(losses[i]), i)
    before = meter.state.clone()
    meter.update(values[7], 7)
    after = meter.state.clone()
    for i in range(8, 13):                                                 # five further finite losses change nothing
        meter.update(values[i], i)
    assert torch.equal(meter.state, after)
    snap = meter.read()
    assert snap.bad == 1 and snap.bad_iter == 7 and int(meter.bad_flag) == 1
    assert _same(snap, {k: v for k, v in want.fields().items() if k not in ("bad", "bad_iter")}) and snap.count == 7
    changed = (before != after).nonzero().flatten().tolist()                # bad_iter (bytes 16 .. 23) and bad (24 .. 27) only
    assert changed and set(changed) <= set(range(16, 28))


@pytest.mark.parametrize("window", [0, -3, 65, 2 ** 31 - 1])
def test_a_window_out_of_range_on_the_device_is_refused_by_the_kernel(window):
    """the window is device data: the kernel does not index with it"""
    from vdetr_amd import engine
    meter = engine.LossMeter(window_size=10, device=DEV)
    meter.state[28:32].view(torch.int32).fill_(window)
    before = meter.state.clone()
    meter.update(torch.tensor(1.5, device=DEV), 0)
    meter.update(torch.tensor(2.5, device=DEV), 1)
    after = meter.state.clone()
    assert int(meter.bad_flag) == 2
    changed = (before != after).nonzero().flatten().tolist()
    assert set(changed) == {24}                                            # the low byte of `bad`


def test_update_validates_its_tensor():
    from vdetr_amd import engine
    meter = engine.LossMeter(device=DEV)
    for bad in (torch.ones(2, device=DEV), torch.ones(()), 1.0):
        with pytest.raises(ValueError, match="one-element"):
            meter.update(bad, 0)
    with pytest.raises(RuntimeError, match="iter=-1"):
        meter.update(torch.ones((), device=DEV), -1)
    meter.update(torch.ones((), device=DEV, dtype=torch.float64) * 3, 0)   # another dtype is converted on the device
    snap = meter.read()
    assert snap.count == 1 and snap.value == 3.0


# ---- the guarded AdamW launch --------------------------------------------------------------------------------------------------
ARMS = [(max_norm, table, mask) for max_norm in (0.1, None) for table, mask in ((True, True), (False, True), (True, False))]


def _table():
    return load_golden("lr_schedule")["cosine_warm:table"]


def _small_pair():
    """optim_sched_cases.small_model() twice with the same weights: 176 parameters, less than one workgroup"""
    torch.manual_seed(3)
    a, b = small_model().to(DEV), small_model().to(DEV)
    b.load_state_dict(a.state_dict())
    return [(list(m.named_parameters()), m) for m in (a, b)]


def _large_pair():
    """a flat buffer of more than one grid stride: the launch has the capped multi_processor_count * 16 workgroups of 256 float4
    lanes (vdetr_adamw_sched_f32), so a workgroup takes a second, partial stride; 70004 is not a multiple of anything in sight"""
    stride = torch.cuda.get_device_properties(0).multi_processor_count * 16 * 256 * 4
    g = torch.Generator(device=DEV).manual_seed(4)
    w = torch.randn((stride // 1024 + 1, 1024), device=DEV, generator=g)
    bias = torch.randn(70004 - 1024, device=DEV, generator=g)
    pairs = []
    for _ in range(2):
        named = [("w.weight", torch.nn.Parameter(w.clone())), ("w.bias", torch.nn.Parameter(bias.clone()))]
        pairs.append((named, None))
    assert w.numel() + bias.numel() > stride and (w.numel() + bias.numel()) % stride == 70004
    return pairs


def _optimizers(pairs, max_norm, table, mask):
    from vdetr_amd.dist import FlatParams
    from vdetr_amd.optim import ClipAdamW
    out = []
    for named, _ in pairs:
        flat = FlatParams([p for _, p in named])
        out.append(ClipAdamW(flat, lr=7e-4, weight_decay=0.1, max_norm=max_norm, norm_from_pack=False,
                             lr_schedule=_table() if table else None, lr_offset=58,
                             decay_mask=flat.decay_mask(named) if mask else None))
    return out


def _everything(opt):
    st = opt.state[opt.flat.param]
    return [opt.flat.data, st["exp_avg"], st["exp_avg_sq"], st["step"], opt.grad_norm, opt.last_lr, opt._ticket]


def _bits_equal(xs, ys):
    return [i for i, (x, y) in enumerate(zip(xs, ys)) if not torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8))]


@pytest.fixture(scope="module")
def large_grads():
    """one set of flat gradients for every arm of the large case (alternately far above and far below the clipping bound)"""
    stride = torch.cuda.get_device_properties(0).multi_processor_count * 16 * 256 * 4
    n = (stride // 1024 + 1) * 1024 + 70004 - 1024
    g = torch.Generator(device=DEV).manual_seed(5)
    return [torch.randn(n, device=DEV, generator=g) * (1e-6 if it % 2 else 1.0) for it in range(7)]


@pytest.mark.parametrize("size", ["small", "large"])
@pytest.mark.parametrize("max_norm,table,mask", ARMS)
def test_guard_with_a_clear_flag_is_the_unguarded_step_and_with_a_raised_one_nothing(size, max_norm, table, mask, large_grads):
    """five steps with skip == 0 against a twin's plain step(): parameters, both moments, the step count, the norm and the rate, bit
    for bit; then one launch with skip == 1: all of those and the ticket word keep every bit; then skip back to 0: the next step is
    the twin's next step"""
    pairs = _small_pair() if size == "small" else _large_pair()
    guarded, plain = _optimizers(pairs, max_norm, table, mask)
    assert guarded.flat.data.numel() == plain.flat.data.numel()
    if size == "large":
        assert guarded.flat.data.numel() == large_grads[0].numel()
    skip = torch.zeros((), dtype=torch.int32, device=DEV)
    gen = torch.Generator().manual_seed(6)

    def gradients(it):
        if size == "large":
            for opt in (guarded, plain):
                opt.flat.grad.copy_(large_grads[it])
            return
        x = torch.randn((16, 7), generator=gen).to(DEV) * (100.0 if it % 2 else 0.01)
        for (_, model), opt in zip(pairs, (guarded, plain)):
            for p in model.parameters():
                p.grad = None
            (model(x) ** 2).sum().backward()
            opt.flat.pack_grads()

    for it in range(5):
        gradients(it)
        guarded.step(skip=skip)
        plain.step()
        assert not _bits_equal(_everything(guarded), _everything(plain)), (it, _bits_equal(_everything(guarded), _everything(plain)))
    assert float(plain.state[plain.flat.param]["step"]) == 5.0
    if max_norm is not None:
        assert float(plain.grad_norm) > 0
    if table:
        assert float(plain.last_lr) == float(_table()[58 + 4])

    gradients(5)
    before = [t.clone() for t in _everything(guarded)]
    skip.fill_(1)
    guarded.step(skip=skip)
    assert not _bits_equal(_everything(guarded), before), _bits_equal(_everything(guarded), before)
    assert int(guarded._ticket[0]) == 0
    skip.fill_(2)                                                          # any nonzero word
    guarded.step(skip=skip)
    assert not _bits_equal(_everything(guarded), before)

    skip.zero_()
    guarded.step(skip=skip)
    plain.step()
    assert not _bits_equal(_everything(guarded), _everything(plain))
    assert float(guarded.state[guarded.flat.param]["step"]) == 6.0 and _bits_equal(_everything(guarded)[:4], before[:4]) == [0, 1, 2, 3]


def test_guard_without_table_and_mask_is_the_clip_launch():
    """the arm train_one_epoch takes with a plain ClipAdamW (the rate from param_groups): the twin's step() is vdetr_adamw_clip_f32"""
    pairs = _small_pair()
    guarded, plain = _optimizers(pairs, 0.1, False, False)
    skip = torch.zeros((), dtype=torch.int32, device=DEV)
    gen = torch.Generator().manual_seed(8)
    for it in range(4):
        x = torch.randn((16, 7), generator=gen).to(DEV) * (100.0 if it % 2 else 0.01)
        for (_, model), opt in zip(pairs, (guarded, plain)):
            for p in model.parameters():
                p.grad = None
            (model(x) ** 2).sum().backward()
            opt.flat.pack_grads()
            opt.param_groups[0]["lr"] = 1e-3 * (it + 1)
        guarded.step(skip=skip)
        plain.step()
        assert not _bits_equal(_everything(guarded)[:5], _everything(plain)[:5]), it
        assert float(guarded.last_lr) == 1e-3 * (it + 1)


def test_skip_is_validated():
    from vdetr_amd.dist import FlatParams
    from vdetr_amd.optim import ClipAdamW
    flat = FlatParams([torch.nn.Parameter(torch.randn((40, 3), device=DEV))])
    opt = ClipAdamW(flat, lr=1e-3)
    flat.grad.normal_()
    data = flat.data.clone()
    for bad in (torch.zeros((), dtype=torch.int64, device=DEV), torch.zeros((), dtype=torch.float32, device=DEV),
                torch.zeros((), dtype=torch.int32), torch.zeros(2, dtype=torch.int32, device=DEV), 0):
        with pytest.raises(ValueError, match="skip"):
            opt.step(skip=bad)
    assert torch.equal(flat.data, data) and float(opt.state[flat.param]["step"]) == 0.0
    opt.step(skip=torch.zeros(1, dtype=torch.int32, device=DEV))            # one element, whatever its shape
    assert float(opt.state[flat.param]["step"]) == 1.0 and not torch.equal(flat.data, data)
