"""The AdamW launch with a per-step learning rate and a no-decay mask (vdetr_adamw_sched_f32, optim.ClipAdamW(lr_schedule=...,
decay_mask=...)) against torch.optim.AdamW with the two parameter groups of optimizer.py:4-26 whose ``lr`` engine.py:52-56 sets before
every iteration, from the reference's own rates (tests/golden/lr_schedule.npz)."""
import ctypes
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _models(seed=0, copies=2):
    """the small model of tests/test_gpu_optim.py, `copies` times with the same weights"""
    torch.manual_seed(seed)
    def make():
        return torch.nn.Sequential(torch.nn.Linear(37, 64), torch.nn.ReLU(), torch.nn.Linear(64, 129), torch.nn.LayerNorm(129),
                                   torch.nn.Linear(129, 5, bias=False)).to(DEV)
    ms = [make() for _ in range(copies)]
    for m in ms[1:]:
        m.load_state_dict(ms[0].state_dict())
    return ms


def _table():
    return load_golden("lr_schedule")["cosine_warm:table"]


def _exempt(name, p):  # optimizer.py:11
    return p.ndim == 1 or name.endswith("bias")


@pytest.mark.parametrize("max_norm,use_table,use_mask", [(0.1, True, True), (None, True, True), (0.1, False, True), (0.1, True, False)])
def test_scheduled_masked_step_equals_torch(max_norm, use_table, use_mask):
    """twelve steps at entries 58 .. 69 of the cosine table (lr_offset 58): the warm-up ends with entry 63, so six steps of either
    part; the mask alone (constant rate) and the table alone (everything decayed) as well"""
    from vdetr_amd.dist import FlatParams
    from vdetr_amd.optim import ClipAdamW
    table, off = _table(), 58
    assert table[off + 5] > table[off + 4] and table[off + 7] < table[off + 6]  # both parts
    ref, own = _models(1)
    no_decay = [p for n, p in ref.named_parameters() if use_mask and _exempt(n, p)]
    decay = [p for n, p in ref.named_parameters() if not (use_mask and _exempt(n, p))]
    groups = [{"params": no_decay, "weight_decay": 0.0}, {"params": decay, "weight_decay": 0.1}]
    opt_ref = torch.optim.AdamW([g for g in groups if g["params"]], lr=7e-4)
    flat = FlatParams(list(own.parameters()))
    opt = ClipAdamW(flat, lr=7e-4, weight_decay=0.1, max_norm=max_norm, lr_schedule=table if use_table else None,
                    decay_mask=flat.decay_mask(own.named_parameters()) if use_mask else None, lr_offset=off)
    g = torch.Generator().manual_seed(3)
    for it in range(12):
        x = torch.randn((16, 37), generator=g).to(DEV) * (10.0 if it % 2 else 0.1)
        for m in (ref, own):
            for p in m.parameters():
                p.grad = None
            (m(x) ** 2).sum().backward()
        if use_table:
            for group in opt_ref.param_groups:
                group["lr"] = float(table[off + it])
        norm_ref = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm) if max_norm is not None else None
        opt_ref.step()
        flat.pack_grads()
        opt.step()
        if max_norm is not None:
            np.testing.assert_allclose(float(opt.grad_norm), float(norm_ref), rtol=2e-6)
        assert float(opt.last_lr) == (float(table[off + it]) if use_table else 7e-4)
        for (n, a), b in zip(ref.named_parameters(), own.parameters()):
            np.testing.assert_allclose(b.detach().cpu().numpy(), a.detach().cpu().numpy(), rtol=2e-5, atol=2e-7, err_msg=f"step {it}: {n}")
    assert float(opt.state[flat.param]["step"]) == 12.0 and int(opt._ticket[0]) == 0
    assert opt.param_groups[0]["lr"] == 7e-4  # the fallback rate is not rewritten


def test_captured_step_follows_the_schedule():
    """ONE captured launch replayed eleven times behind an eager first step = twelve eager steps of an optimizer whose rate the host
    sets to table[i] before step i: the replays read the rate on the device, through the step count"""
    from vdetr_amd.dist import FlatParams
    from vdetr_amd.optim import ClipAdamW
    table = _table()
    a, b = _models(2)
    fa, fb = FlatParams(list(a.parameters())), FlatParams(list(b.parameters()))
    eager = ClipAdamW(fa, lr=1e-3, weight_decay=0.05, max_norm=0.5, norm_from_pack=False, decay_mask=fa.decay_mask(a.named_parameters()))
    sched = ClipAdamW(fb, lr=1e-3, weight_decay=0.05, max_norm=0.5, norm_from_pack=False, decay_mask=fb.decay_mask(b.named_parameters()),
                      lr_schedule=table)
    grads = torch.randn((12, fa.grad.numel()), device=DEV)
    for i in range(12):
        fa.grad.copy_(grads[i])
        eager.param_groups[0]["lr"] = float(table[i])
        eager.step()
    fb.grad.copy_(grads[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sched.step()  # step 1, eager (allocates the partials)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            sched.step()
    torch.cuda.current_stream().wait_stream(s)
    for i in range(1, 12):  # (capturing does not execute)
        fb.grad.copy_(grads[i])
        graph.replay()
    torch.cuda.synchronize()
    assert float(sched.state[fb.param]["step"]) == 12.0 and int(sched._ticket[0]) == 0
    assert float(sched.last_lr) == float(table[11])
    assert torch.equal(fa.data, fb.data)


def _entry(n, p0, g0, mask=None, table=None, offset=0, n_lr=None, lr=1e-2, wd=0.2, steps=2, old=False):
    """`steps` launches of the C entry point on rows at a 16-B aligned pitch -> (p, m, v, step, last rate)"""
    from vdetr_amd import _lib as L
    lib = L.lib()
    buf = torch.zeros((4, (n + 3) // 4 * 4), device=DEV)[:, :n]
    p, grad, m, v = buf[0], buf[1], buf[2], buf[3]
    p.copy_(p0)
    grad.copy_(g0)
    step = torch.zeros((), device=DEV)
    ticket = torch.zeros(4, dtype=torch.int32, device=DEV)
    lr_out = torch.full((), -1.0, dtype=torch.float64, device=DEV)
    d = L.AdamWDesc() if old else L.AdamWSchedDesc()
    d.param, d.grad, d.exp_avg, d.exp_avg_sq = p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr()
    d.n, d.step, d.ticket = n, step.data_ptr(), ticket.data_ptr()
    d.lr, d.beta1, d.beta2, d.eps, d.weight_decay = lr, 0.8, 0.95, 1e-6, wd
    if not old:
        if table is not None:
            d.lr_table, d.n_lr, d.lr_offset = table.data_ptr(), table.numel() if n_lr is None else n_lr, offset
        if mask is not None:
            d.decay_mask = mask.data_ptr()
        d.lr_out = lr_out.data_ptr()
    fn = lib.vdetr_adamw_clip_f32 if old else lib.vdetr_adamw_sched_f32
    for _ in range(steps):
        status = fn(ctypes.byref(d), L.stream_ptr())
        assert status == 0, lib.vdetr_last_error()
    assert int(ticket[0]) == 0
    return p.clone(), m.clone(), v.clone(), float(step), float(lr_out)


def _words(bits):
    """0/1 per element -> the mask words (bit i & 31 of word i >> 5), spare bits 0"""
    bits = np.asarray(bits, dtype=np.uint8)
    padded = np.zeros((bits.size + 31) // 32 * 32, np.uint8)
    padded[:bits.size] = bits
    words = np.packbits(padded.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
    return torch.from_numpy(words.astype(np.uint32).view(np.int32)).to(DEV)


@pytest.mark.parametrize("n", [1, 3, 31, 32, 33, 4099])
def test_mask_at_the_edges_through_the_entry_point(n):
    """Two steps.  AdamW's moments do not read p, so an element's result is that of the all-decayed run where its bit is set and
    that of the undecayed run where it is clear: both runs are held to torch, every mask to their per-element selection bit for bit.
    Masks: random, and a 0 -> 1 / 1 -> 0 boundary at every position of the first two float4, around the word boundaries and in the
    tail that is not a whole float4."""
    gen = torch.Generator().manual_seed(5 + n)
    p0, g0 = torch.randn(n, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV)
    refs = []
    for wd in (0.2, 0.0):  # per element: decay applied / not applied
        pr = torch.nn.Parameter(p0.clone())
        pr.grad = g0.clone()
        o = torch.optim.AdamW([pr], lr=1e-2, weight_decay=wd, betas=(0.8, 0.95), eps=1e-6)
        o.step()
        o.step()
        refs.append(pr.detach())
    all_on = _entry(n, p0, g0)                    # null mask: everything decayed
    all_off = _entry(n, p0, g0, old=True, wd=0.0)  # the existing entry without decay
    assert all_on[3] == all_off[3] == 2.0 and all_on[4] == 1e-2
    np.testing.assert_allclose(all_on[0].cpu().numpy(), refs[0].cpu().numpy(), rtol=2e-5, atol=2e-7)
    np.testing.assert_allclose(all_off[0].cpu().numpy(), refs[1].cpu().numpy(), rtol=2e-5, atol=2e-7)
    if n > 8:
        assert not torch.equal(all_on[0], all_off[0])
    ones = _entry(n, p0, g0, mask=torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=DEV))
    zeros = _entry(n, p0, g0, mask=torch.zeros((n + 31) // 32, dtype=torch.int32, device=DEV))
    for k in range(3):
        assert torch.equal(ones[k], all_on[k]) and torch.equal(zeros[k], all_off[k])
    rng = np.random.default_rng(n)
    masks = [rng.integers(0, 2, n), rng.integers(0, 2, n)]
    for b in sorted({b for b in (1, 2, 3, 4, 5, 6, 7, 8, 31, 32, 33, 63, 64, 65, 4064, 4095, 4096, 4097, 4098, n - 3, n - 2, n - 1) if 0 < b < n}):
        lo = (np.arange(n) < b).astype(np.uint8)
        masks += [lo, 1 - lo]
    for bits in masks:
        got = _entry(n, p0, g0, mask=_words(bits))
        sel = torch.from_numpy(np.asarray(bits).astype(bool)).to(DEV)
        for k in range(3):
            assert torch.equal(got[k], torch.where(sel, all_on[k], all_off[k])), (n, k, np.flatnonzero(np.diff(bits))[:4])
        # ... and against torch, decay applied only where the bit is set
        np.testing.assert_allclose(got[0].cpu().numpy(), torch.where(sel, refs[0], refs[1]).cpu().numpy(), rtol=2e-5, atol=2e-7)


def test_table_indexing_offsets_and_clamping():
    """entry = clamp(step + lr_offset, 0, n_lr - 1): the rate reported AND used (equal to the existing entry at that rate)"""
    n = 301
    gen = torch.Generator().manual_seed(9)
    p0, g0 = torch.randn(n, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV)
    rates = [1e-3, 2e-3, 4e-3, 8e-3, 1.6e-2]
    table = torch.tensor(rates, dtype=torch.float64, device=DEV)
    for offset, steps, want in [(0, 1, 0), (0, 5, 4), (2, 1, 2), (2, 3, 4), (2, 6, 4), (-2, 1, 0), (-2, 3, 0), (-2, 5, 2), (-100, 4, 0), (100, 1, 4),
                                (0, 9, 4)]:
        got = _entry(n, p0, g0, table=table, offset=offset, steps=steps)
        assert got[3] == float(steps) and got[4] == rates[want], (offset, steps, got[4])
    # the rate is the one the update uses: three steps at offset 1 = one step each at rates[1], rates[2], rates[3] from the descriptor
    got = _entry(n, p0, g0, table=table, offset=1, steps=3)
    from vdetr_amd import _lib as L
    buf = torch.zeros((4, 304), device=DEV)[:, :n]
    buf[0].copy_(p0)
    buf[1].copy_(g0)
    step, ticket = torch.zeros((), device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    d = L.AdamWSchedDesc()
    d.param, d.grad, d.exp_avg, d.exp_avg_sq = (buf[k].data_ptr() for k in range(4))
    d.n, d.step, d.ticket = n, step.data_ptr(), ticket.data_ptr()
    d.beta1, d.beta2, d.eps, d.weight_decay = 0.8, 0.95, 1e-6, 0.2
    for k in (1, 2, 3):
        d.lr = rates[k]
        assert L.lib().vdetr_adamw_sched_f32(ctypes.byref(d), L.stream_ptr()) == 0
    assert torch.equal(got[0], buf[0]) and torch.equal(got[1], buf[2]) and torch.equal(got[2], buf[3])
    assert not torch.equal(got[0], _entry(n, p0, g0, table=table, offset=0, steps=3)[0])
    # a table of one entry, whatever the offset
    one = torch.tensor([3e-3], dtype=torch.float64, device=DEV)
    for offset in (0, 5, -5):
        assert _entry(n, p0, g0, table=one, offset=offset, steps=3)[4] == 3e-3
    # the optimizer's offset: set_lr_offset moves eager steps
    from vdetr_amd.dist import FlatParams
    from vdetr_amd.optim import ClipAdamW
    w = torch.nn.Parameter(torch.randn((20, 3), device=DEV))
    flat = FlatParams([w])
    opt = ClipAdamW(flat, lr=1e-3, lr_schedule=np.array(rates), lr_offset=-1)
    flat.grad.normal_()
    seen = []
    for k in range(4):
        if k == 2:
            opt.set_lr_offset(1)
        opt.step()
        seen.append(float(opt.last_lr))
    assert seen == [rates[0], rates[0], rates[3], rates[4]]


def test_resume_keeps_the_step_count_on_the_device(tmp_path):
    """six steps, a checkpoint through torch.save / torch.load(map_location="cpu") (utils/io.py:48-54) or through the per-parameter
    states, six more = twelve uninterrupted ones; the step count is back on the device BEFORE the first launch reads it"""
    from vdetr_amd.dist import FlatParams
    from vdetr_amd.optim import ClipAdamW
    table = _table()
    models = _models(4, copies=4)
    flats = [FlatParams(list(m.parameters())) for m in models]

    def make(i):
        return ClipAdamW(flats[i], lr=7e-4, weight_decay=0.1, max_norm=0.5, norm_from_pack=False, lr_schedule=table, lr_offset=55,
                         decay_mask=flats[i].decay_mask(models[i].named_parameters()))

    grads = torch.randn((12, flats[0].grad.numel()), device=DEV)
    covered = torch.zeros(flats[0].grad.numel(), dtype=torch.bool, device=DEV)
    for p in flats[0].params:
        covered[flats[0].offsets[id(p)]:flats[0].offsets[id(p)] + p.numel()] = True
    grads *= covered  # the alignment padding never has a gradient (and the per-parameter states do not carry its moments)

    def run(opt, flat, lo, hi):
        for i in range(lo, hi):
            flat.grad.copy_(grads[i])
            opt.step()

    whole, first = make(0), make(1)
    run(whole, flats[0], 0, 12)
    run(first, flats[1], 0, 6)
    torch.save({"optimizer": first.state_dict(), "flat": flats[1].data}, tmp_path / "ckpt.pth")
    ckpt = torch.load(tmp_path / "ckpt.pth", map_location="cpu")
    assert ckpt["optimizer"]["state"][0]["step"].device.type == "cpu"

    resumed = make(2)
    flats[2].data.copy_(ckpt["flat"])
    resumed.load_state_dict(ckpt["optimizer"])
    st = resumed.state[flats[2].param]
    assert st["step"].device == flats[2].data.device and st["step"].dtype == torch.float32 and st["step"].ndim == 0 and float(st["step"]) == 6.0
    assert all(st[k].device == flats[2].data.device and st[k].dtype == torch.float32 and st[k].numel() == flats[2].data.numel()
               for k in ("exp_avg", "exp_avg_sq"))
    run(resumed, flats[2], 6, 12)
    assert float(st["step"]) == 12.0 and torch.equal(flats[2].data, flats[0].data)
    assert float(resumed.last_lr) == float(table[55 + 11])

    per_param = [{k: v.cpu() for k, v in d.items()} for d in flats[1].per_param_optimizer_state(first, list(models[1].parameters()))]
    again = make(3)
    flats[3].data.copy_(ckpt["flat"])
    flats[3].load_per_param_optimizer_state(again, per_param, list(models[3].parameters()))
    st = again.state[flats[3].param]
    assert st["step"].device == flats[3].data.device and st["step"].dtype == torch.float32 and float(st["step"]) == 6.0
    run(again, flats[3], 6, 12)
    assert torch.equal(flats[3].data, flats[0].data)

    # a state that does not fit the buffer is refused, not launched on
    other = FlatParams([torch.nn.Parameter(torch.randn((8, 3), device=DEV))])
    with pytest.raises(RuntimeError, match="exp_avg"):
        ClipAdamW(other, lr=7e-4).load_state_dict(ckpt["optimizer"])


def test_bad_tables_and_masks_raise_before_any_launch():
    from vdetr_amd import _lib as L
    from vdetr_amd.dist import FlatParams
    from vdetr_amd.optim import ClipAdamW
    flat = FlatParams([torch.nn.Parameter(torch.randn((40, 3), device=DEV))])
    words = (flat.data.numel() + 31) // 32
    good = np.array([1e-3, 2e-3])
    for bad in (dict(decay_mask=torch.zeros(words + 1, dtype=torch.int32, device=DEV)),
                dict(decay_mask=torch.zeros(words, dtype=torch.int32)),
                dict(decay_mask=torch.zeros(words, dtype=torch.float32, device=DEV)),
                dict(lr_schedule=good.astype(np.float32)),
                dict(lr_schedule=torch.tensor(good, dtype=torch.float32, device=DEV)),
                dict(lr_schedule=torch.tensor(good, dtype=torch.float64)),  # a CPU tensor: the kernel would read a host address
                dict(lr_schedule=np.zeros(0)),
                dict(lr_schedule=torch.zeros(0, dtype=torch.float64, device=DEV)),
                dict(lr_schedule=np.array([1e-3, -1e-3])),
                dict(lr_schedule=np.array([1e-3, float("nan")])),
                dict(lr_schedule=torch.tensor([float("inf")], dtype=torch.float64, device=DEV)),
                dict(lr_schedule=np.ones((2, 2)))):
        with pytest.raises((ValueError, RuntimeError)):
            ClipAdamW(flat, lr=1e-3, **bad)
    assert float(flat.data.abs().sum()) > 0
    # the C entry point: status code + message, nothing launched
    lib = L.lib()
    n = 64
    buf = torch.ones((4, n), device=DEV)
    step, ticket = torch.zeros((), device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    table = torch.tensor([1e-3, 2e-3, 3e-3], dtype=torch.float64, device=DEV)
    mask = torch.zeros(2, dtype=torch.int32, device=DEV)
    d = L.AdamWSchedDesc()
    d.param, d.grad, d.exp_avg, d.exp_avg_sq = (buf[k].data_ptr() for k in range(4))
    d.n, d.step, d.ticket = n, step.data_ptr(), ticket.data_ptr()
    d.lr, d.beta1, d.beta2, d.eps, d.weight_decay = 1e-2, 0.9, 0.999, 1e-8, 0.1
    d.lr_table, d.n_lr = None, 3
    assert lib.vdetr_adamw_sched_f32(ctypes.byref(d), L.stream_ptr()) != 0 and b"lr_table" in lib.vdetr_last_error()
    d.lr_table, d.n_lr = table.data_ptr(), 0
    assert lib.vdetr_adamw_sched_f32(ctypes.byref(d), L.stream_ptr()) != 0 and b"lr_table" in lib.vdetr_last_error()
    d.n_lr = -1
    assert lib.vdetr_adamw_sched_f32(ctypes.byref(d), L.stream_ptr()) != 0 and b"lr_table" in lib.vdetr_last_error()
    d.lr_table, d.n_lr = table.data_ptr() + 4, 2
    assert lib.vdetr_adamw_sched_f32(ctypes.byref(d), L.stream_ptr()) != 0 and b"8-B aligned" in lib.vdetr_last_error()
    d.lr_table, d.n_lr, d.decay_mask = table.data_ptr(), 3, mask.data_ptr() + 2
    assert lib.vdetr_adamw_sched_f32(ctypes.byref(d), L.stream_ptr()) != 0 and b"4-B aligned" in lib.vdetr_last_error()
    d.decay_mask, d.beta1 = mask.data_ptr(), 1.0
    assert lib.vdetr_adamw_sched_f32(ctypes.byref(d), L.stream_ptr()) != 0 and b"betas" in lib.vdetr_last_error()
    assert lib.vdetr_adamw_sched_f32(None, L.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert float(step) == 0.0 and bool((buf == 1).all())


def test_build_optimizer_is_the_references_constructor_call():
    from vdetr_amd.dist import FlatParams
    from vdetr_amd.optim import ClipAdamW, build_optimizer, lr_table
    model, = _models(7, copies=1)
    flat = FlatParams(list(model.parameters()))
    args = Namespace(base_lr=7e-4, warm_lr=1e-6, warm_lr_epochs=9, final_lr=1e-6, lr_scheduler="cosine", max_epoch=20, step_epoch="",
                     weight_decay=0.1, filter_biases_wd=True, clip_gradient=0.1)
    opt = build_optimizer(args, model, flat, iters_per_epoch=7)
    assert isinstance(opt, ClipAdamW) and opt.max_norm == 0.1
    assert opt.param_groups[0]["lr"] == 7e-4 and opt.param_groups[0]["weight_decay"] == 0.1
    assert np.array_equal(opt.lr_schedule.cpu().numpy(), lr_table(args, 7)) and np.array_equal(lr_table(args, 7), _table())
    assert torch.equal(opt.decay_mask, flat.decay_mask(model.named_parameters()))
    (model(torch.randn((4, 37), device=DEV)) ** 2).sum().backward()
    flat.pack_grads()
    opt.step()
    assert float(opt.last_lr) == float(_table()[0]) and float(opt.state[flat.param]["step"]) == 1.0
    args.filter_biases_wd, args.clip_gradient = False, 0.0
    plain = build_optimizer(args, model, FlatParams(list(_models(7, copies=1)[0].parameters())))
    assert plain.decay_mask is None and plain.lr_schedule is None and plain.max_norm is None
