"""Host side of the scheduled / masked AdamW launch (v-detr_amd/optim.py, FlatParams.decay_mask) against what the reference's own
engine.compute_learning_rate and optimizer.build_optimizer gave (tests/golden/lr_schedule.npz, tools/make_lr_schedule_golden.py)."""
import ctypes
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import load_golden
from optim_sched_cases import SCHEDULES, small_model


def mask_bits(mask, n):
    """the mask words as one 0/1 per bit, bit i & 31 of word i >> 5 at position i"""
    words = mask.cpu().numpy().view(np.uint32)
    return ((words[:, None] >> np.arange(32, dtype=np.uint32)[None]) & 1).reshape(-1).astype(np.uint8), words.size * 32 - n


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_lr_table_is_the_references_bit_for_bit(name):
    from vdetr_amd.optim import compute_learning_rate, lr_table
    g = load_golden("lr_schedule")
    args = Namespace(**json.loads(str(g[f"{name}:settings"])))
    ipe = int(g[f"{name}:iters_per_epoch"])
    want = g[f"{name}:table"]
    got = lr_table(args, ipe)
    assert got.dtype == np.float64 and got.shape == want.shape == (args.max_epoch * ipe,)
    assert (got == want).all(), np.flatnonzero(got != want)[:5]
    assert compute_learning_rate(args, 1.0) >= 0.0  # the closed end of the reference's assertion
    with pytest.raises(AssertionError):
        compute_learning_rate(args, 1.5)


def test_fixture_covers_warm_up_cosine_and_both_steps():
    g = load_golden("lr_schedule")
    cos, nowarm, step = g["cosine_warm:table"], g["cosine_nowarm:table"], g["step:table"]
    assert cos[0] == 1e-6 and (np.diff(cos[:64]) > 0).all() and (np.diff(cos[64:]) < 0).all()  # 9 of 20 epochs x 7: warm-up to 63
    assert nowarm[0] == 7e-4 and (np.diff(nowarm) < 0).all()
    assert sorted(set(step[64:])) == [7e-4 / 100, 7e-4 / 10, 7e-4] and step[12 * 7] == 7e-4 / 10 and step[16 * 7] == 7e-4 / 100


@pytest.mark.parametrize("filter_biases_wd", [True, False])
def test_decay_mask_marks_the_references_decayed_group(filter_biases_wd):
    from vdetr_amd.dist import FlatParams
    g = load_golden("lr_schedule")
    model = small_model()
    named = list(model.named_parameters())
    assert [n for n, _ in named] == list(g["names:all"]) and [list(p.shape) for _, p in named] == json.loads(str(g["shapes:all"]))
    assert sorted(list(g["names:decay"]) + list(g["names:no_decay"])) == sorted(g["names:all"])
    flat = FlatParams(list(model.parameters()))
    mask = flat.decay_mask(named, filter_biases_wd)
    n = flat.data.numel()
    assert mask.dtype in (torch.int32, torch.uint32) and mask.shape == ((n + 31) // 32,) and mask.device == flat.data.device
    decayed = set(g["names:decay"]) if filter_biases_wd else set(g["names:all"])
    want = np.zeros(mask.numel() * 32, np.uint8)
    for name, p in named:
        if name in decayed:
            o = flat.offsets[id(p)]
            want[o:o + p.numel()] = 1
    bits, _ = mask_bits(mask, n)
    assert (bits == want).all()
    assert int(bits.sum()) == sum(p.numel() for name, p in named if name in decayed)  # padding bits are 0
    if filter_biases_wd:  # the rule decay_vector applies: the same elements
        vec = flat.decay_vector(named, 0.5, 0.5)
        assert ((vec.numpy() != 1.0) == bits[:n].astype(bool)).all()


def test_decay_mask_boundaries_inside_a_float4_and_a_word():
    """parameters of 1, 3, 5, 31, 32 and 33 elements back to back (an adjacency group): the boundaries fall inside a float4 and on
    both sides of a word boundary; a slotted group and the 16-B alignment of the rest leave padding, which stays 0"""
    from vdetr_amd.dist import FlatParams
    sizes = (1, 3, 5, 31, 32, 33)
    ps = [torch.nn.Parameter(torch.randn(k, 1)) for k in sizes]
    slotted = [torch.nn.Parameter(torch.randn(3, 2)) for _ in range(2)]
    rest = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(7, 3))]
    named = [(f"g{i}.weight" if i % 2 else f"g{i}.bias", p) for i, p in enumerate(ps)]
    named += [(f"s{i}.weight", p) for i, p in enumerate(slotted)] + [("r0.weight", rest[0]), ("r1.weight", rest[1])]
    flat = FlatParams(ps + slotted + rest, groups=[(ps, None), (slotted, 8)])
    offs = [flat.offsets[id(p)] for p in ps]
    assert offs == [0, 1, 4, 9, 40, 72]  # back to back
    n = flat.data.numel()
    bits, spare = mask_bits(flat.decay_mask(named), n)
    want = np.zeros(n + spare, np.uint8)
    for name, p in named:
        if not (p.ndim == 1 or name.endswith("bias")):
            o = flat.offsets[id(p)]
            want[o:o + p.numel()] = 1
    assert (bits == want).all()
    assert bits[0] == 0 and bits[1:4].all() and not bits[4:9].any() and bits[9:40].all() and not bits[40:72].any() and bits[72:105].all()
    covered = np.zeros(n + spare, bool)
    for p in flat.params:
        covered[flat.offsets[id(p)]:flat.offsets[id(p)] + p.numel()] = True
    assert (~covered).sum() > spare and not bits[~covered].any()  # slot padding, alignment padding, the last word's spare bits
    everything, _ = mask_bits(flat.decay_mask(named, filter_biases_wd=False), n)
    assert (everything.astype(bool) == covered).all()


def test_the_new_symbol_is_bound_and_its_descriptor_extends_the_old_one():
    from vdetr_amd import _lib as L
    assert "vdetr_adamw_sched_f32" in L.exported_symbols()
    restype, argtypes = L._SIGNATURES["vdetr_adamw_sched_f32"]
    assert restype is ctypes.c_int and argtypes[0] is ctypes.POINTER(L.AdamWSchedDesc)
    assert hasattr(L.lib(), "vdetr_adamw_sched_f32")
    old, new = L.AdamWDesc, L.AdamWSchedDesc
    assert ctypes.sizeof(old) == 128  # the existing descriptor, byte for byte: 8 x 8 | 3 x 4 + pad | 8 | 5 x 8
    for name, _ in old._fields_:
        assert getattr(new, name).offset == getattr(old, name).offset
    assert [f[0] for f in new._fields_[len(old._fields_):]] == ["lr_table", "n_lr", "lr_offset", "decay_mask", "lr_out"]
    assert new.lr_table.offset == 128 and ctypes.sizeof(new) == 168


def test_package_exports_the_optimizer():
    import vdetr_amd
    from vdetr_amd import optim
    assert vdetr_amd.ClipAdamW is optim.ClipAdamW and vdetr_amd.build_optimizer is optim.build_optimizer
    assert vdetr_amd.lr_table is optim.lr_table and vdetr_amd.compute_learning_rate is optim.compute_learning_rate
