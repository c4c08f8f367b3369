"""The C ABI of the training loop's two launches (vdetr_loss_meter_update_f32, vdetr_adamw_guard_f32): exported, bound, laid out as
the header says, argument errors as status codes before anything is launched; and the meter's numpy restatement against the
reference's recorded SmoothedValue (tests/golden/train_meter.npz).  No GPU needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

SYMS = ("vdetr_loss_meter_update_f32", "vdetr_adamw_guard_f32")
SCHED_FIELDS = ["param", "grad", "exp_avg", "exp_avg_sq", "n", "step", "ticket", "sumsq", "nsumsq", "max_norm", "norm_eps", "norm_out",
                "lr", "beta1", "beta2", "eps", "weight_decay", "lr_table", "n_lr", "lr_offset", "decay_mask", "lr_out"]


def test_entry_points_are_exported_bound_and_declared():
    from test_capi import header_symbols
    from vdetr_amd import _lib
    handle = _lib.lib()
    for sym in SYMS:
        assert sym in _lib.exported_symbols(), sym
        assert sym in header_symbols(), sym
        assert hasattr(handle, sym), sym
    assert header_symbols() == _lib.exported_symbols()
    assert handle.vdetr_abi_version() == 3  # additive: the version and every existing descriptor stay


@pytest.mark.parametrize("cls_name,c_name,fields,size", [
    ("LossMeterState", "vdetr_loss_meter_state", ["total", "count", "bad_iter", "bad", "window", "ring"], 8 + 8 + 8 + 4 + 4 + 64 * 4),
    ("LossMeterDesc", "vdetr_loss_meter_desc", ["loss", "state", "iter"], 3 * 8),
    ("AdamWGuardDesc", "vdetr_adamw_guard_desc", SCHED_FIELDS + ["skip"], 168 + 8),
    ("AdamWSchedDesc", "vdetr_adamw_sched_desc", SCHED_FIELDS, 168)])                 # unchanged
def test_layouts_match_the_header(tmp_path, cls_name, c_name, fields, size):
    """sizeof / offsetof of every field, as gcc compiles include/vdetr_hip.h"""
    from vdetr_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    cls = getattr(_lib, cls_name)
    assert [f[0] for f in cls._fields_] == fields
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vdetr_hip.h"', 'int main(void) {',
             f'  printf("%zu\\n", sizeof({c_name}));']
    want = [(f"sizeof({c_name})", ctypes.sizeof(cls))]
    for field in cls._fields_:
        lines.append(f'  printf("%zu\\n", offsetof({c_name}, {field[0]}));')
        want.append((f"offsetof({c_name}, {field[0]})", getattr(cls, field[0]).offset))
    lines += ['  printf("%d\\n", VDETR_LOSS_METER_MAX_WINDOW);', '  return 0;', '}']
    c_file = tmp_path / "layout.c"
    c_file.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(c_file), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(got.pop()) == _lib.VDETR_LOSS_METER_MAX_WINDOW == 64
    assert len(got) == len(want)
    bad = [(what, int(g), w) for (what, w), g in zip(want, got) if int(g) != w]
    assert not bad, bad
    assert ctypes.sizeof(cls) == size


def test_the_guard_descriptor_is_the_sched_descriptor_and_one_pointer():
    from vdetr_amd import _lib
    for name in SCHED_FIELDS:
        assert getattr(_lib.AdamWGuardDesc, name).offset == getattr(_lib.AdamWSchedDesc, name).offset, name
    assert _lib.AdamWGuardDesc.skip.offset == ctypes.sizeof(_lib.AdamWSchedDesc)
    assert _lib.LossMeterState.bad.offset == 24 and _lib.LossMeterState.ring.offset == 32


def _spare():
    buf = np.zeros(1024, np.uint8)
    return buf, (buf.ctypes.data + 255) & ~255


def test_loss_meter_update_rejects_bad_arguments():
    """status 1 with a message naming the entry point and the value; nothing is launched (there is no device here to launch on)"""
    from vdetr_amd import _lib
    lib = _lib.lib()
    keep, p = _spare()
    fn = lib.vdetr_loss_meter_update_f32
    assert fn(None, None) == 1
    assert b"loss_meter_update" in lib.vdetr_last_error() and b"null descriptor" in lib.vdetr_last_error()
    for text, fields in [(b"loss is NULL", dict(loss=None)), (b"state is NULL", dict(state=None)), (b"iter=-1", dict(iter=-1)),
                         (b"iter=-7", dict(iter=-7)), (b"aligned", dict(state=p + 4)), (b"aligned", dict(loss=p + 2))]:
        d = _lib.LossMeterDesc(loss=p, state=p + 256, iter=3)
        for name, value in fields.items():
            setattr(d, name, value)
        status = fn(ctypes.byref(d), None)
        err = lib.vdetr_last_error()
        assert status == 1 and b"loss_meter_update" in err and text in err, (fields, status, err)
    del keep


def _guard_desc(_lib, p):
    d = _lib.AdamWGuardDesc()
    d.param, d.grad, d.exp_avg, d.exp_avg_sq = p, p + 64, p + 128, p + 192
    d.n, d.step, d.ticket, d.skip = 16, p + 256, p + 260, p + 264
    d.lr, d.beta1, d.beta2, d.eps, d.weight_decay = 1e-3, 0.9, 0.999, 1e-8, 0.1
    return d


def test_adamw_guard_rejects_bad_arguments():
    """the checks of vdetr_adamw_sched_f32 under the guard's own name, and a null or misaligned `skip`"""
    from vdetr_amd import _lib
    lib = _lib.lib()
    keep, p = _spare()
    fn = lib.vdetr_adamw_guard_f32
    assert fn(None, None) == 1
    assert b"adamw_guard" in lib.vdetr_last_error() and b"null descriptor" in lib.vdetr_last_error()
    cases = [(b"skip is NULL", dict(skip=None)), (b"skip must be 4-B aligned", dict(skip=p + 266)),
             (b"null pointer or empty buffer", dict(param=None)), (b"null pointer or empty buffer", dict(grad=None)),
             (b"null pointer or empty buffer", dict(exp_avg=None)), (b"null pointer or empty buffer", dict(exp_avg_sq=None)),
             (b"null pointer or empty buffer", dict(step=None)), (b"null pointer or empty buffer", dict(ticket=None)),
             (b"null pointer or empty buffer", dict(n=0)), (b"16-B aligned", dict(grad=p + 68)),
             (b"betas (1, 0.999)", dict(beta1=1.0)), (b"lr -0.5", dict(lr=-0.5)), (b"weight_decay -1", dict(weight_decay=-1.0)),
             (b"0 partial sums", dict(sumsq=p + 320, nsumsq=0, max_norm=0.1)), (b"max_norm 0", dict(sumsq=p + 320, nsumsq=2, max_norm=0.0)),
             (b"lr_table null with n_lr 3", dict(n_lr=3)), (b"lr_table given with n_lr 0", dict(lr_table=p + 384)),
             (b"8-B aligned", dict(lr_table=p + 388, n_lr=2)), (b"8-B aligned", dict(lr_out=p + 388)),
             (b"4-B aligned", dict(decay_mask=p + 386))]
    for text, fields in cases:
        d = _guard_desc(_lib, p)
        for name, value in fields.items():
            setattr(d, name, value)
        status = fn(ctypes.byref(d), None)
        err = lib.vdetr_last_error()
        assert status == 1 and err.startswith(b"adamw_guard:") and text in err, (fields, status, err)
    # the entry point it shares its checks with keeps its own name in them
    s = _lib.AdamWSchedDesc()
    assert lib.vdetr_adamw_sched_f32(ctypes.byref(s), None) == 1 and lib.vdetr_last_error() == b"adamw_sched: null pointer or empty buffer"
    del keep


def test_restatement_reproduces_the_recorded_smoothed_value():
    """every recorded property with == after every one of the 25 updates"""
    from train_meter_restatement import FIELDS, Meter
    z = load_golden("train_meter")
    losses = z["losses"]
    assert losses.dtype == np.float32 and losses.shape == (25,) and int(z["window"]) == 10
    meter = Meter(10)
    for i, x in enumerate(losses):
        meter.update(x, i)
        got = meter.fields()
        for k in FIELDS:
            assert got[k] == z[k][i].item(), (i, k, got[k], z[k][i])
    assert meter.bad == 0 and meter.bad_iter == -1


def test_host_snapshot_equals_the_restatement():
    """engine.snapshot (what LossMeter.read derives from a copied block) on the restatement's words"""
    from train_meter_restatement import FIELDS, Meter
    from vdetr_amd import engine
    losses = load_golden("train_meter")["losses"]
    for window in (1, 3, 10, 64):
        meter = Meter(window)
        for i, x in enumerate(losses):
            meter.update(x, i)
            snap = engine.snapshot(float(meter.total), meter.count, meter.bad, meter.bad_iter, meter.window, [float(v) for v in meter.ring])
            want = meter.fields()
            assert all(getattr(snap, k) == want[k] for k in FIELDS + ("bad", "bad_iter")), (window, i)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_restatement_freezes_at_a_non_finite_loss(bad):
    from train_meter_restatement import Meter
    losses = load_golden("train_meter")["losses"].copy()
    losses[7] = bad
    meter, before = Meter(10), None
    for i, x in enumerate(losses):
        if i == 7:
            before = (meter.fields(), meter.ring.copy())
        meter.update(x, i)
        if i >= 7:
            assert meter.bad == 1 and meter.bad_iter == 7
            now = meter.fields()
            assert {k: v for k, v in now.items() if k not in ("bad", "bad_iter")} == {k: v for k, v in before[0].items() if k not in ("bad", "bad_iter")}
            assert np.array_equal(meter.ring, before[1]) and meter.count == 7
    out_of_range = Meter(65)
    out_of_range.update(1.0, 0)
    assert out_of_range.bad == 2 and out_of_range.count == 0
