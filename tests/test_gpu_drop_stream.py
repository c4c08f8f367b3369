"""The keep masks the kernels draw against the host restatement of the generator (tests/drop_stream_restatement.py, pinned to known
answers by tests/test_drop_stream.py): bit for bit, per stream and dispatch arm, through the entry points the model uses.

The step's device state {seed, offset} is read back after reset_rng() and begin_step(); the by-value seed of a launch is its
`salt`, the by-value offset 0.  Masks are read out of the kernels as tests/test_gpu_norm_parity.py does (LayerNorm: x = 0, r = 1;
BatchNorm: gamma = 1 on x = 0; relu_dropout: ones) and through attention.dropout_keep_mask.  The row-block kernels draw the same
streams: test_gpu_rowblock_parity.py reads their four masks (and ffn0's two) out of the launches and holds them to the same host
restatement, bit for bit, at a tail block and at three scenes; test_gpu_rowblock.py still holds them to these launches through a
whole layer.  The heads kernels are held to these launches by test_gpu_heads.py.

Not reached at test size: the `(i >> 32)` term of the flat form (a tensor of 2^34 floats); tests/drop_stream_check.cpp covers it
on the host."""
import numpy as np
import pytest
import torch

import drop_stream_restatement as R
from norm_cases import drop_threshold

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture()
def state():
    """unsigned 64-bit {seed, offset} of the step"""
    from vdetr_amd import attention as A
    A.reset_rng()
    A.begin_step(torch.device(DEV))
    s = A.current_rng(torch.device(DEV)).cpu()
    return tuple(int(v) & 0xFFFFFFFFFFFFFFFF for v in s.tolist())


def _scale32(p):
    return np.float32(65536.0) / np.float32(65536 - drop_threshold(p))


def _same(keep, want):
    assert keep.shape == want.shape
    assert torch.equal(keep.cpu().bool(), torch.from_numpy(np.ascontiguousarray(want)))


@pytest.mark.parametrize("C", [256, 512])  # NPASS 1 and 2
def test_add_ln_mask(state, C):
    from vdetr_amd import add_ln as ALN
    rows, p, salt = 9, 0.3, 1234  # one row past a workgroup's 8
    ln = torch.nn.LayerNorm(C).to(DEV)
    y = ALN.add_dropout_layer_norm(torch.zeros(rows, C, device=DEV), torch.ones(rows, C, device=DEV), torch.nn.Dropout(p).train(), ln,
                                   salt=salt)[0].detach().cpu()
    _same(y > 0, R.keep_add_ln(rows, C, p, R.stream(salt, 0, state)))
    assert torch.equal(y[y > 0], torch.full_like(y[y > 0], float(_scale32(p))))


@pytest.mark.parametrize("B,C,N", [(2, 5, 128), (3, 5, 7)])  # the register arm (B N = 256) and the sweep arm (N % 4 != 0)
def test_bn_act_mask(state, B, C, N):
    from vdetr_amd.bn_act import bn_act
    p, salt = 0.3, 77
    y = bn_act(torch.zeros(B, C, N, device=DEV), torch.ones(C, device=DEV), torch.ones(C, device=DEV), None, None, True, 1e-5, 0.1,
               relu=True, dropout_p=p, salt=salt).detach().cpu()
    _same(y > 0, R.keep_bn(B, C, N, p, R.stream(salt, 0, state)))
    assert torch.equal(y[y > 0], torch.full_like(y[y > 0], float(_scale32(p))))


def test_relu_dropout_mask(state):
    from vdetr_amd.bn_act import relu_dropout
    p, salt = 0.1, 9
    y = relu_dropout(torch.ones(5, 256, device=DEV), torch.nn.Dropout(p).train(), salt=salt).detach().cpu()
    _same((y > 0).reshape(-1), R.keep_flat(5 * 256, p, R.stream(salt, 0, state)))
    assert torch.equal(y[y > 0], torch.full_like(y[y > 0], float(_scale32(p))))


# H = 8 reaches head group 1; it goes with the per-head kind, because the library builds shared-KV attention for 4 heads only
# (attn_fill_params refuses any other count)
@pytest.mark.parametrize("H,shared_kv", [(8, False), (4, True)])
def test_attention_mask(state, H, shared_kv):
    from vdetr_amd import attention as A
    B, nQ, nK, p, salt = 2, 5, 33, 0.1, 4242
    keep = A.dropout_keep_mask(B, H, nQ, nK, shared_kv, p, A.current_rng(torch.device(DEV)), salt=salt)
    _same(keep, R.keep_attention(B, H, nQ, nK, p, R.stream(salt, 0, state)))
