"""attn_bwd_box4.hip's quad walk at key sets whose GROUP sizes are known.

A group is the run of sorted slots of one 64-key chunk whose pairs share their table cells; keys at one position share them for
every query.  The walk keeps the groups of even and odd parity in the two row halves of the matrix instruction's tile
(csrc/box4_walk.h), so what can go wrong depends on where in a quad of four slots the groups end: the key sets below put the
ends on slot 3 only, on every slot, two and three times inside one quad, and into a ragged last chunk.  Reference: the general
kernel (BWD_KERNEL = 1) on the same dS, with the bounds of test_sorted_box_backward_kernel_shapes.
"""
import pytest
import torch

import rpe_nearest_restatement as R
from test_gpu_attention import _rotated_boxes, _scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, NQ = 1, 8
LO, EXT = torch.tensor([1.0, 1.0, 1.0]), torch.tensor([8.0, 6.0, 3.0])  # the room of _scene


def _clusters(sizes, nK, g, centres=None):
    """[1, nK, 3]: consecutive runs of sizes[i] keys at one position each (the last run cut at nK)"""
    if centres is None:
        centres = LO + torch.rand((len(sizes), 3), generator=g) * EXT
    xyz = torch.repeat_interleave(centres, torch.tensor(sizes), dim=0)
    assert xyz.shape[0] >= nK
    return xyz[None, :nK].contiguous()


def _mixed_sizes(nK, g):
    sizes, pool = [], torch.tensor([1, 2, 3, 5, 9])
    while sum(sizes) < nK:
        sizes.append(int(pool[torch.randint(0, 5, (1,), generator=g)]))
    return sizes


def _keys(kind, nK, g):
    if kind == "one":  # one position per 64-key chunk
        return _clusters([64] * ((nK + 63) // 64), nK, g)
    if kind == "distinct":
        return (LO + torch.rand((1, nK, 3), generator=g) * EXT).contiguous()
    if kind == "mixed":
        return _clusters(_mixed_sizes(nK, g), nK, g)
    size = int(kind)
    return _clusters([size] * ((nK + size - 1) // size), nK, g)


def _check(monkeypatch, xyz, verts, tables, cs, rpe, seed, box_must_differ=False):
    from vdetr_amd import attention as A
    monkeypatch.setattr(A, "FUSED_KV_BWD", True)
    nK = xyz.shape[1]
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(s, generator=g).to(DEV) for s in ((B, NQ, 256), (B, nK, 64), (B, nK, 64)))
    wout = torch.randn((B, NQ, 256), generator=g).to(DEV)
    kw = dict(num_heads=4, scale=0.125, shared_kv=True, rpe=rpe, vertices=verts.to(DEV).contiguous(), xyz=xyz.to(DEV),
              cos_sin=None if cs is None else cs.to(DEV))

    def run():
        args = [x.clone().requires_grad_(True) for x in (q, k, v)]
        tb = tables.to(DEV).requires_grad_(True)
        (A.fused_attention(*args, table=tb, **kw) * wout).sum().backward()
        return [a.grad for a in args] + [tb.grad]

    monkeypatch.setattr(A, "BWD_KERNEL", 1)  # the general kernel alone
    ref = run()
    monkeypatch.setattr(A, "BWD_KERNEL", 0)
    got, again = run(), run()
    scale = float(ref[3].abs().max())
    err, l2 = float((got[3] - ref[3]).abs().max()), float((got[3] - ref[3]).norm() / ref[3].norm())
    print(f"dtable: max err {err:.3e} of scale {scale:.3e} ({err / scale:.2e}), relative L2 {l2:.2e}")
    assert scale > 0 and torch.isfinite(got[3]).all()
    assert err <= 3e-4 * scale, "dtable"
    assert l2 < 1e-3, "dtable, relative L2"
    for name, r, o in zip(("dq", "dk", "dv"), ref, got):
        assert torch.equal(r, o), f"{name} differs between the box and the general kernel"
    for name, a, b in zip(("dq", "dk", "dv", "dtable"), got, again):
        assert torch.equal(a, b), f"{name} not reproducible"
    if box_must_differ:  # (different arithmetic: equal bits would mean that the general kernel ran twice)
        assert not torch.equal(got[3], ref[3]), "the box kernel did not run"


def _bilinear():
    from vdetr_amd import attention as A
    return A.RPEConfig()


def test_one_group_per_chunk(monkeypatch):
    """every 64-key chunk at one position of its own: no group end inside a chunk, every quad a single instruction into half 0.
    (Not ALL keys at one position: a softmax's dS sums to zero over the keys of a (query, head), so the gradient of a table
    that every key reads at the same cells is zero but for rounding — measured 1.0e-5 at its largest entry, with the two
    kernels 9e-6 apart — and a bound relative to it tests nothing.  With one position per chunk the sums do not cancel.)"""
    g = torch.Generator().manual_seed(100)
    _, verts, tables, _ = _scene(B, NQ, 256, 5)
    _check(monkeypatch, _keys("one", 256, g), verts, tables, None, _bilinear(), 1)


def test_all_keys_at_one_position(monkeypatch):
    """the literal degenerate case: one group per chunk and the same cells in every chunk.  The gradient is zero but for rounding
    (see above), so only what does not need a scale is asserted: finite, bit-equal run to run, dq / dk / dv those of the general
    kernel, and no entry above the fixed-point resolution's share of the largest |dS| sum — 1e-3 of the non-cancelling case's
    largest entry (0.75, test_one_group_per_chunk: same queries, tables and operand seeds)"""
    from vdetr_amd import attention as A
    monkeypatch.setattr(A, "FUSED_KV_BWD", True)
    g = torch.Generator().manual_seed(100)
    _, verts, tables, _ = _scene(B, NQ, 256, 5)
    xyz = _clusters([256], 256, g)
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(s, generator=g).to(DEV) for s in ((B, NQ, 256), (B, 256, 64), (B, 256, 64)))
    wout = torch.randn((B, NQ, 256), generator=g).to(DEV)
    kw = dict(num_heads=4, scale=0.125, shared_kv=True, rpe=A.RPEConfig(), vertices=verts.to(DEV).contiguous(), xyz=xyz.to(DEV))

    def run():
        args = [x.clone().requires_grad_(True) for x in (q, k, v)]
        tb = tables.to(DEV).requires_grad_(True)
        (A.fused_attention(*args, table=tb, **kw) * wout).sum().backward()
        return [a.grad for a in args] + [tb.grad]

    monkeypatch.setattr(A, "BWD_KERNEL", 1)
    ref = run()
    monkeypatch.setattr(A, "BWD_KERNEL", 0)
    got, again = run(), run()
    print(f"dtable: largest entry {float(got[3].abs().max()):.3e} (general kernel {float(ref[3].abs().max()):.3e})")
    assert torch.isfinite(got[3]).all()
    assert float(got[3].abs().max()) <= 1e-3 * 0.75
    for name, r, o, a in zip(("dq", "dk", "dv"), ref, got, again):
        assert torch.equal(r, o) and torch.equal(o, a), name
    assert torch.equal(got[3], again[3]), "dtable not reproducible"


@pytest.mark.parametrize("size", [2, 3, 4, 5, 7])
def test_groups_of_a_fixed_size(monkeypatch, size):
    """clusters of `size` keys: the bucket order is hashed, so over 4 chunks x 8 queries x 2 z halves the ends fall on every
    slot of a quad; size 4 gives ends on slot 3 only, size 2 on slots 1 and 3"""
    g = torch.Generator().manual_seed(200 + size)
    _, verts, tables, _ = _scene(B, NQ, 256, 5)
    _check(monkeypatch, _keys(str(size), 256, g), verts, tables, None, _bilinear(), 2 + size)


@pytest.mark.parametrize("nK", [256, 200, 64 - 3])
def test_groups_of_mixed_sizes(monkeypatch, nK):
    """sizes drawn from {1, 2, 3, 5, 9}: quads with two ends inside; 200: a ragged last chunk behind three full ones;
    61: fewer keys than a wave, the rolled walk alone"""
    g = torch.Generator().manual_seed(300 + nK)
    _, verts, tables, _ = _scene(B, NQ, nK, 5)
    _check(monkeypatch, _keys("mixed", nK, g), verts, tables, None, _bilinear(), 20 + nK, box_must_differ=True)


def test_every_pair_its_own_group(monkeypatch):
    """256 distinct keys over the room: two or three ends inside most quads, the cut quad"""
    g = torch.Generator().manual_seed(400)
    _, verts, tables, _ = _scene(B, NQ, 256, 5)
    _check(monkeypatch, _keys("distinct", 256, g), verts, tables, None, _bilinear(), 30)


def test_mixed_groups_rotated_boxes(monkeypatch):
    g = torch.Generator().manual_seed(500)
    _, verts, tables, cs = _rotated_boxes(B, NQ, 256, 7)
    _check(monkeypatch, _keys("mixed", 256, g), verts, tables, cs, _bilinear(), 40, box_must_differ=True)


def test_mixed_groups_nearest_lookup(monkeypatch):
    """rpe_quant nearest (the other instantiation of the kernel).  Nearest is discontinuous: the cluster CENTRES are nudged off
    the cell boundaries as test_gpu_attention_nearest.py does with its keys, then repeated, so that a cluster stays one position"""
    from types import SimpleNamespace
    from vdetr_amd import attention as A
    g = torch.Generator().manual_seed(600)
    _, verts, tables, _ = _scene(B, NQ, 256, 5)
    sizes = _mixed_sizes(256, g)
    centres = (LO + torch.rand((1, len(sizes), 3), generator=g) * EXT).contiguous()
    centres = R.clean_keys(verts, centres, SimpleNamespace(table_size=10, log_scale=512.0, max_value=4.0), 1e-4, g)
    _check(monkeypatch, _clusters(sizes, 256, g, centres[0]), verts, tables, None, A.RPEConfig(10, 512.0, 4.0, "nearest"), 50)
