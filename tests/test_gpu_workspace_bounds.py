"""Every launch that takes a caller-provided workspace, on a buffer that is NOT 256-B aligned, has not one byte to spare and
holds no zero.

Every workspace the package hands to the library comes from torch's allocator: it starts on a multiple of 256 B and is rounded
up to at least 512 B, so neither the rounding of the start, nor a size function that counts one partial too few, nor a word
read before it was written is exercised anywhere else.  Here `_lib.workspace` is replaced (tests/workspace_guard.py): a request
of n bytes gets the n-byte view that starts `front` bytes past a 256-B boundary of an allocation filled with 0xA5; the view
itself is filled with 0xFF (NaN as a float, -1 as an int).  After the op the bytes in front and behind must still read 0xA5, and
the results must be those of the ordinary workspace.

`front` is 8 for the layouts that round the start themselves (csrc/workspace.h: nms, fps, the attention passes, the loader
chain, the scan export, the union / prune / voxel maps) and 16 for the layouts whose descriptor carries a bare pointer (their
contract, include/vdetr_hip.h: 16-B aligned).  The guard behind the view is 256 B or one further unit of the op's layout,
whichever is larger; every test names its unit.  Every test makes three assertions: the number of workspaces asked for is the
number the host code is expected to ask for (no path skips the guard), the guards are untouched, and the results equal those of
the same call on the ordinary workspace (`monkeypatch.undo()`), bit for bit where the op is documented as deterministic.
Every docstring says which launch writes each region before which launch reads it.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_attention import _scene
from workspace_guard import guarded  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _boxes(B, K, seed, rotated):
    """K boxes per scene around 12 centres, so that many overlap; corners in the order of the reference's box parametrisation"""
    g = torch.Generator().manual_seed(seed)
    centre = (torch.rand((B, 12, 3), generator=g) * 4)[:, torch.randint(0, 12, (K,), generator=g)] + 0.2 * torch.randn((B, K, 3), generator=g)
    half = 0.3 + 0.4 * torch.rand((B, K, 3), generator=g)
    ang = torch.rand((B, K), generator=g) * 3.1 if rotated else torch.zeros((B, K))
    sx = torch.tensor([1.0, 1, -1, -1, 1, 1, -1, -1])
    sy = torch.tensor([1.0, 1, 1, 1, -1, -1, -1, -1])
    sz = torch.tensor([1.0, -1, -1, 1, 1, -1, -1, 1])
    x, y, z = half[..., 0:1] * sx, half[..., 1:2] * sy, half[..., 2:3] * sz
    c, s = torch.cos(ang)[..., None], torch.sin(ang)[..., None]
    corners = torch.stack((c * x + s * z, y, -s * x + c * z), -1) + centre[:, :, None, :]
    return corners.to(DEV).contiguous(), torch.rand((B, K), generator=g).to(DEV), torch.randint(0, 3, (B, K), generator=g).to(DEV)


@pytest.mark.parametrize("rotated", [False, True])
def test_nms_workspace_stays_inside_its_bytes(monkeypatch, guarded, rotated):
    """B 2, K 70: two 64-bit mask words per row, all three regions.  The keep mask is bit-equal."""
    from vdetr_amd import nms
    corners, scores, classes = _boxes(2, 70, 5, rotated)
    keep = nms.batched_nms_3d(corners, scores, classes, iou_threshold=0.25, rotated=rotated)
    assert guarded() == 1
    monkeypatch.undo()
    ref = nms.batched_nms_3d(corners, scores, classes, iou_threshold=0.25, rotated=rotated)
    assert guarded() == 1, "the second run is meant to take the ordinary workspace"
    assert 0 < int(ref.sum()) < ref.numel(), "the case must suppress some boxes and keep some"
    assert torch.equal(keep, ref)


@pytest.mark.parametrize("case", ["fixed", "varlen", "buckets"])
def test_fps_workspace_stays_inside_its_bytes(monkeypatch, guarded, case):
    """b 2, n 300, m 16 and the counts [300, 130] on the row kernel (fps_rows.hip); `buckets` is the cloud of
    test_fps_large_property, past the row kernel's 262,144 points, on fps.hip's own kernel.  Indices are bit-equal."""
    from vdetr_amd import pointnet2_utils as PU
    rng = np.random.default_rng(3)
    if case == "buckets":
        x = torch.from_numpy(rng.uniform(1, 9, size=(1, 300000, 3)).astype(np.float32)).to(DEV)
        run = lambda: PU.furthest_point_sample(x, 64)
    elif case == "fixed":
        x = torch.from_numpy(rng.uniform(1, 9, size=(2, 300, 3)).astype(np.float32)).to(DEV)
        run = lambda: PU.furthest_point_sample(x, 16)
    else:
        clouds = [torch.from_numpy(rng.uniform(1, 9, size=(n, 3)).astype(np.float32)).to(DEV) for n in (300, 130)]
        run = lambda: PU.furthest_point_sample_varlen(clouds, 16)
    got = run()
    assert guarded() == 1
    monkeypatch.undo()
    ref = run()
    assert len(set(ref[0].tolist())) == ref.shape[1]
    assert torch.equal(got, ref)


def _attention_inputs(T):
    B, nQ, nK = 2, 12, 272
    g = torch.Generator().manual_seed(41)
    xyz, verts, tables, _ = _scene(B, nQ, nK, 9)
    q, k, v = torch.randn((B, nQ, 256), generator=g), torch.randn((B, nK, 64), generator=g), torch.randn((B, nK, 64), generator=g)
    wout = torch.randn((B, nQ, 256), generator=g)
    tables = tables[:, :T, :T, :T].contiguous() if T else None
    return [None if x is None else x.to(DEV).contiguous() for x in (q, k, v, wout, tables, verts, xyz)]


@pytest.mark.parametrize("T", [10, 6, 0])
def test_attention_workspaces_stay_inside_their_bytes(monkeypatch, guarded, T):
    """fused_attention forward + backward, shared K/V, H 4, B 2, nQ 12, nK 272 (key split 2, ragged last tile).  Table edge 10:
    the persistent forward with its key-split partials and its own K/V image, the table gradient's partial tables, the key-side
    backward's operand images.  Edge 6: the grid kernel with the key split.  0: no table.  (The package always brings the
    persistent forward's counter; the test below covers the workspace's own.)

    Against the run on the ordinary workspace.  Bit-equal: `out` (every partial is one workgroup's own sum and the merge adds
    them in a fixed order) and `dtable` (an integer fixed-point histogram, which test_sorted_box_backward_kernel_shapes already
    holds to equal bits).  dk and dv are accumulated with float atomics by two workgroups per key tile and dq is the library's
    GEMM on dS: these take the tolerance of test_fused_attention_forward_backward, 1e-3 relative + 1e-4 of the tensor's
    maximum."""
    from vdetr_amd import attention as A
    q, k, v, wout, tables, verts, xyz = _attention_inputs(T)

    def run():
        args = [x.clone().requires_grad_(True) for x in (q, k, v)]
        tb = tables.clone().requires_grad_(True) if T else None
        extra = dict(table=tb, rpe=A.RPEConfig(table_size=T), vertices=verts, xyz=xyz) if T else {}
        out = A.fused_attention(*args, num_heads=4, scale=0.125, shared_kv=True, **extra)
        (out * wout).sum().backward()
        torch.cuda.synchronize()
        return {"out": out.detach(), "dq": args[0].grad, "dk": args[1].grad, "dv": args[2].grad, **({"dtable": tb.grad} if T else {})}

    got = run()
    assert guarded() == (3 if T else 2)                                   # forward, key-side backward, table gradient
    monkeypatch.undo()
    ref = run()
    for name, r in ref.items():
        assert torch.isfinite(r).all() and float(r.abs().max()) > 0, name
        if name in ("out", "dtable"):
            assert torch.equal(got[name], r), name
        else:
            torch.testing.assert_close(got[name], r, rtol=1e-3, atol=1e-4 * float(r.abs().max()) + 1e-7, msg=name)


@pytest.mark.parametrize("nK,regions", [(272, "counter, image and partials"), (64, "counter and image")])
def test_forward_counter_in_the_workspace_head(guarded, nK, regions):
    """vdetr_attn_fwd_f32 called without fwd_sched: the item counter is the 16-B slot at the head of the workspace, in front of
    the 256-B regions.  With nK 64 there is no key split.  `out` and `lse` are bit-equal to fused_attention's, which brings a
    counter of its own."""
    from vdetr_amd import _lib as L
    from vdetr_amd import attention as A
    B, nQ, H = 2, 12, 4
    q, k, v, _, tables, verts, xyz = _attention_inputs(10)
    k, v, xyz = k[:, :nK].contiguous(), v[:, :nK].contiguous(), xyz[:, :nK].contiguous()
    cfg = A.RPEConfig()
    d = A._desc(L.VDETR_ATTN_SHARED_KV, B, H, nQ, nK, 0.125, tables, cfg, verts, xyz, None, None, 0.0, None)
    lib = L.lib()
    nbytes = lib.vdetr_attn_fwd_workspace_bytes(ctypes.byref(d))
    image = lib.vdetr_attn_kv_image_bytes(B, nK)
    assert nbytes == 512 + image + (2 * B * nQ * H * 65 * 4 + 256 if nK == 272 else 0), regions
    ws = L.workspace(nbytes, q.device)
    out, lse = torch.empty_like(q), torch.empty((B, nQ, H), device=DEV)
    L.check(lib.vdetr_attn_fwd_f32(ctypes.byref(d), L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), L.ptr(lse), None, L.ptr(ws), nbytes,
                                   L.stream_ptr()), "attn_fwd")
    assert guarded() == 1
    ref = A.fused_attention(q, k, v, num_heads=H, scale=0.125, shared_kv=True, table=tables, rpe=cfg, vertices=verts, xyz=xyz)
    assert torch.isfinite(ref).all() and torch.equal(out, ref)


# ---- everything added since: the bare-pointer layouts (front 16) and the remaining carved ones (front 8) ------------------------------
SCENES = (33, 0, 37)  # rows per scene: the middle one is empty; 70 rows in all


def _twice(monkeypatch, guarded, run, count):
    """run() on the guarded workspaces, then on the ordinary ones -> (guarded results, ordinary results)"""
    got = run()
    assert guarded() == count
    monkeypatch.undo()
    ref = run()
    assert guarded() == count, "the second run is meant to take the ordinary workspace"
    return got, ref


def _usable(name, r):
    if r.is_floating_point():
        assert bool(torch.isfinite(r).all()), name
    assert bool((r != 0).any()), name


def _bit_equal(got, ref):
    assert list(got) == list(ref)
    for name, r in ref.items():
        _usable(name, r)
        assert got[name].dtype == r.dtype and got[name].shape == r.shape and torch.equal(got[name], r), name


def _seg():
    return torch.tensor([0, 33, 33, 70], dtype=torch.int32, device=DEV)


def _table(seed, *shape):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) + 0.25).to(DEV)


def test_sp_bn_workspace_stays_inside_its_bytes(monkeypatch, guarded):
    """sparse_ops.bn_act, N 70, C 8, training, ReLU, residual, forward + backward: bn_rows is 16, so 5 workgroups, the last with 6
    rows.  Workspace [5][3][8] floats and [2][8] behind them (544 B); unit: one workgroup's partial [3][8] (96 B); 2 workspaces
    (forward, backward).  Bit-equal (fixed merge order, no atomics).
    Forward: sp_bn_stats writes [nblk][3][C] -> sp_bn_finalize reads them; sp_bn_apply reads save_mean / save_invstd only.
    Backward: sp_bn_bwd_stats writes [nblk][2][C] from the head -> sp_bn_bwd_finalize reads them and writes the sums [2][C] at
    nblk * 3 * C -> sp_bn_bwd_apply reads the sums.  The floats between nblk * 2 * C and nblk * 3 * C stay unwritten and unread."""
    from vdetr_amd import sparse_ops as S
    x, res, w = _table(1, 70, 8), _table(2, 70, 8), _table(3, 70, 8)
    guarded.layout(front=16, unit=3 * 8 * 4)

    def run():
        torch.manual_seed(4)
        bn = torch.nn.BatchNorm1d(8).to(DEV).train()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.3)
        xx, rr = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
        y = S.bn_act(xx, bn, "relu", residual=rr)
        (y * w).sum().backward()
        return {"y": y.detach(), "dx": xx.grad, "dres": rr.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
                "running_mean": bn.running_mean.clone(), "running_var": bn.running_var.clone()}

    _bit_equal(*_twice(monkeypatch, guarded, run, 2))


def test_sp_inorm_workspace_stays_inside_its_bytes(monkeypatch, guarded):
    """sparse_ops.instance_norm, N 70, C 8, scenes of 33, 0 and 37 rows, dgamma and dbeta wanted, forward + backward: statistics
    chunks of 16 rows, 3 + 0 + 3 = 6 of them, the last of either scene ragged; the launch has ceil(70 / 16) + 3 = 8 workgroups
    and the size function covers 9 partials (864 B).  Unit: one chunk's partial [3][8] (96 B); 2 workspaces.  Bit-equal.
    Forward: sp_in_stats writes partial b for every chunk b that exists -> sp_in_apply reads the partials p0 .. p0 + np of ITS
    scene, all of which exist.  Backward: sp_in_bwd_stats writes [chunk][2][C] -> sp_in_bwd_apply reads its scene's, and
    sp_in_bwd_params the partials 0 .. (all chunks).  Partials past the last chunk are neither written nor read."""
    from vdetr_amd import sparse_ops as S
    x, w, seg = _table(5, 70, 8), _table(6, 70, 8), _seg()
    guarded.layout(front=16, unit=3 * 8 * 4)

    def run():
        g = torch.Generator().manual_seed(7)
        gamma = (torch.rand(8, generator=g) + 0.5).to(DEV).requires_grad_(True)
        beta = torch.randn(8, generator=g).to(DEV).requires_grad_(True)
        xx = x.clone().requires_grad_(True)
        y = S.instance_norm(xx, seg, 3, gamma, beta)
        (y * w).sum().backward()
        return {"y": y.detach(), "dx": xx.grad, "dgamma": gamma.grad, "dbeta": beta.grad}

    _bit_equal(*_twice(monkeypatch, guarded, run, 2))


@pytest.mark.parametrize("mode", ["sum", "avg", "max"])
def test_sp_global_pool_workspace_stays_inside_its_bytes(monkeypatch, guarded, mode):
    """sparse_ops.global_pool forward, N 70, C 8, scenes of 33, 0 and 37 rows: chunks of 16 rows, 6 of them (two ragged); the
    size function covers min(ceil(70 / 16), 64) + 3 = 8 chunks of values [8] f32 and, behind all values, rows [8] i32 (512 B).
    Unit: one chunk's values and rows (64 B); 1 workspace.  Bit-equal (y; for max also arg).
    sg_pool_sum_part / sg_pool_max_part write part[b] (max: and parg[b]) for every chunk b that exists -> sg_fold_sum /
    sg_fold_max, one workgroup per scene, read the chunks p0 .. p0 + np of their scene (none for the empty one).  sum and avg
    never touch the row half."""
    from vdetr_amd import sparse_ops as S
    x, seg = _table(8, 70, 8), _seg()
    guarded.layout(front=16, unit=8 * 8)

    def run():
        y, arg = S.global_pool(x, seg, 3, mode, return_arg=True)
        return {"y": y, **({"arg": arg} if mode == "max" else {})}

    got, ref = _twice(monkeypatch, guarded, run, 1)
    _bit_equal(got, ref)
    assert not bool(ref["y"][1].any()) and bool(ref["y"][0].all()) and bool(ref["y"][2].all())  # the empty scene gives zeros


@pytest.mark.parametrize("mode,Cg", [("add", 8), ("mul", 8), ("cat", 4)])
def test_sp_broadcast_backward_workspace_stays_inside_its_bytes(monkeypatch, guarded, mode, Cg):
    """sparse_ops.broadcast backward with dg, N 70, Cx 8, scenes of 33, 0 and 37 rows: with dg the sweep runs on the large chunks
    (16 rows, 6 chunks, two ragged); the size function covers 8 chunks of [Cg] floats (256 B / 128 B).  Unit: one chunk's
    partial (Cg * 4 B); 1 workspace.  Bit-equal (dx, dg).
    sg_bcast_bwd writes part[b][0 .. Cg) for every chunk b that exists (cat: from the last Cg columns of dy) -> sg_fold_sum
    reads the chunks of its scene; the empty scene's dg is the fold of nothing, +0."""
    from vdetr_amd import sparse_ops as S
    x, gsrc, seg = _table(9, 70, 8), _table(10, 3, Cg), _seg()
    w = _table(11, 70, 8 + Cg if mode == "cat" else 8)
    guarded.layout(front=16, unit=Cg * 4)

    def run():
        xx, gg = x.clone().requires_grad_(True), gsrc.clone().requires_grad_(True)
        (S.broadcast(xx, gg, seg, 3, mode) * w).sum().backward()
        return {"dx": xx.grad, "dg": gg.grad}

    got, ref = _twice(monkeypatch, guarded, run, 1)
    _bit_equal(got, ref)
    assert not bool(ref["dg"][1].any()) and bool(ref["dg"][0].all()) and bool(ref["dg"][2].all())


def test_sp_se_gate_workspace_stays_inside_its_bytes(monkeypatch, guarded):
    """sparse_ops.se_scale, N 70, C 8, H 4, scenes of 33, 0 and 37 rows: the pooling workspace of the test above (8 chunks of
    64 B), of which the gate uses the value half.  Unit: one chunk (64 B); 1 workspace.  Bit-equal (y = x * gate[s]).
    sg_pool_sum_part writes part[b] for every chunk that exists -> sg_gate, one workgroup per scene, folds the chunks of its
    scene."""
    from vdetr_amd import sparse_ops as S
    x, seg = _table(12, 70, 8), _seg()
    w1, b1, w2, b2 = _table(13, 4, 8), _table(14, 4), _table(15, 8, 4), _table(16, 8)
    guarded.layout(front=16, unit=8 * 8)
    got, ref = _twice(monkeypatch, guarded, lambda: {"y": S.se_scale(x, seg, 3, w1, b1, w2, b2)}, 1)
    _bit_equal(got, ref)


@pytest.mark.parametrize("arm", ["dw and db", "db alone"])
def test_sp_cwconv_wgrad_workspace_stays_inside_its_bytes(monkeypatch, guarded, arm):
    """sparse_ops.channelwise_conv weight gradient, kernel size 3 (K 27), C 8, nout = 2 * chunk_rows + 5 = 133: three chunks of
    64 rows, the last with 5.  Workspace [3][K + 1][8] floats (2688 B); unit: one chunk's partial [K + 1][8] (896 B); 1 workspace.
    Bit-equal (dW, db).
    sp_cwconv_wgrad_part writes rows 0 .. K of every chunk's partial (`db alone`: row K only) -> sp_cwconv_wgrad_fold reads
    rows 0 .. K of every chunk (`db alone`: row K only; its lanes for the rows below K are not live)."""
    from vdetr_amd import sparse_ops as S
    rows = S.cwconv_chunk_rows(133)
    nout = 2 * rows + 5
    assert rows == 64 and nout == 133 and S.cwconv_chunk_rows(nout) == rows
    g = torch.Generator().manual_seed(17)
    nbr = torch.randint(-nout // 2, nout, (27, nout), generator=g).clamp_(min=-1).int().to(DEV)  # about a third of the neighbours absent
    x, dy = _table(18, nout, 8), _table(19, nout, 8)
    guarded.layout(front=16, unit=28 * 8 * 4)

    def run():
        wt = _table(20, 27, 8).requires_grad_(arm == "dw and db")
        b = _table(21, 8).requires_grad_(True)
        (S.channelwise_conv(x, wt, nbr, None, b) * dy).sum().backward()
        return {**({"dw": wt.grad} if arm == "dw and db" else {}), "db": b.grad}

    _bit_equal(*_twice(monkeypatch, guarded, run, 1))


def _keys(seed, n, span):
    """n sorted unique int64 keys out of 0 .. span"""
    return torch.randperm(span, generator=torch.Generator().manual_seed(seed))[:n].sort().values.to(DEV)


def test_sp_union_map_workspace_stays_inside_its_bytes(monkeypatch, guarded):
    """sparse_ops.union_map, na = 2 tiles + 5, nb = 2 tiles + 11 keys, about a third shared: three tiles on either side, the last
    ragged.  Carved: found_pos [na + nb] u32, tile_matches [3 + 3] i32, each rounded up to 256 B.  Unit: one tile's record (one
    int, below the 256 B); 1 workspace.  Bit-equal (u, row_a, row_b, src_a, src_b).
    union_search writes found_pos[i] for every key and tile_matches[t] for every tile -> union_fill reads the found_pos of its
    own tile and the tile_matches of its side's earlier tiles."""
    from vdetr_amd import sparse_ops as S
    tile = S.union_tile()
    na, nb = 2 * tile + 5, 2 * tile + 11
    a, b = _keys(22, na, 3 * na), _keys(23, nb, 3 * na)
    guarded.layout(front=8, unit=4)
    names = ("u", "row_a", "row_b", "src_a", "src_b")
    got, ref = _twice(monkeypatch, guarded, lambda: dict(zip(names, S.union_map(a, b))), 1)
    _bit_equal(got, ref)
    assert max(na, nb) < ref["u"].shape[0] < na + nb  # some keys are shared, some are not


def test_sp_prune_map_workspace_stays_inside_its_bytes(monkeypatch, guarded):
    """sparse_ops.prune_map, N = 2 tiles + 5 rows, about half kept.  Carved: tile_counts [3] i32.  Unit: one tile's count (one
    int); 1 workspace.  Bit-equal (kept, pos, keys_out).
    prune_count writes tile_counts[t] for every tile -> prune_fill reads the counts of the earlier tiles."""
    from vdetr_amd import sparse_ops as S
    N = 2 * S.union_tile() + 5
    keys = _keys(24, N, 4 * N)
    mask = (torch.rand(N, generator=torch.Generator().manual_seed(25)) < 0.5).to(DEV)
    guarded.layout(front=8, unit=4)
    got, ref = _twice(monkeypatch, guarded, lambda: dict(zip(("kept", "pos", "keys_out"), S.prune_map(mask, keys))), 1)
    _bit_equal(got, ref)
    assert 0 < ref["kept"].shape[0] < N


def test_sp_voxel_sites_workspace_stays_inside_its_bytes(monkeypatch, guarded):
    """sparse_ops.voxel_map_coords, N = 2 tiles + 7 points in scenes 0 and 2 (scene 1 has none), some sites hit more than once.
    Carved: tile_counts [3] i32.  Unit: one tile's count (one int); 1 workspace.  Bit-equal (sites, inverse, first, seg, order).
    voxel_heads writes tile_counts[t] for every tile -> voxel_fill reads the counts of the earlier tiles."""
    from vdetr_amd import sparse_ops as S
    N = 2 * S.voxel_tile() + 7
    g = torch.Generator().manual_seed(26)
    coords = torch.cat((torch.randint(0, 2, (N, 1), generator=g) * 2, torch.randint(-4, 4, (N, 3), generator=g) * torch.tensor([1, 1, 8])), 1)
    coords[:, 1] += torch.arange(N) // 3 % 97
    coords = coords.int().to(DEV)
    guarded.layout(front=8, unit=4)

    def run():
        vm = S.voxel_map_coords(coords)
        assert vm.num_scenes == 3
        return dict(zip(("sites", "inverse", "first", "seg", "order"), vm))

    got, ref = _twice(monkeypatch, guarded, run, 1)
    _bit_equal(got, ref)
    assert 1 < ref["sites"].shape[0] < N


@pytest.mark.parametrize("N,arm", [(64, "every consumer merges the tiles"), (49 * 32, "a launch merges the tiles")])
def test_heads_workspace_stays_inside_its_bytes(monkeypatch, guarded, N, arm):
    """vdetr_heads_fwd_f32 through the decoder's recorded heads (heads.heads_forward), B 1, G 5 (the model's five heads), dropout
    0.  N 64 is the smallest the fused launch takes with two token tiles of 32; N 1568 gives 49 tiles, one past kHdMergeAbove =
    48, where heads_merge folds the tiles between the launches (the existing tests run that arm at 4096 tokens within seconds; 49
    tiles are the cheapest that reach it).  Workspace: two tables [tiles][5 * 256][2] floats (40,960 B / 1,003,520 B); unit: one
    tile's row of one table (10,240 B); 1 workspace.
    Tolerance: that of test_gpu_heads.py::test_fused_heads_equal_the_batched_path for the same tensors (2e-5 of the tensor's
    scale for pre1 and its statistics, 5e-5 for the rest); the launches use no atomics.
    heads_l1 writes table 0, every tile and channel -> (heads_merge reads all tiles of table 0 and writes tile 0) -> heads_l2
    reads table 0 (merged: tile 0 only) and writes table 1 -> (heads_merge on table 1) -> heads_l3 reads table 1."""
    from test_gpu_heads import _close, _model
    from vdetr_amd import attention as A
    from vdetr_amd import heads as HD
    model, _flat = _model(64, 512)
    dec = model.decoder
    heads = dec.mlp_heads[1]
    names = dec._HEAD_NAMES
    for n in names:
        for i in (3, 7):
            heads[n].layers[i].p = 0.0
    g = torch.Generator().manual_seed(N)
    seq = (torch.randn((N, 1, 256), generator=g) * 1.5 + 0.2).to(DEV)
    feats = seq.permute(1, 2, 0)
    for i in (1, 5):  # (the first training-mode call lays a group's running statistics out adjacently)
        dec._bn_group(feats.repeat(1, 5, 1), [heads[n].layers[i] for n in names], True)
    state = {k: v.clone() for k, v in heads.state_dict().items()}
    assert HD.FUSED and HD.heads_usable(seq, [heads[n].layers for n in names], 18)
    guarded.layout(front=16, unit=5 * 256 * 2 * 4)

    def run():
        with torch.no_grad():
            for k, v in heads.state_dict().items():
                v.copy_(state[k])
        A.reset_rng()
        y, _, rec = dec._run_heads_recorded(heads, feats, None, seq)
        torch.cuda.synchronize()
        out = {"y": y.clone(), "h1": rec["h1"].clone(), "h2": rec["h2"].clone()}
        for tag in ("bn1", "bn2"):
            out.update({f"{tag}.pre": rec[tag][0].clone(), f"{tag}.save_mean": rec[tag][3].clone(), f"{tag}.save_invstd": rec[tag][4].clone()})
        out.update({k: v.clone() for k, v in heads.state_dict().items() if "running" in k})
        return out

    got, ref = _twice(monkeypatch, guarded, run, 1)
    assert list(got) == list(ref)
    for name, r in ref.items():
        _usable(name, r)
        _close(got[name], r, 2e-5 if name.startswith("bn1.") or ".layers.1.running" in name else 5e-5, name)


def test_add_ln_backward_workspace_stays_inside_its_bytes(monkeypatch, guarded):
    """add_ln.layer_norm backward, rows 77, C 256: 5 workgroups of 16 rows, the last with 13.  Workspace: 5 partial rows of
    [4][256] floats (20,480 B); unit: one partial row (4096 B); 1 workspace (the forward takes none).
    Tolerance: that of test_gpu_add_ln.py::test_layer_norm_matches_oracle (rtol 1e-4, atol 1e-5 of the tensor's maximum).
    add_ln_bwd writes [which][C] of its partial row for which < 2 (one output: no d_out2) -> add_ln_param_reduce reads which < 2
    of every row.  The halves [2][C], [3][C] of a row stay unwritten and unread."""
    from test_gpu_add_ln import _compare, _mods
    from vdetr_amd import add_ln as ALN
    g = torch.Generator().manual_seed(77 + 256)
    x, w = (torch.randn(77, 1, 256, generator=g) * 2 + 0.5).to(DEV), torch.randn(77, 1, 256, generator=g).to(DEV)
    guarded.layout(front=16, unit=4 * 256 * 4)

    def run():
        ln = _mods(256, 3, 1)[0].to(DEV)
        xx = x.clone().requires_grad_(True)
        out = ALN.layer_norm(xx, ln)
        (out * w).sum().backward()
        return {"out": out.detach(), "dx": xx.grad, "dgamma": ln.weight.grad, "dbeta": ln.bias.grad}

    got, ref = _twice(monkeypatch, guarded, run, 1)
    for name, r in ref.items():
        _usable(name, r)
    _compare(list(got.values()), list(ref.values()), list(ref))


def test_colsum_split_workspace_stays_inside_its_bytes(monkeypatch, guarded):
    """helpers.colsum_batched, n 2, rows 128, cols 8: the split path with S = 4 row ranges of 32 rows.  Workspace [2][4][8] floats
    (256 B); unit: one item's partial rows [4][8] (128 B); 1 workspace.  Bit-equal (fixed summation order).
    colsum4 (first launch) writes partial [item][sp][0 .. cols) for every item and split -> colsum4 (second launch) reads them
    all as n matrices of S rows."""
    from vdetr_amd import _lib as L
    from vdetr_amd.helpers import colsum_batched
    assert L.lib().vdetr_colsum_workspace_bytes(2, 128, 8) == 256 > 0  # the split path is the one under test
    x = _table(27, 2, 128, 8)
    guarded.layout(front=16, unit=4 * 8 * 4)
    got = colsum_batched(x)
    assert guarded() == 1
    assert not bool((guarded.interior(0) == 0xFF).all()), "the partials went through the workspace, not round it"
    monkeypatch.undo()
    ref = colsum_batched(x)
    assert guarded() == 1
    _bit_equal({"sums": got}, {"sums": ref})
    torch.testing.assert_close(ref, x.sum(1), rtol=1e-5, atol=1e-5)


def test_colsum_ptrs_split_workspace_stays_inside_its_bytes(monkeypatch, guarded):
    """helpers._wgrad_ptrs (the bias gradients of 8 parked linear layers, read where they are: vdetr_colsum_ptrs_f32), rows 128,
    out 8: S = 4.  Workspace [8][4][8] floats (1024 B); unit: one item's partial rows (128 B); 1 workspace.  Bit-equal.
    The two launches of the test above, with the items behind a pointer table."""
    from vdetr_amd.helpers import _wgrad_ptrs
    group = [(None, None, _table(30 + i, 128, 8), _table(40 + i, 128, 4)) for i in range(8)]
    guarded.layout(front=16, unit=4 * 8 * 4)
    got, ref = _twice(monkeypatch, guarded, lambda: {"db": _wgrad_ptrs(group, False, True)[1]}, 1)
    _bit_equal(got, ref)
    torch.testing.assert_close(ref["db"], torch.stack([it[2].sum(0) for it in group]), rtol=1e-5, atol=1e-5)


def test_pair_plan_workspace_stays_inside_its_bytes(monkeypatch, guarded):
    """sparse_ops.PairPlan on the device, K 27, nout 300, nin 300: two blocks of 256 output rows, the second with 44.  Workspace
    [27][2] ints (54 ints, 216 B), handed over as the int32 view of a byte buffer; unit: one block's column of counts (27 ints,
    108 B); 1 workspace.  Bit-equal (pin, pout, slot, islot, counts).
    sp_plan_count writes bc[k][b] for every offset and block -> sp_plan_scan reads all K * nb of them and writes their exclusive
    offsets in place -> sp_plan_fill reads bc[k][b]."""
    from vdetr_amd import _lib as L
    from vdetr_amd import sparse_ops as S
    assert L.lib().vdetr_sp_pair_plan_workspace_ints(27, 300) == 54
    g = torch.Generator().manual_seed(28)
    nbr = torch.stack([torch.where(torch.rand(300, generator=g) < 0.6, torch.randperm(300, generator=g), torch.tensor(-1)) for _ in range(27)])
    nbr = nbr.int().to(DEV)
    guarded.layout(front=16, unit=27 * 4)

    def run():
        plan = S.PairPlan(nbr, 300).finalize()
        return {"pin": plan.pin.clone(), "pout": plan.pout.clone(), "slot": plan.slot.clone(), "islot": plan.islot.clone(),
                "counts": torch.tensor(plan.counts)}

    got, ref = _twice(monkeypatch, guarded, run, 1)
    _bit_equal(got, ref)
    assert 0 < ref["pin"].shape[0] < 27 * 300


def test_loader_chain_workspaces_stay_inside_their_bytes(monkeypatch, guarded):
    """The training loader's device chain on two scenes of 300 and 130 points (tiles of 256 rows: two and a ragged one, then one),
    rows of xyz + rgb: augment_colors (drop, contrast, jitter and hue all fired) -> append_height -> crop_and_sample (8 attempts,
    64 points kept) -> prepare_scenes with the crop's choices.  4 workspaces, one per step; all carved by csrc/workspace.h
    (front 8).  Unit: the largest record of a tile over the four layouts, cuboid.hip's [8 attempts][7] ints (224 B), below the
    256 B.  Bit-equal: every output of every step (the chain is IEEE operations in a stated order, ordinary stores).
    color_aug.hip  color_bounds writes bounds[tile] -> color_scale reads them, writes scene[b] -> color_apply reads scene[b]
    (height)       per pass of 8 bits: height_hist writes partial[tile] (the first pass reads no state) -> height_pick reads the
                   partials of its scene and writes state[b] (the first pass without reading it) -> height_write reads state[b]
    cuboid.hip     cuboid_bounds writes bounds[tile] -> cuboid_boxes reads them, writes crop[b][attempt] for every attempt ->
                   cuboid_count reads crop, writes stats[tile][attempt] -> cuboid_select reads the stats of its scene, writes
                   tile_base[tile] -> cuboid_compact reads crop and tile_base
    scene_prep.hip scene_prep_points writes 6 floats per tile of kept rows -> scene_prep_targets reads them (the same workspace)"""
    from test_gpu_scene_prep import random_case
    from vdetr_amd import scene_prep as SP
    c, pose = random_case(29, (300, 130), 3, (2, 3), C=3)
    c["points"][:, 3:] = np.round(c["points"][:, 3:].clip(1, 254))
    off = c["offsets"]
    pts = torch.from_numpy(c["points"]).to(DEV)
    boxes, counts, classes = (torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ("boxes", "box_counts", "box_classes"))
    from helpers import cfg

    def run():
        rs = [np.random.RandomState(50 + b) for b in range(2)]
        params = [SP.draw_color_augment(n, r, color_drop=0.1, color_contrastp=1.0, color_jitterp=1.0, hue_sat="0.5_0.2_1.0")
                  for n, r in zip((300, 130), rs)]
        assert all(p.keep is not None and p.blend is not None and p.noise is not None and p.hue_val is not None for p in params)
        coloured = SP.augment_colors(pts, off, params)
        tall = SP.append_height(coloured, off)
        crop = SP.crop_and_sample(tall, off, boxes, counts, classes, rs, 64, min_points=20, max_trials=8)
        fin = SP.prepare_scenes(tall, off, crop["boxes"].float(), crop["box_counts"], crop["box_classes"], pose, cfg(),
                                choices=crop["choices"], color_mean=-1.0)
        out = {"coloured": coloured, "tall": tall, "choices": crop["choices"], "crop boxes": crop["boxes"],
               "trial + 2": torch.from_numpy(crop["trial"] + 2), "kept_points": torch.from_numpy(crop["kept_points"]),
               "kept_rows": torch.cat(crop["kept_rows"]), "out_points": torch.cat(fin["point_clouds"])}
        out.update({k: v for k, v in fin.items() if k in ("point_cloud_dims_min", "point_cloud_dims_max", "gt_box_corners",
                                                           "gt_box_centers", "gt_box_sizes", "gt_box_present")})
        return out

    got, ref = _twice(monkeypatch, guarded, run, 4)
    _bit_equal(got, ref)
    assert ref["tall"].shape == (430, 7) and ref["out_points"].shape == (128, 7)


def test_vertex_normals_workspace_stays_inside_its_bytes(monkeypatch, guarded):
    """scene_prep.vertex_normals on the ragged batch of test_gpu_normals.py::test_ragged_batch_equals_the_single_calls (the
    fixture's `isolated`, a lone vertex without a face, `fan`, `grid`): the meshes its existing tests use at their smallest, as four
    scenes.  Carved (front 8): w [F][3] f32, count / start / cursor [N] i32 each, tile_sum [tiles] i32, adj [F][3] i32.  Unit:
    one face's record (12 B), below the 256 B; 1 workspace.  Bit-equal.
    normals_clear writes count[v] = 0 for every vertex -> normals_face writes w[f] for every face and adds to count ->
    normals_tile_sum reads count, writes tile_sum[t] -> normals_top_scan scans tile_sum in place -> normals_starts reads both,
    writes start[v] and cursor[v] -> normals_fill takes slots from cursor and writes adj[slot] -> normals_vertex reads count,
    start, the count[v] entries of adj behind start[v], and w of those faces."""
    from helpers import dev
    from test_gpu_normals import batch_of
    from test_normals_restatement import golden
    from vdetr_amd.scene_prep import vertex_normals
    g = golden()
    lonely = (np.array([[0.5, -1.0, 2.0]], np.float32), np.zeros((0, 3), np.int32))
    meshes = [(g["isolated"]["ply_vertices"][:, :3], g["isolated"]["faces"]), lonely, (g["fan"]["ply_vertices"][:, :3], g["fan"]["faces"]),
              (g["grid"]["ply_vertices"][:, :3], g["grid"]["faces"])]
    verts, voff, faces, foff = batch_of(meshes)
    vd = dev(verts)
    guarded.layout(front=8, unit=12)
    got, ref = _twice(monkeypatch, guarded, lambda: {"normals": vertex_normals(vd, voff, faces, foff)}, 1)
    _bit_equal(got, ref)


def test_scan_export_workspace_stays_inside_its_bytes(monkeypatch, guarded):
    """scan_export.export_scans on two scans built as test_gpu_scan_export.py's ragged batch builds its smaller ones: 1200
    vertices with 7 objects (tiles of 512 rows: two and a ragged one) and 333 vertices without any, so Kmax is 7; five label
    ids dropped, which brings the compaction and its two regions in.  Carved (front 8): partial [4 tiles][7][6] u32, tile_kept
    [4] and tile_base [4] i32.  Unit: one tile's partial (168 B), below the 256 B; 1 workspace.  Bit-equal (no tolerance there
    either).
    scan_export_points writes partial[tile][k < the scene's objects] and tile_kept[tile] -> scan_export_boxes reads the
    partials of its scene's objects, scans tile_kept into tile_base -> scan_export_compact reads tile_base."""
    from test_gpu_scan_export import export
    from test_scan_export_restatement import make_scan
    rng = np.random.default_rng(33)
    scans = [make_scan(rng, 1200, 7, cover=0.6), make_scan(rng, 333, 0, cover=0.0)]
    guarded.layout(front=8, unit=7 * 6 * 4)

    def run():
        out = export(scans, (1, 2, 5, 7, 40))
        return {k: (torch.from_numpy(np.asarray(v)) if not torch.is_tensor(v) else v) for k, v in out.items()
                if k in ("offsets", "mesh_vertices", "semantic_labels", "instance_labels", "instance_bboxes", "boxes", "box_counts")}

    got, ref = _twice(monkeypatch, guarded, run, 1)
    _bit_equal(got, ref)
    assert ref["instance_bboxes"].shape == (2, 7, 7) and int(ref["box_counts"][1]) == 0
