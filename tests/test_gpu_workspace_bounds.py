"""The workspace layouts of nms.hip, fps.hip, attn_fwd.hip, attn_bwd.hip and attn_bwd_kv.hip on a buffer that is NOT 256-B
aligned and has not one byte to spare.

Every workspace the package hands to the library comes from torch's allocator and starts on a multiple of 256 B, so neither the
rounding of the start nor the 256 B the size functions add for it is exercised anywhere else.  Here `_lib.workspace` is replaced:
a request of n bytes gets an allocation of n + 8 + 256 bytes filled with 0xA5 and the n-byte view that starts 8 bytes in.  After
the op the 8 bytes in front and the 256 behind must still read 0xA5, and the results must be those of the ordinary workspace.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_attention import _scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 0xA5


@pytest.fixture
def guarded(monkeypatch):
    """replaces _lib.workspace as described above; the returned function checks the guard bytes of every workspace handed out
    since, and answers how many there were"""
    from vdetr_amd import _lib
    made = []

    def workspace(nbytes, device):
        n = max(int(nbytes), 1)
        raw = torch.full((n + 8 + 256,), GUARD, dtype=torch.uint8, device=device)
        made.append((raw, n))
        return raw[8:8 + n]

    def check():
        torch.cuda.synchronize()
        for raw, n in made:
            assert raw[8:].data_ptr() % 256 == 8, "the view is meant to be off the 256-B grid"
            assert bool((raw[:8] == GUARD).all()), f"bytes in front of a workspace of {n} B were written"
            assert bool((raw[8 + n:] == GUARD).all()), f"bytes behind a workspace of {n} B were written"
        return len(made)

    monkeypatch.setattr(_lib, "workspace", workspace)
    return check


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
