"""The eval forward under no_grad (the reference's evaluate() / --test_only): a stage's heads as ONE launch
(vdetr_heads_infer_f32), the position MLP with its running statistics (vdetr_pos_mlp_infer_f32 / vdetr_rb_qkv_pos_infer_f32), the
GenericMLPs as GEMM + the eval form of bn_act — against torch's modules in fp64, against the paths the eval forward took before
(heads.INFER = False), bit for bit against itself, after optimiser steps, and as a captured graph."""
import copy

import numpy as np
import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _close(a, b, tol, what):
    scale = float(b.abs().max()) + 1e-20
    err = float((a.double() - b.double()).abs().max())
    assert err <= tol * scale, f"{what}: max |diff| {err:.3e} vs scale {scale:.3e}"


def _stage_model(rotated):
    from test_gpu_heads import _model
    return _model(64, 512, angle_type="object_coords" if rotated else "")


def _perturb_bn(mods, g):
    """running statistics, gammas, betas that are not the initial 0 / 1 / 1 / 0"""
    with torch.no_grad():
        for bn in mods:
            bn.running_mean.copy_(torch.randn(bn.num_features, generator=g) * 0.5)
            bn.running_var.copy_(torch.rand(bn.num_features, generator=g) * 2 + 0.2)
            bn.weight.copy_(torch.rand(bn.num_features, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(bn.num_features, generator=g) * 0.3)


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("B,N", [(1, 1024), (1, 4096), (2, 512)])
def test_heads_infer_vs_fp64_modules(rotated, B, N):
    """vdetr_heads_infer_f32 (16- and 32-token tiles and the library's choice) against a .double().eval() copy of the stage's five
    GenericMLPs; the ScanNet rows and the rotated dataset's; two runs bit-identical"""
    from vdetr_amd import heads as HD
    model, _flat = _stage_model(rotated)
    dec = model.decoder
    heads = dec.mlp_heads[2]
    names = dec._HEAD_NAMES
    L = dec._head_layers(2)
    g = torch.Generator().manual_seed(N + B + rotated)
    _perturb_bn([l[i] for l in L for i in (1, 5)], g)
    with torch.no_grad():
        for l in L:
            l[8].bias.copy_(torch.randn(l[8].bias.shape, generator=g) * 0.5)
            l[8].weight.add_((torch.randn(l[8].weight.shape, generator=g) * 0.05).to(DEV))
    heads.eval()
    seq = (torch.randn((N, B, 256), generator=g) * 1.5 + 0.2).to(DEV)
    outs = [l[8].weight.shape[0] for l in L]
    rows = max(outs)
    assert rows == (12 if rotated else 18) and HD.heads_infer_usable(seq, L, rows)  # (ScanNet: 18 classes; rotated: 12 angle bins)
    ref = copy.deepcopy(heads).double().eval()
    with torch.no_grad():
        want = {n: ref[n](seq.permute(1, 2, 0).double()) for n in names}
        for tile in (16, 32, 0):
            HD.INFER_TILE = tile
            try:
                y = HD.heads_infer(seq, L, rows)
                y2 = HD.heads_infer(seq, L, rows)
            finally:
                HD.INFER_TILE = 0
            torch.cuda.synchronize()
            assert y.shape == (B, 5, rows, N)
            assert torch.equal(y, y2), f"tile {tile}: two runs differ"
            for gi, n in enumerate(names):
                _close(y[:, gi, :outs[gi]], want[n], 2e-5, f"tile {tile} {n}")


def test_heads_shapes_outside_the_constraints_fall_back_and_match():
    """token counts that are no multiple of 16 and non-contiguous features take the ATen path; it still matches the modules"""
    from vdetr_amd import heads as HD
    model, _flat = _stage_model(False)
    dec = model.decoder.eval()
    heads = dec.mlp_heads[1]
    L = dec._head_layers(1)
    g = torch.Generator().manual_seed(5)
    _perturb_bn([l[i] for l in L for i in (1, 5)], g)
    ref = copy.deepcopy(heads).double().eval()
    for seq in (torch.randn((40, 1, 256), generator=g).to(DEV), torch.randn((2, 64, 256), generator=g).to(DEV).transpose(0, 1)):
        assert not HD.heads_infer_usable(seq, L, 18)
        with torch.no_grad():
            raw = dec._run_heads(heads, seq.permute(1, 2, 0))
            want = {n: ref[n](seq.permute(1, 2, 0).double()) for n in dec._HEAD_NAMES}
        if "_joint" in raw:
            y, chans = raw["_joint"]
            got = {n: y[:, gi, :chans[gi]] for gi, n in enumerate(dec._HEAD_NAMES)}
        else:
            got = raw
        for n in dec._HEAD_NAMES:
            _close(got[n], want[n], 2e-5, n)


def _pos_module(seed):
    from vdetr_amd.helpers import PositionEmbeddingLearned
    torch.manual_seed(seed)
    mod = PositionEmbeddingLearned(6, 256).to(DEV)
    g = torch.Generator().manual_seed(seed)
    _perturb_bn([mod.position_embedding_head[1]], g)
    with torch.no_grad():
        if mod.position_embedding_head[0].bias is not None:
            mod.position_embedding_head[0].bias.copy_(torch.randn(256, generator=g) * 0.2)
    return mod.eval()


def _boxes(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat((torch.rand((B, N, 3), generator=g) * torch.tensor([8.0, 6.0, 0.5]) + 1.0,
                      torch.rand((B, N, 3), generator=g) + 0.1), -1).to(DEV)


@pytest.mark.parametrize("B,N", [(1, 1024), (4, 1024), (2, 48)])
def test_pos_mlp_infer_vs_fp64_module(B, N, monkeypatch):
    """vdetr_pos_mlp_infer_f32, at once and left to a consumer (heads.lazy_pos + materialize_pos), against the fp64 module in eval
    mode; the running statistics are read, not updated"""
    from vdetr_amd import heads as HD
    mod = _pos_module(B * 10 + N)
    xyz = _boxes(B, N, N)
    ref = copy.deepcopy(mod).double().cpu().eval()
    bn = mod.position_embedding_head[1]
    stats = (bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone())
    calls = []
    real = HD.pos_mlp_infer
    monkeypatch.setattr(HD, "pos_mlp_infer", lambda *a: calls.append(1) or real(*a))
    with torch.no_grad():
        want = ref(xyz.double().cpu())
        out = mod(xyz)
        prev = HD.lazy_pos(True)
        try:
            lazy = mod(xyz)
        finally:
            HD.lazy_pos(prev)
        assert HD._pending_pos
        HD.materialize_pos(lazy.permute(2, 0, 1))
    assert not HD._pending_pos and len(calls) == 2
    torch.cuda.synchronize()
    _close(out.cpu(), want, 2e-5, "out")
    assert torch.equal(out, lazy)
    assert torch.equal(bn.running_mean, stats[0]) and torch.equal(bn.running_var, stats[1]) and torch.equal(bn.num_batches_tracked, stats[2])


@pytest.mark.parametrize("B,nQ,nK", [(1, 64, 256), (1, 1024, 512), (2, 48, 130)])
def test_rb_qkv_pos_infer_vs_own_launch_and_fp64(monkeypatch, B, nQ, nK):
    """a decoder layer in eval mode under no_grad whose query position is computed by its q / k / v launch
    (vdetr_rb_qkv_pos_infer_f32) against the same layer behind the position MLP's own inference launch, and the position against
    the fp64 module"""
    from test_gpu_rowblock import _layer, _scene
    from vdetr_amd import heads as HD
    from vdetr_amd import rowblock as RB
    from vdetr_amd import vdetr_transformer as T
    monkeypatch.setattr(T, "_ROWBLOCK", True)
    layer = _layer(7).eval()
    posm = _pos_module(11)
    ref = copy.deepcopy(posm).double().cpu().eval()
    out_norm = torch.nn.LayerNorm(256).to(DEV)
    g = torch.Generator().manual_seed(B * 77 + nQ)
    tgt = torch.randn((nQ, B, 256), generator=g).to(DEV)
    mem = torch.randn((nK, B, 256), generator=g).to(DEV)
    boxes = _boxes(B, nQ, nQ + 1)
    xyz, verts = _scene(B, nQ, nK, 12)
    launches = []
    real = HD.take_pending_pos
    monkeypatch.setattr(HD, "take_pending_pos", lambda pos: launches.append(real(pos)) or launches[-1])
    assert RB.usable(layer, tgt, None, ())

    def run(lazy):
        with torch.no_grad():
            prev = HD.lazy_pos(lazy)
            try:
                pos = posm(boxes).permute(2, 0, 1)
            finally:
                HD.lazy_pos(prev)
            assert bool(HD._pending_pos) == lazy
            layer.post_norms = (out_norm,)
            layer.pre_normed = None
            out, _ = layer(tgt, mem, verts, None, xyz, None, query_pos=pos)
            (o1,) = layer.post_normed
            layer.post_norms = layer.post_normed = None
            assert not HD._pending_pos
        return out, o1, pos.clone()

    a = run(False)
    b = run(True)
    assert [r is not None and r[2] for r in launches] == [False, True], launches
    for n, x, y in zip(("out", "norm(out)", "query_pos"), b, a):
        _close(x, y, 2e-5, n)
    with torch.no_grad():
        want = ref(boxes.double().cpu()).permute(2, 0, 1)
    _close(b[2].cpu(), want, 2e-5, "query_pos vs fp64")


def _c1_model(rotated=False):
    from test_gpu_model import _make_model
    return _make_model(nq=64, npre=512, angle_type="object_coords" if rotated else "").to(DEV)


def test_routing_one_heads_launch_per_stage(monkeypatch):
    """model.eval() + no_grad: one heads_infer launch per stage (the proposals on the encoder tokens included), the ATen heads path
    never; with autograd on, eval mode does not take the inference launch at all"""
    from test_gpu_model import _inputs
    from vdetr_amd import heads as HD
    from vdetr_amd import vdetr_transformer as T
    model = _c1_model().eval()
    inp = _inputs(6000, 5, DEV)
    calls = {"infer": 0, "aten": 0}
    real_infer, real_aten = HD.heads_infer, T.TransformerDecoder._run_heads

    def infer(*a):
        calls["infer"] += 1
        return real_infer(*a)

    def aten(self, *a):
        calls["aten"] += 1
        return real_aten(self, *a)

    monkeypatch.setattr(HD, "heads_infer", infer)
    monkeypatch.setattr(T.TransformerDecoder, "_run_heads", aten)
    with torch.no_grad():
        model(inp)
    assert calls == {"infer": len(model.decoder.mlp_heads), "aten": 0}, calls
    assert len(model.decoder.mlp_heads) == len(model.decoder.layers) + 1
    calls.update(infer=0, aten=0)
    with torch.inference_mode():
        model(inp)
    assert calls == {"infer": len(model.decoder.mlp_heads), "aten": 0}, calls
    calls.update(infer=0, aten=0)
    out = model(inp)  # eval mode WITH autograd: today's path
    assert calls["infer"] == 0 and calls["aten"] == len(model.decoder.mlp_heads), calls
    out["outputs"]["sem_cls_logits"].sum().backward()


def _tensors(out):
    stages = [("outputs", out["outputs"])] + [(f"aux{i}", o) for i, o in enumerate(out["aux_outputs"])]
    return {f"{s}.{k}": v for s, o in stages for k, v in o.items() if torch.is_tensor(v) and v.is_floating_point()}


def _stages(out):
    return out["aux_outputs"] + [out["outputs"]]


def _compare(a, b, what):
    """every floating tensor of every stage within test_gpu_model.py's tolerance, except the queries that two fp32 evaluation
    orders legitimately send elsewhere: a proposal whose stage-0 objectness is within rounding of the top-k boundary (its query
    carries another proposal, seen in pre_box_center_unnormalized) and an angle bin whose two largest logits are within rounding
    (angle_continuous and the rotated corners follow the arg-max).  Those are a handful of a scene's 1024 queries."""
    sa, sb = _stages(a), _stages(b)
    assert len(sa) == len(sb)
    for s, (x, y) in enumerate(zip(sa, sb)):
        B, Q = y["center_unnormalized"].shape[:2]
        moved = (x["pre_box_center_unnormalized"] - y["pre_box_center_unnormalized"]).abs().amax(-1) > 1e-4
        flip = x["angle_logits"].argmax(-1) != y["angle_logits"].argmax(-1)
        assert int(moved.sum()) <= 4 * B and int(flip.sum()) <= max(4, Q * B // 500), (what, s, int(moved.sum()), int(flip.sum()))
        keep = ~moved
        keep_angle = keep & ~flip
        n = 0
        for k, t in y.items():
            if not (torch.is_tensor(t) and t.is_floating_point()) or k.startswith("_"):
                continue
            m = keep_angle if k in ("angle_continuous", "box_corners") else keep
            ref = t[m].detach().cpu().double().numpy()
            assert_close(x[k][m], ref, 1e-3, 2e-4 * max(1.0, float(np.abs(ref).max())), f"{what} stage {s} {k}")
            n += 1
        assert n >= 10


def _eval_forward(model, inp, infer, monkeypatch):
    from vdetr_amd import heads as HD
    monkeypatch.setattr(HD, "INFER", infer)
    with torch.no_grad():
        out = model(inp)
    torch.cuda.synchronize()
    return out


def _bench_model(cfg):
    import bench
    from vdetr_amd.dist import FlatParams
    model = bench.build_model(cfg, torch.device(DEV))
    flat = FlatParams([p for p in model.parameters() if p.requires_grad], groups=model.flat_param_groups())
    inp = bench.make_inputs(cfg, torch.device(DEV), 0)
    inp["fps_inds"] = model.sample_indices(inp)
    return model, flat, inp


@pytest.mark.parametrize("cfg", ["c2", "c5"])
def test_whole_model_eval_forward_vs_fallback(cfg, monkeypatch):
    """the C2-shaped model and the rotated C5 cut (bench.py's configurations): the eval forward's fast path against heads.INFER =
    False on every tensor of outputs and aux_outputs; the same forward twice is bit-identical"""
    model, _flat, inp = _bench_model(cfg)
    model.eval()
    ref = _eval_forward(model, inp, False, monkeypatch)
    got = _eval_forward(model, inp, True, monkeypatch)
    again = _eval_forward(model, inp, True, monkeypatch)
    _compare(got, ref, cfg)
    ta, tb = _tensors(got), _tensors(again)
    for k in ta:
        assert torch.equal(ta[k], tb[k]), f"{k}: two runs differ"


def test_eval_after_optimizer_steps_reads_the_updated_weights(monkeypatch):
    """a few ClipAdamW training steps, then the eval forward: equal to the fallback on the updated weights (a stale W^T image would
    give the old weights' result without an error)"""
    import bench
    from vdetr_amd.optim import ClipAdamW
    model, flat, inp = _bench_model("c1")
    opt = ClipAdamW(flat, lr=1e-3, weight_decay=0.1, max_norm=0.1)
    model.eval()
    before = _eval_forward(model, inp, True, monkeypatch)
    model.train()
    for _ in range(3):
        flat.grad.zero_()
        bench.loss_fn(model(inp)).backward()
        opt.step()
    model.eval()
    got = _eval_forward(model, inp, True, monkeypatch)
    ref = _eval_forward(model, inp, False, monkeypatch)
    _compare(got, ref, "after 3 steps")
    moved = max(float((a - b).abs().max()) for a, b in zip(_tensors(got).values(), _tensors(before).values()))
    assert moved > 1e-4, "the optimiser steps did not change the eval outputs"


def test_captured_eval_forward_replays_bit_identically(monkeypatch):
    """with precomputed fps_inds the eval forward captures in a torch.cuda.graph; two replays equal the eager call bit for bit"""
    from vdetr_amd import heads as HD
    monkeypatch.setattr(HD, "INFER", True)
    model, _flat, inp = _bench_model("c1")
    model.eval()
    with torch.no_grad():
        eager = _tensors(model(inp))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            model(inp)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(inp)
        captured = _tensors(out)
        for _ in range(2):
            for t in captured.values():
                t.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            for k in eager:
                assert torch.equal(captured[k], eager[k]), f"{k}: replay differs from the eager forward"
