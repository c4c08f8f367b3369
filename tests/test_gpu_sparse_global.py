"""Global pooling, broadcast and the squeeze-excite blocks on the GPU (csrc/sparse_global.hip through sparse_ops, the Minkowski*
modules and modules/senet.py) against the float64 restatement of tests/sparse_global_restatement.py.

Sums and averages (pooling y; dg of every broadcast mode; everything behind the SE gate) go under the rule of tests/norm_cases.py
(imported, not restated): FACTOR x the error of the float32 restatements over its summation orders + FACTOR x ulp32.  What is one
rounding is held to equality with the float32 restatement: max values and rows, the pooling dx of every mode, broadcast y and dx.
The fused inference form and the composition both meet the rule; behind the gate, multiply, residual add and ReLU are one rounding
each of the gate's value, so the two forms agree within the gate's tolerance times |x| — not bit for bit."""
import numpy as np
import pytest
import torch

import norm_cases as NC
import sparse_global_restatement as G
import sparse_modules_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL_CASES = G.CASES + G.CHUNK_CASES


@pytest.fixture(scope="module", autouse=True)
def chunk_case():
    """the case whose scene sizes come from the kernel's own chunk-row function"""
    from vdetr_amd import sparse_ops as S
    sizes = G.chunk_sizes(S.global_chunk_rows)
    r = S.global_chunk_rows(sum(sizes))
    assert -(-sizes[0] // r) >= 3 and sizes[1] % r == 0 and sizes[2] == r + 1
    G.set_chunk_sizes(sizes)


def _segments(sizes):
    return torch.tensor(np.concatenate(([0], np.cumsum(sizes))), dtype=torch.int32).to(DEV)


def _starts(sizes):
    return np.concatenate(([0], np.cumsum(sizes)))[:-1]


def _pool_run(x, sizes, mode, dy):
    from vdetr_amd import sparse_ops as S
    xd = x.to(DEV).requires_grad_(True)
    y, arg = S.global_pool(xd, _segments(sizes), len(sizes), mode, return_arg=True)
    assert (arg is None) == (mode != "max") and not (arg is not None and arg.requires_grad)
    y.backward(dy.to(DEV))
    out = {"y": y.detach().cpu(), "dx": xd.grad.cpu()}
    if arg is not None:
        assert arg.dtype == torch.int32
        out["arg"] = arg.cpu()
    return out


@pytest.mark.parametrize("mode", G.POOL_MODES)
@pytest.mark.parametrize("scenes,C", ALL_CASES)
def test_global_pool_forward_backward(scenes, C, mode):
    c = G.case(scenes, C)
    sizes, dy = c["sizes"], c["dy_pool"]
    x = c["x_max"] if mode == "max" else c["x"]
    got = _pool_run(x, sizes, mode, dy)
    r32 = G.pool_eval(x, sizes, mode, dy, dtype=G.F32)
    if mode == "max":
        assert G.same(got["y"], r32["y"]) and G.same(got["arg"], r32["arg"])
        first = torch.tensor([a if n else -1 for a, n in zip(_starts(sizes), sizes)])
        assert torch.equal(got["arg"][:, 1].long(), first), "a column of -inf ends at the scene's first row"
    else:
        ref = G.pool_eval(x, sizes, mode, dy)
        rests = [G.pool_eval(x, sizes, mode, dy, dtype=G.F32, order=o) for o in NC.ORDERS]
        figures = NC.compare(got, ref, rests, ("y",), label=f"{scenes} C={C} {mode}")
        print(scenes, C, mode, {k: f"{v[0]:.2e} (restatement {v[1]:.2e}, factor {v[2]:.2f})" for k, v in figures.items()})
    assert G.same(got["dx"], r32["dx"]), "dx is one rounding"
    for s, (a, n) in enumerate(zip(_starts(sizes), sizes)):
        if n == 0:
            assert bool((got["y"][s] == 0).all()) and (mode != "max" or bool((got["arg"][s] == -1).all()))
        if n == 1:
            assert G.same(got["y"][s], x[a]), "a scene of one row gives the row"
    again = _pool_run(x, sizes, mode, dy)
    assert all(G.same(got[k], again[k]) for k in got), "two runs must agree bit for bit"


def _bcast_run(x, g, sizes, mode, dy, grad_x=True, grad_g=True):
    from vdetr_amd import sparse_ops as S
    xd, gd = x.to(DEV).requires_grad_(grad_x), g.to(DEV).requires_grad_(grad_g)
    y = S.broadcast(xd, gd, _segments(sizes), len(sizes), mode)
    y.backward(dy.to(DEV))
    return {"y": y.detach().cpu(), "dx": None if xd.grad is None else xd.grad.cpu(), "dg": None if gd.grad is None else gd.grad.cpu()}


@pytest.mark.parametrize("mode", G.BCAST_MODES)
@pytest.mark.parametrize("scenes,C", ALL_CASES)
def test_broadcast_forward_backward(scenes, C, mode):
    c = G.case(scenes, C)
    sizes = c["sizes"]
    g, dy = (c["g_cat"], c["dy_cat"]) if mode == "cat" else (c["g"], c["dy"])
    got = _bcast_run(c["x"], g, sizes, mode, dy)
    ref = G.broadcast_eval(c["x"], g, sizes, mode, dy)
    rests = [G.broadcast_eval(c["x"], g, sizes, mode, dy, dtype=G.F32, order=o) for o in NC.ORDERS]
    assert torch.equal(got["y"], rests[0]["y"].float()) and torch.equal(got["dx"], rests[0]["dx"].float()), "y and dx are one rounding"
    figures = NC.compare(got, ref, rests, ("dg",), label=f"{scenes} C={C} {mode}")
    print(scenes, C, mode, {k: f"{v[0]:.2e} (restatement {v[1]:.2e}, factor {v[2]:.2f})" for k, v in figures.items()})
    for s, n in enumerate(sizes):
        if n == 0:
            assert bool((got["dg"][s] == 0).all()), "the row of a scene without rows gets an exact zero"
    again = _bcast_run(c["x"], g, sizes, mode, dy)
    assert all(torch.equal(got[k], again[k]) for k in got), "two runs must agree bit for bit"


@pytest.mark.parametrize("mode", G.BCAST_MODES)
def test_broadcast_halves(mode):
    """needs_input_grad per input: either half alone gives what both give"""
    c = G.case("single", 20)
    g, dy = (c["g_cat"], c["dy_cat"]) if mode == "cat" else (c["g"], c["dy"])
    both = _bcast_run(c["x"], g, c["sizes"], mode, dy)
    only_x = _bcast_run(c["x"], g, c["sizes"], mode, dy, grad_g=False)
    only_g = _bcast_run(c["x"], g, c["sizes"], mode, dy, grad_x=False)
    assert only_x["dg"] is None and only_g["dx"] is None
    assert torch.equal(only_x["dx"], both["dx"]) and torch.equal(only_g["dg"], both["dg"])


def test_arguments_are_checked():
    from vdetr_amd import sparse_ops as S
    x = torch.zeros((10, 8), device=DEV)
    g = torch.zeros((1, 8), device=DEV)
    seg = torch.tensor([0, 10], dtype=torch.int32, device=DEV)
    for call in (lambda t, sg, n: S.global_pool(t, sg, n, "sum"), lambda t, sg, n: S.broadcast(t, g[:, :t.shape[1]].contiguous(), sg, n, "add"),
                 lambda t, sg, n: S.se_scale(t, sg, n, torch.zeros((2, t.shape[1]), device=DEV), None,
                                             torch.zeros((t.shape[1], 2), device=DEV), None)):
        for bad in ((x.cpu(), seg, 1), (x.double(), seg, 1), (x[:, ::2], seg, 1), (x, seg, 2), (x, seg.long(), 1), (x, seg.cpu(), 1)):
            with pytest.raises(RuntimeError):
                call(*bad)
        with pytest.raises(RuntimeError, match="=6"):
            call(torch.zeros((10, 6), device=DEV), seg, 1)
    with pytest.raises(ValueError, match="median"):
        S.global_pool(x, seg, 1, "median")
    with pytest.raises(ValueError, match="sub"):
        S.broadcast(x, g, seg, 1, "sub")
    with pytest.raises(RuntimeError, match=r"\(1, 12\)"):
        S.broadcast(x, torch.zeros((1, 12), device=DEV), seg, 1, "mul")
    with pytest.raises(RuntimeError, match=r"\(2, 8\)"):
        S.broadcast(x, torch.zeros((2, 8), device=DEV), seg, 1, "add")
    empty, seg0 = torch.zeros((0, 8), device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    y, arg = S.global_pool(empty, seg0, 1, "max", return_arg=True)
    assert y.shape == (1, 8) and bool((y == 0).all()) and bool((arg == -1).all())
    assert S.broadcast(empty, g, seg0, 1, "cat").shape == (0, 16)


# ---- modules ---------------------------------------------------------------------------------------------------------------------
def _sites(sizes, batch_ids):
    rng = np.random.default_rng(sum(sizes))
    coords = []
    for b, n in zip(batch_ids, sizes):
        cells = rng.choice(20 ** 3, size=n, replace=False)
        coords.append(np.stack((np.full(n, b), cells // 400 - 10, (cells // 20) % 20 - 10, cells % 20 - 10), 1))
    return R.sort_sites(np.concatenate(coords))


def _tensor(feats, sites):
    """(SparseTensor on the sorted sites with `feats` as its leaf table, the leaf)"""
    from vdetr_amd import minkowski as ME
    leaf = feats.to(DEV).requires_grad_(True)
    cm = ME.SparseTensor(leaf.detach(), torch.from_numpy(sites).int().to(DEV)).coordinate_manager
    return ME.SparseTensor(leaf, coordinate_manager=cm, tensor_stride=1), leaf


def test_state_dict_keys():
    from vdetr_amd.modules import senet
    se = ["fc.0.linear.weight", "fc.0.linear.bias", "fc.2.linear.weight", "fc.2.linear.bias"]
    assert list(senet.SELayer(32, reduction=4).state_dict()) == se
    bn = lambda p: [f"{p}.bn.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]  # noqa: E731
    assert list(senet.SEBasicBlock(32, 32, reduction=4).state_dict()) == \
        ["conv1.kernel"] + bn("norm1") + ["conv2.kernel"] + bn("norm2") + ["se." + k for k in se]
    keys = list(senet.SEBottleneckIN(16, 8).state_dict())
    assert keys[-4:] == ["se." + k for k in se] and "norm3.weight" in keys
    assert senet.SEBottleneck(16, 8).se.fc[0].linear.in_features == 32 and senet.SEBasicBlockINBN(16, 16).se.fc[0].linear.out_features == 1


def test_origin_tensor_of_a_batch_with_an_absent_scene():
    from vdetr_amd import minkowski as ME
    sizes, C = (120, 75), 20
    sites = _sites(sizes, (0, 2))
    feats = torch.randn(len(sites), C, generator=torch.Generator().manual_seed(4))
    x, leaf = _tensor(feats, sites)
    full = (120, 0, 75)
    for cls, mode in ((ME.MinkowskiGlobalSumPooling, "sum"), (ME.MinkowskiGlobalAvgPooling, "avg"), (ME.MinkowskiGlobalMaxPooling, "max"),
                      (ME.MinkowskiGlobalPooling, "avg")):
        out = cls()(x)
        assert out.tensor_stride == 0 and out.coordinate_manager is x.coordinate_manager and out.F.shape == (3, C)
        assert out.C.cpu().tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0]]
        dyp = torch.randn(3, C, generator=torch.Generator().manual_seed(6))
        leaf.grad = None
        out.F.backward(dyp.to(DEV))
        r32 = G.pool_eval(feats, full, mode, dyp, dtype=G.F32)
        assert bool((out.F[1] == 0).all()) and G.same(leaf.grad.cpu(), r32["dx"])
        if mode == "max":
            assert G.same(out.F.detach().cpu(), r32["y"])
        parts = out.decomposed()
        assert len(parts) == 3 and all(f.shape == (1, C) and c.shape == (1, 3) for c, f in parts)
    lin = ME.MinkowskiLinear(C, 8).to(DEV)
    assert list(lin.state_dict()) == ["linear.weight", "linear.bias"]
    y = ME.MinkowskiSigmoid()(lin(out))
    assert y.tensor_stride == 0 and y.keys is out.keys and torch.equal(y.F, torch.sigmoid(lin.linear(out.F)))
    assert lin(x).F.shape == (len(sites), 8) and lin(x).tensor_stride == 1


def test_modules_refuse_what_they_cannot_combine():
    from vdetr_amd import minkowski as ME
    sites = _sites((60, 40), (0, 1))
    x, _ = _tensor(torch.randn(len(sites), 8), sites)
    other, _ = _tensor(torch.randn(len(sites), 8), sites)
    cm = x.coordinate_manager
    pooled = ME.MinkowskiGlobalAvgPooling()(x)
    mul, add, cat = ME.MinkowskiBroadcastMultiplication(), ME.MinkowskiBroadcastAddition(), ME.MinkowskiBroadcastConcatenation()
    with pytest.raises(ValueError, match="tensor_stride 1"):
        mul(x, x)
    with pytest.raises(ValueError, match="coordinate manager"):
        mul(x, ME.MinkowskiGlobalAvgPooling()(other))
    short = ME.SparseTensor(pooled.F[:1], tensor_stride=0, coordinate_manager=cm, keys=cm.origin_keys()[:1])
    with pytest.raises(ValueError, match="1 rows.*2 scenes"):
        add(x, short)
    wide = ME.SparseTensor(torch.zeros((2, 12), device=DEV), tensor_stride=0, coordinate_manager=cm, keys=cm.origin_keys())
    for op in (mul, add):
        with pytest.raises(ValueError, match="8 channels.*12"):
            op(x, wide)
    assert cat(x, wide).F.shape == (len(sites), 20) and cat(x, wide).tensor_stride == 1 and cat(x, wide).keys is x.keys
    with pytest.raises(NotImplementedError):
        ME.MinkowskiBroadcast()(x, pooled)
    for layer in (ME.MinkowskiConvolution(8, 8, kernel_size=3, dimension=3).to(DEV), ME.MinkowskiAvgPooling(2, 2),
                  ME.MinkowskiConvolutionTranspose(8, 8, kernel_size=2, stride=2, dimension=3).to(DEV), ME.MinkowskiGlobalMaxPooling()):
        with pytest.raises(ValueError, match="origin tensor"):
            layer(pooled)


def test_geometry_only():
    from vdetr_amd import minkowski as ME
    from vdetr_amd.modules import senet
    sites = _sites((60, 40), (0, 1))
    x, _ = _tensor(torch.randn(len(sites), 8), sites)
    cm = x.coordinate_manager
    with ME.geometry_only():
        pooled = ME.MinkowskiGlobalMaxPooling()(x)
        assert pooled.F.shape == (2, 8) and pooled.tensor_stride == 0 and x.keys.data_ptr() in cm._scene_segments
        assert ME.MinkowskiBroadcastMultiplication()(x, pooled) is x and ME.MinkowskiBroadcastAddition()(x, pooled) is x
        both = ME.MinkowskiBroadcastConcatenation()(x, pooled)
        assert both.F.shape == (len(sites), 16) and both.keys is x.keys
        assert ME.MinkowskiLinear(8, 4).to(DEV)(pooled).F.shape == (2, 4)
        layer = senet.SELayer(8, reduction=2).to(DEV).eval()
        assert layer(x) is x and layer.last_path is None


def _block_setup():
    from vdetr_amd.modules import senet
    torch.manual_seed(5)
    block = senet.SEBasicBlock(32, 32, reduction=4, D=3).to(DEV)
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():  # norms that are no identity, a gate that is not flat
        for name, p in block.named_parameters():
            if "kernel" not in name and "linear.weight" not in name:
                p.copy_((torch.rand(p.shape, generator=gen) + 0.5) if name.endswith("weight") else torch.randn(p.shape, generator=gen) * 0.3)
    sites = R.cloud(400, 33, batch=2)
    nbr = R.neighbour_table(sites, sites, R.cube_offsets(3))
    g = torch.Generator().manual_seed(1)
    return block, sites, nbr, torch.randn(len(sites), 32, generator=g), torch.randn(len(sites), 32, generator=g)


def _block_reference(block, f, gout, nbr, sizes, dtype, order="torch", training=True):
    P = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in block.state_dict().items() if v.is_floating_point()}
    fr = f.detach().clone().to(dtype).requires_grad_(True)
    out = G.se_basic_block(P, fr, nbr, sizes, order, training=training)
    res = {"out": out.detach()}
    if training:
        (out * gout.to(dtype)).sum().backward()
        res["dfeats"] = fr.grad
        res.update({k: P[k].grad for k, _ in block.named_parameters()})
    return {k: v.to(G.F64) for k, v in res.items()}


def test_se_basic_block_forward_backward():
    from vdetr_amd import minkowski as ME
    block, sites, nbr, f, gout = _block_setup()
    sizes = R.scene_sizes(sites, 2)
    block.train()
    fd = f.to(DEV).requires_grad_(True)
    out = block(ME.SparseTensor(fd, torch.from_numpy(sites).int().to(DEV)))
    assert block.se.last_path == "composition" and out.tensor_stride == 1 and np.array_equal(out.C.cpu().numpy(), sites)
    (out.F * gout.to(DEV)).sum().backward()
    got = {"out": out.F.detach().cpu(), "dfeats": fd.grad.cpu()}
    got.update({k: p.grad.cpu() for k, p in block.named_parameters()})
    ref = _block_reference(block, f, gout, nbr, sizes, G.F64)
    rests = [_block_reference(block, f, gout, nbr, sizes, G.F32, o) for o in NC.ORDERS]
    figures = NC.compare(got, ref, rests, tuple(ref), label="SEBasicBlock")
    print({k: f"{v[0]:.2e} (restatement {v[1]:.2e}, factor {v[2]:.2f})" for k, v in figures.items()})


def test_pooling_and_broadcast_read_nothing_back():
    """forward and backward of MinkowskiGlobalAvgPooling -> MinkowskiBroadcastMultiplication contain no device-to-host read
    (torch's sync debug mode, shown first to raise on a plain .item())"""
    from vdetr_amd import minkowski as ME
    sizes, C = (260, 1, 90), 20
    sites = _sites(sizes, (0, 1, 2))
    g = torch.Generator().manual_seed(3)
    feats, dy = torch.randn(len(sites), C, generator=g) * 2 + 1, torch.randn(len(sites), C, generator=g)
    x, leaf = _tensor(feats, sites)
    pool, mul = ME.MinkowskiGlobalAvgPooling(), ME.MinkowskiBroadcastMultiplication()
    dyd = dy.to(DEV)
    mul(x, pool(x)).F.backward(dyd)  # (first call: builds the segment table and the origin keys; libraries and allocator warm)
    torch.cuda.synchronize()
    leaf.grad = None
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            raises = False
        except RuntimeError:
            raises = True
        if raises:
            y = mul(x, pool(x))
            y.F.backward(dyd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raises:
        y = mul(x, pool(x))
        y.F.backward(dyd)

    def evaluate(dtype, order="torch"):
        xr = feats.to(dtype).requires_grad_(True)
        out = torch.cat([xr[a:a + n] * (NC._sum(xr[a:a + n], (0,), order) * G._inv(n, dtype)) for a, n in zip(_starts(sizes), sizes)])
        (out * dy.to(dtype)).sum().backward()
        return {"y": out.detach().to(G.F64), "dx": xr.grad.to(G.F64)}

    NC.compare({"y": y.F.detach().cpu(), "dx": leaf.grad.cpu()}, evaluate(G.F64), [evaluate(G.F32, o) for o in NC.ORDERS], ("y", "dx"))
    if not raises:
        pytest.skip("this runtime ignores torch.cuda.set_sync_debug_mode: the no-host-read check did not run (parity did, and passed)")


def _gate_tolerance(ref_gate, rest_gates, scene_of):
    return torch.from_numpy(NC.tolerance(ref_gate, rest_gates))[scene_of]


def test_se_layer_inference_form():
    from vdetr_amd import minkowski as ME
    from vdetr_amd.modules import senet
    c = G.case("two", 64)
    sizes = c["sizes"]
    sites = _sites(sizes, (0, 1))
    layer = senet.SELayer(64, reduction=4).to(DEV)
    with torch.no_grad():
        for lin, w, b in ((layer.fc[0].linear, c["w1"], c["b1"]), (layer.fc[2].linear, c["w2"], c["b2"])):
            lin.weight.copy_(w), lin.bias.copy_(b)
    x, leaf = _tensor(c["x"], sites)
    layer.eval()
    assert layer(x).F.requires_grad and layer.last_path == "composition", "with autograd on the module takes the composition"
    relu = ME.MinkowskiReLU()
    for residual, act in ((None, None), (c["residual"], relu)):
        res = None if residual is None else x._like(residual.to(DEV))
        with torch.no_grad():
            fused = layer(x, res, act).F.cpu()
            assert layer.last_path == "fused"
            ME.INFER_FUSED = False
            try:
                plain = layer(x, res, act).F.cpu()
                assert layer.last_path == "composition"
            finally:
                ME.INFER_FUSED = True
        args = (c["x"], sizes, c["w1"], c["b1"], c["w2"], c["b2"], residual, act is not None)
        ref = G.se_layer_eval(*args)
        rests = [G.se_layer_eval(*args, dtype=G.F32, order=o) for o in NC.ORDERS]
        for name, y in (("fused", fused), ("composition", plain)):
            figures = NC.compare({"y": y}, ref, rests, ("y",), label=f"SELayer {name}")
            print(name, {k: f"{v[0]:.2e} (restatement {v[1]:.2e}, factor {v[2]:.2f})" for k, v in figures.items()})
        scene_of = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
        tol = 2 * _gate_tolerance(ref["gate"], [r["gate"] for r in rests], scene_of) * c["x"].abs().double() \
            + 4 * NC.ulp32(float(ref["y"].abs().max()))
        assert bool(((fused.double() - plain.double()).abs() <= tol).all()), "the two forms differ by more than the gate's tolerance times |x|"
    layer.train()
    with torch.no_grad():
        layer(x)
    assert layer.last_path == "composition"


def test_se_basic_block_inference_form():
    from vdetr_amd import minkowski as ME
    block, sites, nbr, f, gout = _block_setup()
    sizes = R.scene_sizes(sites, 2)
    block.eval()
    coords = torch.from_numpy(sites).int().to(DEV)
    with torch.no_grad():
        fused = block(ME.SparseTensor(f.to(DEV), coords)).F.cpu()
        assert block.se.last_path == "fused"
        ME.INFER_FUSED = False
        try:
            plain = block(ME.SparseTensor(f.to(DEV), coords)).F.cpu()
            assert block.se.last_path == "composition"
        finally:
            ME.INFER_FUSED = True
    block(ME.SparseTensor(f.to(DEV), coords))
    assert block.se.last_path == "composition", "with autograd on the module takes the composition"
    ref = _block_reference(block, f, gout, nbr, sizes, G.F64, training=False)
    rests = [_block_reference(block, f, gout, nbr, sizes, G.F32, o, training=False) for o in NC.ORDERS]
    for name, y in (("fused", fused), ("composition", plain)):
        figures = NC.compare({"out": y}, ref, rests, ("out",), label=f"SEBasicBlock {name}")
        print(name, {k: f"{v[0]:.2e} (restatement {v[1]:.2e}, factor {v[2]:.2f})" for k, v in figures.items()})
