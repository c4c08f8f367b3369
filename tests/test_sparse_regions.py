"""Kernel regions of the sparse layers (minkowski.RegionType / KernelGenerator) and the module library built on them
(vdetr_amd.modules): offset lists and their order, volumes, scaling, parameter shapes, state-dict keys.  No GPU needed."""
import pytest
import torch

import sparse_modules_restatement as R

CUBE3 = [(-1, -1, -1), (0, -1, -1), (1, -1, -1), (-1, 0, -1), (0, 0, -1), (1, 0, -1), (-1, 1, -1), (0, 1, -1), (1, 1, -1),
         (-1, -1, 0), (0, -1, 0), (1, -1, 0), (-1, 0, 0), (0, 0, 0), (1, 0, 0), (-1, 1, 0), (0, 1, 0), (1, 1, 0),
         (-1, -1, 1), (0, -1, 1), (1, -1, 1), (-1, 0, 1), (0, 0, 1), (1, 0, 1), (-1, 1, 1), (0, 1, 1), (1, 1, 1)]
CUBE2 = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
CUBE313 = [(-1, 0, -1), (0, 0, -1), (1, 0, -1), (-1, 0, 0), (0, 0, 0), (1, 0, 0), (-1, 0, 1), (0, 0, 1), (1, 0, 1)]
CROSS3 = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
CROSS5 = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (-2, 0, 0), (2, 0, 0), (0, -1, 0), (0, 1, 0), (0, -2, 0), (0, 2, 0),
          (0, 0, -1), (0, 0, 1), (0, 0, -2), (0, 0, 2)]


def test_region_type_values():
    from vdetr_amd import minkowski as ME
    assert [ME.RegionType(m) for m in range(3)] == [ME.RegionType.HYPER_CUBE, ME.RegionType.HYPER_CROSS, ME.RegionType.CUSTOM]
    assert [m.value for m in ME.RegionType] == [0, 1, 2]


def test_offset_lists_and_volumes():
    from vdetr_amd import minkowski as ME
    gen = lambda *a, **kw: ME.KernelGenerator(*a, dimension=3, **kw)  # noqa: E731
    cross = ME.RegionType.HYPER_CROSS
    for got, want in ((gen(3), CUBE3), (gen(2), CUBE2), (gen((3, 1, 3)), CUBE313), (gen(3, region_type=cross), CROSS3),
                      (gen(5, region_type=cross), CROSS5)):
        assert got.offsets == want
        assert got.kernel_volume == len(want)
    assert gen((3, 5, 1), region_type=cross).kernel_volume == 1 + 2 + 4 + 0
    assert gen(5).kernel_volume == 125 and gen(4).kernel_volume == 64 and gen(1).offsets == [(0, 0, 0)]
    custom = [(1, 0, 0), (0, 5, 0), (-1, -1, 0)]
    for offs in (custom, torch.tensor(custom)):
        g = gen(region_type=ME.RegionType.CUSTOM, region_offsets=offs)
        assert g.offsets == custom and g.kernel_volume == 3
    # the restatement's lists are written independently: the same order
    assert R.cube_offsets(3) == CUBE3 and R.cube_offsets((3, 1, 3)) == CUBE313 and R.cross_offsets(5) == CROSS5
    assert gen(3, axis_types=[cross] * 3).offsets == CROSS3  # three equal entries: that region


def test_existing_layers_keep_their_offsets_and_kernel_shapes():
    from vdetr_amd import minkowski as ME
    for k in (1, 2, 3):
        assert ME.KernelGenerator(k, dimension=3).offsets == ME._region_offsets(k)
        conv = ME.MinkowskiConvolution(8, 12, kernel_size=k, dimension=3)
        assert tuple(conv._offsets) == tuple(ME._region_offsets(k)) == ME._kernel_offsets(k) == ME._kernel_offsets(conv._offsets)
        assert conv.kernel_size == k
    assert ME.MinkowskiConvolution(8, 12, kernel_size=3, dimension=3).kernel.shape == (27, 8, 12)
    assert ME.MinkowskiConvolution(8, 12, kernel_size=1, dimension=3).kernel.shape == (8, 12)
    assert ME.MinkowskiConvolution(8, 12, kernel_size=1, stride=2, dimension=3).kernel.shape == (1, 8, 12)
    assert ME.MinkowskiConvolutionTranspose(8, 12, kernel_size=2, stride=2, dimension=3).kernel.shape == (8, 8, 12)
    assert ME.MinkowskiGenerativeConvolutionTranspose(8, 12, kernel_size=2, stride=2, dimension=3).kernel.shape == (8, 8, 12)
    assert ME.MinkowskiConvolution(8, 12, kernel_size=(3, 1, 3), dimension=3).kernel.shape == (9, 8, 12)
    cross = ME.KernelGenerator(3, region_type=ME.RegionType.HYPER_CROSS, dimension=3)
    for cls in (ME.MinkowskiConvolution, ME.MinkowskiConvolutionTranspose, ME.MinkowskiGenerativeConvolutionTranspose):
        assert cls(8, 12, kernel_size=3, kernel_generator=cross, dimension=3).kernel.shape == (7, 8, 12)
    # the initialisation scales with the volume where it did with kernel_size ** 3
    torch.manual_seed(0)
    w = ME.MinkowskiConvolution(8, 12, kernel_size=3, kernel_generator=cross, dimension=3).kernel.detach()
    assert float(w.abs().max()) <= 1.0 / (8 * 7) ** 0.5 and float(w.abs().max()) > 1.0 / (8 * 27) ** 0.5


def test_dilation_and_tensor_stride_scaling(monkeypatch):
    from vdetr_amd import minkowski as ME
    g = ME.KernelGenerator(3, 1, 2, region_type=ME.RegionType.HYPER_CROSS, dimension=3)
    assert list(g.scaled_offsets()) == [(2 * x, 2 * y, 2 * z) for x, y, z in CROSS3]
    assert list(ME.KernelGenerator(3, 1, (1, 2, 3), dimension=3).scaled_offsets()) == [(x, 2 * y, 3 * z) for x, y, z in CUBE3]
    conv = ME.MinkowskiConvolution(4, 4, kernel_size=3, dilation=2, dimension=3)
    assert tuple(conv._offsets) == tuple((2 * x, 2 * y, 2 * z) for x, y, z in CUBE3) and conv.kernel.shape == (27, 4, 4)
    # the map a layer asks for: offset * dilation * tensor stride (convolution, pooling), -offset * dilation * out stride (transposed)
    import vdetr_amd.sparse_ops as S
    asked = []
    monkeypatch.setattr(S, "kernel_map", lambda ik, ok, off: asked.append(off.clone()) or torch.full((off.shape[0], ok.shape[0]), -1,
                                                                                                  dtype=torch.int32))
    monkeypatch.setattr(S, "PairPlan", lambda nbr, nin: None)
    monkeypatch.setattr(S, "ConvPlan", lambda nbr, nin: None)
    monkeypatch.setattr(S, "inverse_map", lambda nbr, nin: None)
    cm = ME.CoordinateManager("cpu")
    keys = torch.arange(5, dtype=torch.int64)
    cm.kernel_map(keys, keys, 4, 4, g, False)
    cm.kernel_map(keys, keys, 4, 2, ME.KernelGenerator(2, 2, 1, dimension=3), True)
    n = len(cm.maps)
    cm.kernel_map(keys, keys, 4, 4, 3, False)
    cm.kernel_map(keys, keys, 4, 4, ME.KernelGenerator(3, region_type=ME.RegionType.HYPER_CROSS, dimension=3), False)
    assert len(cm.maps) == n + 2, "a cube and a cross of size 3 over the same sites must not share a plan"
    cm.kernel_map(keys, keys, 4, 4, ME.MinkowskiConvolution(4, 4, 3)._offsets, False)
    assert len(cm.maps) == n + 2, "equal offsets share one plan"
    assert asked[0].tolist() == [[8 * x, 8 * y, 8 * z] for x, y, z in CROSS3]
    assert asked[1].tolist() == [[-2 * x, -2 * y, -2 * z] for x, y, z in CUBE2]


def test_errors():
    from vdetr_amd import minkowski as ME
    from vdetr_amd.modules import common as C
    cube, cross = ME.RegionType.HYPER_CUBE, ME.RegionType.HYPER_CROSS
    with pytest.raises(ValueError):
        ME.KernelGenerator(3, 2, 2, dimension=3)
    with pytest.raises(ValueError):
        ME.MinkowskiConvolution(4, 4, kernel_size=3, stride=2, dilation=2, dimension=3)
    with pytest.raises(ValueError):
        ME.MinkowskiAvgPooling(3, stride=2, dilation=2)
    with pytest.raises(ValueError):
        ME.KernelGenerator(4, region_type=cross, dimension=3)   # a cross needs odd sizes
    for dim in (-1, 2, 4):
        with pytest.raises(NotImplementedError):
            ME.KernelGenerator(3, dimension=dim)
    with pytest.raises(NotImplementedError):
        ME.KernelGenerator(3, axis_types=[cube, cube, cross], dimension=3)
    with pytest.raises(NotImplementedError):
        ME.KernelGenerator((3, 3), dimension=3)
    for kind in C.ConvType:
        with pytest.raises(NotImplementedError):
            C.conv(4, 4, 3, conv_type=kind, D=4)
    with pytest.raises(NotImplementedError):
        C.avg_pool(2, 2, D=4)
    with pytest.raises(AssertionError):
        C.conv(4, 4, 3)   # D defaults to -1


def test_module_library_names_and_shapes():
    from vdetr_amd import minkowski as ME
    from vdetr_amd.modules import common as C
    import vdetr_amd.modules.resnet_block  # noqa: F401
    assert [int(k) for k in C.ConvType] == list(range(7)) and C.ConvType.HYPERCROSS.fullname == "HYPERCROSS"
    assert [n.value for n in C.NormType] == [0, 1, 2]
    assert C.convert_region_type(1) is ME.RegionType.HYPER_CROSS and C.int_to_region_type[2] is ME.RegionType.CUSTOM
    volumes = {C.ConvType.HYPERCUBE: 27, C.ConvType.SPATIAL_HYPERCUBE: 27, C.ConvType.SPATIO_TEMPORAL_HYPERCUBE: 27,
               C.ConvType.HYPERCROSS: 7, C.ConvType.SPATIAL_HYPERCROSS: 7, C.ConvType.SPATIO_TEMPORAL_HYPERCROSS: 7,
               C.ConvType.SPATIAL_HYPERCUBE_TEMPORAL_HYPERCROSS: 27}
    for kind, vol in volumes.items():
        assert C.conv(6, 10, 3, conv_type=kind, D=3).kernel.shape == (vol, 6, 10), kind
        assert C.conv_tr(6, 10, 3, upsample_stride=2, conv_type=kind, D=3).kernel.shape == (vol, 6, 10), kind
        assert C.conv_to_region_type[kind] is (ME.RegionType.HYPER_CROSS if vol == 7 else ME.RegionType.HYPER_CUBE)
        region, axis_types, size = C.convert_conv_type(kind, 3, 3)
        assert size == ([3, 3, 3] if "SPATIAL_HYPERC" in kind.name and "TEMPORAL" not in kind.name else 3)
    assert C.conv(6, 10, 1, D=3).kernel.shape == (6, 10)
    assert C.conv(6, 10, 3, bias=True, D=3).bias.shape == (1, 10)
    assert isinstance(C.avg_pool(2, 2, D=3), ME.MinkowskiAvgPooling) and isinstance(C.sum_pool(2, 2, D=3), ME.MinkowskiSumPooling)
    assert isinstance(C.avg_unpool(2, 2, D=3), ME.MinkowskiAvgUnpooling) and C.avg_unpool(2, 2, D=3).transposed
    assert isinstance(C.get_norm(C.NormType.BATCH_NORM, 8, 3), ME.MinkowskiBatchNorm)
    assert isinstance(C.get_norm(C.NormType.INSTANCE_NORM, 8, 3), ME.MinkowskiInstanceNorm)
    inbn = C.get_norm(C.NormType.INSTANCE_BATCH_NORM, 8, 3, bn_momentum=0.05)
    assert isinstance(inbn[0], ME.MinkowskiInstanceNorm) and inbn[1].bn.momentum == 0.05
    with pytest.raises(ValueError):
        C.get_norm(7, 8, 3)


_BN = lambda p: [f"{p}.bn.weight", f"{p}.bn.bias", f"{p}.bn.running_mean", f"{p}.bn.running_var", f"{p}.bn.num_batches_tracked"]  # noqa: E731
_NORM_KEYS = {"": _BN, "IN": lambda p: [f"{p}.weight", f"{p}.bias"],
              "INBN": lambda p: [f"{p}.0.weight", f"{p}.0.bias"] + _BN(f"{p}.1")}


@pytest.mark.parametrize("suffix", ["", "IN", "INBN"])
def test_block_state_dict_keys(suffix):
    from vdetr_amd.modules import common as C, resnet_block as RB
    nk = _NORM_KEYS[suffix]
    basic = getattr(RB, "BasicBlock" + suffix)(16, 16, stride=2, conv_type=C.ConvType.HYPERCROSS)
    assert list(basic.state_dict()) == ["conv1.kernel"] + nk("norm1") + ["conv2.kernel"] + nk("norm2")
    assert basic.expansion == 1 and basic.conv1.kernel.shape == (7, 16, 16) and basic.conv1.stride == 2 and basic.conv2.stride == 1
    assert isinstance(basic, RB.BasicBlockBase) and basic.NORM_TYPE == C.NormType(["", "IN", "INBN"].index(suffix))
    neck = getattr(RB, "Bottleneck" + suffix)(16, 8, dilation=2)
    assert list(neck.state_dict()) == (["conv1.kernel"] + nk("norm1") + ["conv2.kernel"] + nk("norm2") + ["conv3.kernel"] + nk("norm3"))
    assert neck.expansion == 4 and neck.conv1.kernel.shape == (16, 8) and neck.conv2.kernel.shape == (27, 8, 8)
    assert neck.conv3.kernel.shape == (8, 32) and tuple(neck.conv2._offsets)[0] == (-2, -2, -2)
    assert isinstance(neck, RB.BottleneckBase)
