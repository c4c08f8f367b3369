"""The instrument of tests/test_gpu_sparse_pool.py and tests/test_gpu_sparse_inorm.py discriminates: the float32 restatements meet
the tolerances those files apply, stand-in mutants of the definitions do not, and the shared inputs have the properties the
tolerances lean on (neighbourhoods of several sizes, tied maxima, differing contributor counts).  CPU only."""
import numpy as np
import pytest
import torch

import norm_cases as NC
import sparse_modules_restatement as R

POOLED = [g for g in R.GEOMETRIES if not g.startswith("tr-") and g != "custom-s1"]


def _inside(got, ref, bound):
    return bool(((got.to(R.F64) - ref).abs() <= bound).all())


@pytest.mark.parametrize("geometry", list(R.GEOMETRIES))
def test_geometries_are_the_layers_own(geometry):
    """the instrument's offset lists, written out independently, are in the order the layers use: `arg` of the max pooling and the
    rows of `kernel` are compared index by index"""
    from vdetr_amd import minkowski as ME
    transposed, offsets, dilation, stride = R.GEOMETRIES[geometry]
    if geometry.startswith("custom"):
        gen = ME.KernelGenerator(region_type=ME.RegionType.CUSTOM, region_offsets=offsets, dimension=3)
    else:
        region = geometry.split("-")[1 if transposed else 0]   # "cube2", "cube3", "cross3"
        gen = ME.KernelGenerator(int(region[-1]), stride, dilation, is_transpose=transposed, dimension=3,
                                 region_type=ME.RegionType.HYPER_CROSS if region.startswith("cross") else ME.RegionType.HYPER_CUBE)
    assert list(gen.scaled_offsets()) == R.scale_reach(offsets, dilation)
    cls = ME.MinkowskiAvgUnpooling if transposed else ME.MinkowskiAvgPooling
    layer = cls(gen.kernel_size, stride=stride, dilation=dilation, kernel_generator=gen)
    assert tuple(layer._offsets) == tuple(R.scale_reach(offsets, dilation)) and layer.transposed == transposed


@pytest.mark.parametrize("geometry", list(R.GEOMETRIES))
def test_inputs_have_neighbourhoods_of_several_sizes(geometry):
    _, outs, nbr = R.pool_geometry("two", geometry)
    counts = (nbr >= 0).sum(0)
    distinct = set(counts.tolist())
    if geometry == "tr-cube2-s2":
        assert distinct == {1}  # every fine site has exactly one parent
    else:
        assert len(distinct) >= 3, distinct
    if geometry == "tr-cube3-s2":
        assert len(distinct) >= 2  # it is in the list because the contributor counts differ
    if geometry == "custom-s1":
        assert 0 in distinct and float((counts == 0).float().mean()) > 0.2
    assert len(outs) == nbr.shape[1]


@pytest.mark.parametrize("geometry", POOLED)
def test_maxima_tie(geometry):
    x, _ = R.pool_inputs("two", geometry, 20)
    _, _, nbr = R.pool_geometry("two", geometry)
    g = R._gathered(x.to(R.F64), nbr)
    g = torch.where((nbr >= 0)[:, :, None], g, torch.full_like(g, -float("inf")))
    ties = (g == g.max(0).values[None]).sum(0) >= 2
    assert float(ties.float().mean()) >= 0.05


@pytest.mark.parametrize("geometry", list(R.GEOMETRIES))
@pytest.mark.parametrize("mode", ["sum", "avg"])
def test_float32_restatement_meets_the_pool_bounds(geometry, mode):
    x, dy = R.pool_inputs("two", geometry, 20)
    ins, _, nbr = R.pool_geometry("two", geometry)
    y64, ic, _ = R.pool_forward(x, nbr, mode)
    y32, ic32, _ = R.pool_forward(x, nbr, mode, dtype=R.F32)
    assert _inside(y32, y64, R.pool_bound_forward(x, nbr, ic))
    dx64 = R.pool_backward(dy, nbr, len(ins), mode, ic)
    dx32 = R.pool_backward(dy, nbr, len(ins), mode, ic32, dtype=R.F32)
    assert _inside(dx32, dx64, R.pool_bound_backward(dy, nbr, len(ins), ic))
    if mode == "avg":
        empty = (nbr >= 0).sum(0) == 0
        assert bool((y64[empty] == 0).all()) and bool(torch.isfinite(y64).all())


@pytest.mark.parametrize("geometry", POOLED)
def test_pool_mutants_fall_outside(geometry):
    x, dy = R.pool_inputs("two", geometry, 20)
    ins, _, nbr = R.pool_geometry("two", geometry)
    y64, ic, _ = R.pool_forward(x, nbr, "avg")
    bad, _, _ = R.pool_forward(x, nbr, "avg", dtype=R.F32, defect="avg_by_K")
    assert not _inside(bad, y64, R.pool_bound_forward(x, nbr, ic)), "avg divided by K"
    ym, _, arg = R.pool_forward(x, nbr, "max")
    yb, _, argb = R.pool_forward(x, nbr, "max", defect="tie_highest")
    assert torch.equal(ym, yb) and not torch.equal(arg, argb), "max ties to the highest k"
    dx = R.pool_backward(dy, nbr, len(ins), "max", arg=arg, dtype=R.F32)
    dxb = R.pool_backward(dy, nbr, len(ins), "max", arg=argb, dtype=R.F32)
    assert not torch.equal(dx, dxb)


def test_unpooling_without_the_count_falls_outside():
    x, _ = R.pool_inputs("two", "tr-cube3-s2", 20)
    _, _, nbr = R.pool_geometry("two", "tr-cube3-s2")
    y64, ic, _ = R.pool_forward(x, nbr, "avg")
    plain, _, _ = R.pool_forward(x, nbr, "sum", dtype=R.F32)
    assert not _inside(plain, y64, R.pool_bound_forward(x, nbr, ic))


def test_max_of_an_empty_neighbourhood():
    x, dy = R.pool_inputs("two", "custom-s1", 4)
    ins, _, nbr = R.pool_geometry("two", "custom-s1")
    y, _, arg = R.pool_forward(x, nbr, "max")
    empty = (nbr >= 0).sum(0) == 0
    assert bool((y[empty] == 0).all()) and bool((arg[empty] == -1).all()) and bool((arg[~empty] >= 0).all())
    dx = R.pool_backward(dy, nbr, len(ins), "max", arg=arg)
    unread = torch.ones(len(ins), dtype=torch.bool)
    unread[nbr[nbr >= 0]] = False
    assert bool((dx[unread] == 0).all())


NAMES = ("y", "dx", "dweight", "dbias")


@pytest.mark.parametrize("scenes,C", R.INORM_CASES[:-1])
def test_inorm_held_out_order_meets_the_tolerance(scenes, C):
    """the rule of norm_cases with one summation order held out as a stand-in kernel"""
    case = R.inorm_case(scenes, C)
    ref = R.inorm_reference(case)
    held = ("tree", 64)
    rests = R.inorm_restatements(case, orders=[o for o in NC.ORDERS if o != held])
    stand_in = R.inorm_restatements(case, orders=[held])[0]
    NC.compare(stand_in, ref, rests, NAMES, case["groups"], case["extra"], label=f"{scenes} C={C}")
    sizes = case["sizes"]
    if 1 in sizes:  # a scene with one site gives the bias
        a = sum(sizes[:sizes.index(1)])
        assert torch.equal(ref["y"][a], case["beta"].to(R.F64))
    assert bool(torch.isfinite(ref["y"]).all()) and bool(torch.isfinite(ref["dx"]).all())


@pytest.mark.parametrize("scenes,C", [("two", 20), ("single", 64), ("absent", 4)])
@pytest.mark.parametrize("defect", ["whole_batch", "unbiased"])
def test_inorm_mutants_fall_outside(scenes, C, defect):
    case = R.inorm_case(scenes, C)
    ref = R.inorm_reference(case)
    rests = R.inorm_restatements(case)
    bad = R.inorm_restatements(case, orders=["torch"], defect=defect)[0]
    with pytest.raises(AssertionError):
        NC.compare(bad, ref, rests, ("y",), case["groups"], case["extra"])
    with pytest.raises(AssertionError):
        NC.compare(bad, ref, rests, ("dx",), case["groups"], case["extra"])


def test_cases_cover_the_four_kinds_per_scene():
    case = R.inorm_case("two", 20)
    a = 0
    for n in case["sizes"]:
        assert set(np.unique(case["groups"]["y"][a:a + n])) == {0, 1, 2, 3}
        a += n
    assert case["groups"]["y"][0, 0] != case["groups"]["y"][a - 1, 0]  # the kinds rotate from scene to scene
