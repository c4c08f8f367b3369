"""GPU: ``--use_normals`` on the device (v-detr_amd/scene_prep.py ``vertex_normals`` / ``with_normals`` -> csrc/normals.hip,
DESIGN.md 6.6) against the fixture made by the reference's own loader (tests/golden/normals.npz) and against the numpy
restatement for generated meshes.

Every operation is an IEEE float32 operation on exactly defined inputs and every vertex adds its faces in the serial loop's
order, so everything is compared with NO tolerance: ``torch.equal`` on the int32 views of the floats.  That includes the xyz
columns of the ``chain`` case, which DESIGN 6.4 only bounds by 2 ulps in general."""
import numpy as np
import pytest
import torch

from helpers import dev, same_bits
import normals_restatement as NR
from test_normals_restatement import PLAIN_CASES, fan_hub, golden, settings_of, state_is

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 64


def one(c, faces=None, **kw):
    """B = 1 call on a fixture case's mesh, the seven-column ply rows as they are"""
    from vdetr_amd.scene_prep import vertex_normals
    faces = c["faces"] if faces is None else faces
    return vertex_normals(dev(c["ply_vertices"]), np.array([0, len(c["ply_vertices"])]), faces, np.array([0, len(faces)]), **kw)


@pytest.mark.parametrize("name", PLAIN_CASES)
def test_fixture_cases_bit_for_bit(name):
    c = golden()[name]
    got = one(c)
    assert same_bits(got, c["out_points"][:, 6:9]), name
    if name == "fan":
        hub, _ = fan_hub(c)
        back = NR.vertex_normals(c["ply_vertices"], c["faces"], reverse=True)
        assert not same_bits(got[hub], back[hub])                      # the case can see a wrong order, and the order is right


def test_two_runs_give_the_same_bits():
    for name in ("fan", "grid"):
        a, b = one(golden()[name]), one(golden()[name])
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name


def batch_of(meshes):
    """[(xyz [n,3+], faces [F,3])] -> packed vertices, vert_offsets, packed faces (scene-local), face_offsets"""
    width = min(m[0].shape[1] for m in meshes)
    verts = np.concatenate([np.asarray(m[0], np.float32)[:, :width] for m in meshes])
    faces = np.concatenate([np.asarray(m[1], np.int32).reshape(-1, 3) for m in meshes])
    return (verts, np.cumsum([0] + [len(m[0]) for m in meshes]).astype(np.int32), faces,
            np.cumsum([0] + [len(m[1]) for m in meshes]).astype(np.int32))


def test_ragged_batch_equals_the_single_calls():
    from vdetr_amd.scene_prep import vertex_normals
    g = golden()
    lonely = (np.array([[0.5, -1.0, 2.0]], np.float32), np.zeros((0, 3), np.int32))
    meshes = [(g["isolated"]["ply_vertices"][:, :3], g["isolated"]["faces"]), lonely, (g["fan"]["ply_vertices"][:, :3], g["fan"]["faces"]),
              (g["grid"]["ply_vertices"][:, :3], g["grid"]["faces"])]
    verts, voff, faces, foff = batch_of(meshes)
    got = vertex_normals(dev(verts), voff, faces, foff)
    assert tuple(got.shape) == (len(verts), 3)
    for b, (xyz, f) in enumerate(meshes):
        alone = vertex_normals(dev(xyz), np.array([0, len(xyz)]), f, np.array([0, len(f)]))
        assert torch.equal(got[voff[b]:voff[b + 1]].view(torch.int32), alone.view(torch.int32)), b
        assert same_bits(alone, NR.vertex_normals(xyz, f)), b
    assert same_bits(got[voff[1]:voff[2]], np.zeros((1, 3), np.float32))          # no face: exactly +0


def test_out_lands_in_columns_6_to_9():
    from vdetr_amd.scene_prep import vertex_normals, with_normals
    c = golden()["grid"]
    n = len(c["ply_vertices"])
    plain = one(c)
    cloud = torch.arange(n * 9, dtype=torch.float32, device=DEV).reshape(n, 9)
    before = cloud.clone()
    view = cloud[:, 6:9]
    back = one(c, out=view)
    assert back is view and torch.equal(cloud[:, 6:9].view(torch.int32), plain.view(torch.int32))
    assert torch.equal(cloud[:, :6], before[:, :6])
    joined = with_normals(before[:, :6].contiguous(), plain)
    assert tuple(joined.shape) == (n, 9) and torch.equal(joined.view(torch.int32), cloud.view(torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        vertex_normals(dev(c["ply_vertices"]), np.array([0, n]), c["faces"], np.array([0, len(c["faces"])]), out=cloud[:, 5:9])


def test_int64_faces_equal_int32_faces():
    for name in ("degenerate", "grid"):
        c = golden()[name]
        narrow = one(c)
        assert torch.equal(one(c, faces=c["faces"].astype(np.int64)).view(torch.int32), narrow.view(torch.int32))
        assert torch.equal(one(c, faces=dev(c["faces"])).view(torch.int32), narrow.view(torch.int32))
        assert torch.equal(one(c, faces=dev(c["faces"].astype(np.int64))).view(torch.int32), narrow.view(torch.int32))


@pytest.mark.parametrize("dtype", (np.int32, np.int64))
def test_a_face_outside_its_scene_gives_nan_and_nothing_else(dtype):
    """device faces are not checked on the host: the kernels' bounds test turns the face into NaN for its in-range vertices.  One
    bad face names a row that exists in the packed batch but not in its scene, one a negative index (and, as int64, one an index
    that a cut to 32 bits would bring into range)"""
    from vdetr_amd.scene_prep import vertex_normals
    g = golden()
    meshes = [(g["isolated"]["ply_vertices"][:, :3], g["isolated"]["faces"].copy()), (g["grid"]["ply_vertices"][:, :3], g["grid"]["faces"].copy())]
    n0 = len(meshes[0][0])
    verts, voff, faces, foff = batch_of(meshes)
    faces = faces.astype(dtype)
    good = vertex_normals(dev(verts), voff, dev(faces), foff).cpu().numpy()
    bad = faces.copy()
    first, second = 2, int(foff[1]) + 700
    bad[first, 1] = n0 + 5                                             # a row of the second scene
    bad[second, 0] = -1 if dtype == np.int32 else 2 ** 32 + 7
    want = []
    for b, (xyz, f) in enumerate(meshes):
        f = bad[foff[b]:foff[b + 1]]
        ok = ((f >= 0) & (f < len(xyz))).all(1)
        normals = NR.vertex_normals(xyz, f[ok])
        hit = f[~ok].reshape(-1)
        normals[hit[(hit >= 0) & (hit < len(xyz))]] = np.nan
        want.append(normals)
    want = np.concatenate(want)
    got = vertex_normals(dev(verts), voff, dev(bad), foff).cpu().numpy()
    poisoned = np.isnan(want).all(1)
    assert poisoned.sum() == 4 and np.isnan(got[poisoned]).all()
    assert got[~poisoned].tobytes() == want[~poisoned].tobytes()
    untouched = np.ones(len(verts), bool)
    untouched[np.concatenate([faces[first], faces[second] + voff[1]])] = False
    assert got[untouched].tobytes() == good[untouched].tobytes()
    with pytest.raises(ValueError, match="outside their scene"):
        vertex_normals(dev(verts), voff, bad, foff)                    # the same array on the host is refused


def hub_mesh(rng, valence, twice=False):
    """a hub named by ``valence`` corners: triangles (rim, hub, rim) whose weights are spread over four orders of magnitude along
    the face order; ``twice``: two more faces name the hub twice each"""
    m = valence - (4 if twice else 0)
    rim = rng.normal(size=(m + 1, 3)) * (10.0 ** rng.uniform(-2, 0, (m + 1, 1)))
    xyz = np.concatenate([rng.normal(size=(1, 3)), rim]).astype(np.float32)
    faces = np.stack([np.arange(1, m + 1), np.zeros(m, np.int64), np.arange(2, m + 2)], 1)
    if twice:
        faces = np.concatenate([faces[:5], [(0, 0, 3)], faces[5:], [(0, 7, 0)]])
    return xyz, faces.astype(np.int32)


def test_list_lengths_around_the_workgroup_path():
    """hub valences on both sides of VDETR_NORMALS_SHORT (one lane orders the list / the workgroup sorts it), powers of two and
    not, 1000 faces, a repeated vertex inside a long and inside a short list; one ragged batch"""
    from vdetr_amd import _lib
    from vdetr_amd.scene_prep import vertex_normals
    short = _lib.VDETR_NORMALS_SHORT
    rng = np.random.default_rng(21)
    meshes = [hub_mesh(rng, v) for v in (1, short - 1, short, short + 1, 64, 255, 257, 1000)]
    meshes += [hub_mesh(rng, 20, twice=True), hub_mesh(rng, 300, twice=True)]
    verts, voff, faces, foff = batch_of(meshes)
    got = vertex_normals(dev(verts), voff, faces, foff)
    for b, (xyz, f) in enumerate(meshes):
        assert np.bincount(f.reshape(-1))[0] == (1, short - 1, short, short + 1, 64, 255, 257, 1000, 20, 300)[b]
        assert same_bits(got[voff[b]:voff[b + 1]], NR.vertex_normals(xyz, f)), b


def test_a_mesh_beyond_one_pass_of_the_scan():
    """more than 256 scan tiles of 1024 vertices, so the scan of the tile sums takes a second pass; vertices strided by 4"""
    from vdetr_amd.scene_prep import vertex_normals
    rng = np.random.default_rng(22)
    nx = ny = 515
    gx, gy = np.meshgrid(np.arange(nx, dtype=np.float64) * 0.02, np.arange(ny, dtype=np.float64) * 0.02, indexing="ij")
    xyz = np.stack([gx, gy, rng.uniform(0, 0.05, gx.shape), np.zeros_like(gx)], -1).reshape(-1, 4).astype(np.float32)
    at = np.arange(nx * ny).reshape(nx, ny)
    a, b, c, d = at[:-1, :-1], at[1:, :-1], at[:-1, 1:], at[1:, 1:]
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([b, d, c], -1).reshape(-1, 3)]).astype(np.int32)
    faces = faces[rng.permutation(len(faces))]
    assert len(xyz) > 256 * 1024
    got = vertex_normals(dev(xyz), np.array([0, len(xyz)]), faces, np.array([0, len(faces)]))
    assert same_bits(got, NR.vertex_normals(xyz, faces))


def test_no_scenes():
    from vdetr_amd.scene_prep import vertex_normals
    none = vertex_normals(torch.zeros((0, 3), device=DEV), np.array([0]), np.zeros((0, 3), np.int32), np.array([0]))
    assert tuple(none.shape) == (0, 3)


def test_chain_matches_the_reference_loader():
    """draw_color_augment -> augment_colors -> vertex_normals(out=columns 6:9) -> append_height -> crop_and_sample ->
    draw_augment_params -> prepare_scenes(choices, color_mean) -> sunrgbd_color_augment on one generator: the reference loader's
    [1024,10] cloud bit for bit, and its generator state"""
    from vdetr_amd import scene_prep as SP
    from vdetr_amd.dataset_config import ScannetDatasetConfig
    c = golden()["chain"]
    s = settings_of(c)
    rs = np.random.RandomState(int(c["seed"]))
    vert, boxes7, faces = c["vert"], c["boxes7"], c["faces"]
    n = len(vert)
    off = np.array([0, n])
    params = SP.draw_color_augment(n, rs, color_drop=s["color_drop"], color_contrastp=s["color_contrastp"], color_jitterp=s["color_jitterp"],
                                   hue_sat=s["hue_sat"])
    cloud9 = torch.empty((n, 9), dtype=torch.float32, device=DEV)
    cloud9[:, :6] = SP.augment_colors(dev(vert[:, :6]), off, [params])
    SP.vertex_normals(dev(c["ply_vertices"]), off, faces, np.array([0, len(faces)]), out=cloud9[:, 6:9])
    pts = SP.append_height(cloud9, off)
    cfg = ScannetDatasetConfig()
    boxes, classes = np.zeros((1, G, 6)), np.zeros((1, G), np.int64)
    boxes[0, :len(boxes7)], classes[0, :len(boxes7)] = boxes7[:, :6], SP.nyu40_to_class(boxes7[:, 6], cfg)
    out = SP.crop_and_sample(pts, off, dev(boxes), dev(np.array([len(boxes7)])), dev(classes), [rs], int(s["num_points"]),
                             min_points=int(s["min_points"]))
    pose = SP.draw_augment_params(1, *s["ratios"], random=rs)
    fin = SP.prepare_scenes(pts, off, out["boxes"].float(), out["box_counts"], out["box_classes"], pose, cfg, choices=out["choices"],
                            color_mean=float(s["color_mean"]))
    rows = len(fin["point_clouds"][0])
    SP.sunrgbd_color_augment(fin["point_clouds"], np.array([0, rows]), [SP.draw_sunrgbd_color(rows, rs)])
    got, want = fin["point_clouds"][0], c["out_points"]
    assert tuple(got.shape) == (1024, 10)
    host = got.cpu().numpy()
    for lo, hi, what in ((0, 3, "xyz"), (3, 6, "colours"), (6, 9, "normals"), (9, 10, "height")):
        print(f"chain {what}: {int((host[:, lo:hi].view(np.int32) != want[:, lo:hi].view(np.int32)).sum())} values differ")
    assert same_bits(got, want)
    assert state_is(rs, c["state_keys"], c["state_pos"])
