"""CPU: the numpy restatement of ``--use_normals`` (tests/normals_restatement.py) against the fixture that the reference's own
loader produced (tests/golden/normals.npz, tools/make_normals_golden.py), bit for bit and with the generator's state, and the
cases the fixture has to hold, re-asserted so that a regenerated file cannot lose one."""
import os

import numpy as np
import pytest

import color_aug_restatement as CA
import normals_restatement as NR
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "normals.npz")
CASES = ("single", "isolated", "degenerate", "tiny", "fan", "grid", "chain")
PLAIN_CASES = tuple(c for c in CASES if c != "chain")                  # augment=False: columns 6:9 are every vertex's normal
SETTINGS = dict(CA.SETTINGS, augment=False)
FAN_FACES = 700
_cache = {}


def golden():
    """-> {case name: {key: array}}; loaded once"""
    if not _cache:
        z = np.load(GOLDEN)
        for name in z["cases"]:
            _cache[str(name)] = {k.split(":", 1)[1]: z[k] for k in z.files if k.startswith(f"{name}:")}
    return _cache


def settings_of(c):
    return {k: c[f"set_{k}"].item() if c[f"set_{k}"].ndim == 0 else tuple(c[f"set_{k}"].tolist()) for k in SETTINGS}


def state_is(random, keys, pos):
    s = random.get_state()
    return np.array_equal(s[1], keys) and s[2] == int(pos)


def fan_hub(c):
    """the vertex of the fan that most faces name, and how many"""
    counts = np.bincount(c["faces"].reshape(-1), minlength=len(c["ply_vertices"]))
    return int(np.argmax(counts)), int(counts.max())


def cases_present(name, c, s):
    """the case ``name`` of the fixture holds what DESIGN.md 6.6 says it holds"""
    xyz, faces = c["ply_vertices"][:, :3], c["faces"]
    n, F = len(xyz), len(faces)
    assert c["ply_vertices"].dtype == np.float32 and c["ply_vertices"].shape[1] == 7 and faces.dtype == np.int32 and faces.shape == (F, 3)
    assert faces.min() >= 0 and faces.max() < n and np.isfinite(xyz).all()
    normals = c["out_points"][:, 6:9]
    counts = np.bincount(faces.reshape(-1), minlength=n)
    if name != "chain":
        assert not s["augment"] and c["out_points"].shape == (n, 9)
    if name == "single":
        assert (n, F) == (3, 1) and np.abs(normals).max() > 0.5
    if name == "isolated":
        lone = counts == 0
        assert lone.sum() >= 3 and (~lone).sum() >= 3
        assert normals[lone].tobytes() == np.zeros((int(lone.sum()), 3), np.float32).tobytes()     # exactly +0
    if name == "degenerate":
        twice = [int(f[0] == f[1]) + int(f[1] == f[2]) + int(f[0] == f[2]) for f in faces]
        assert 1 in twice and 3 in twice                               # (a,a,b) / (a,b,b) and (a,a,a)
        assert any(f[0] == f[1] != f[2] for f in faces) and any(f[0] != f[1] == f[2] for f in faces)
        w = NR.face_weights(xyz, faces)
        flat = [i for i, t in enumerate(twice) if t == 0 and not w[i].any()]
        assert flat, "three distinct collinear vertices with a zero weight"
        assert all(not w[i].any() for i, t in enumerate(twice) if t)
    if name == "tiny":
        with np.errstate(all="ignore"):
            u, v = xyz[faces[:, 1]] - xyz[faces[:, 0]], xyz[faces[:, 2]] - xyz[faces[:, 0]]
            sq = np.cross(u, v) ** 2
        smallest = np.finfo(np.float32).tiny
        assert ((sq > 0) & (sq < smallest)).any() and (sq.sum(1) == 0).any()
        edge = np.linalg.norm(u.astype(np.float64), axis=1)
        assert (edge < 3e-12).any() and (edge < 3e-19).any()
        assert np.abs(normals).max() < 0.9                             # + 1e-8 decides: nothing is a unit vector
    if name == "fan":
        hub, faces_at_hub = fan_hub(c)
        assert faces_at_hub >= FAN_FACES
        w = np.linalg.norm(NR.face_weights(xyz, faces).astype(np.float64), axis=1)
        assert w.max() / w.min() >= 1e6
        back = NR.vertex_normals(xyz, faces, reverse=True)
        assert back[hub].tobytes() != normals[hub].tobytes(), "the reversed face order must change the hub's bits"
    if name == "grid":
        assert (n, F) == (1023, 1920) and counts.max() == 6 and n % 64 and F % 256
    if name == "chain":
        assert n == 3000 and s["augment"] and s["use_random_cuboid"] and s["coloraug_sunrgbd"] and s["use_height"]
        assert c["out_points"].shape == (1024, 10)
        _, t = CA.color_augment_scene(c["vert"], np.random.RandomState(int(c["seed"])), **{k: v for k, v in s.items() if k != "augment"})
        assert t["contrast"] and t["jitter"] and t["hue"] and t["dropped"] > 0


def test_fixture_holds_the_cases_of_the_design():
    g = golden()
    assert set(CASES) == set(g)
    for name in CASES:
        cases_present(name, g[name], settings_of(g[name]))
    assert os.path.getsize(GOLDEN) < 400 * 1024


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_bit_for_bit(name):
    c = golden()[name]
    rs = np.random.RandomState(int(c["seed"]))
    out = NR.loader_scene(c["vert"], c["ply_vertices"], c["faces"], c["boxes7"], rs, settings_of(c))
    assert out.dtype == np.float32 and out.shape == c["out_points"].shape
    assert out.tobytes() == c["out_points"].tobytes()
    assert state_is(rs, c["state_keys"], c["state_pos"])


@pytest.mark.parametrize("name", PLAIN_CASES)
def test_normals_alone_equal_the_reference(name):
    c = golden()[name]
    got = NR.vertex_normals(c["ply_vertices"], c["faces"])
    assert got.dtype == np.float32 and got.tobytes() == c["out_points"][:, 6:9].tobytes()
    assert NR.vertex_normals(c["ply_vertices"], c["faces"].astype(np.int64)).tobytes() == got.tobytes()


def test_the_fan_sees_a_wrong_order():
    c = golden()["fan"]
    hub, _ = fan_hub(c)
    forward = NR.vertex_normals(c["ply_vertices"], c["faces"])
    back = NR.vertex_normals(c["ply_vertices"], c["faces"], reverse=True)
    assert forward[hub].tobytes() == c["out_points"][hub, 6:9].tobytes() and back[hub].tobytes() != forward[hub].tobytes()


def test_rounds_are_the_serial_loop():
    """the restatement's grouped rounds against the loop written out, on meshes with repeated vertices inside a face"""
    rng = np.random.default_rng(12)
    for n in (1, 2, 3, 17, 200):
        face = rng.integers(0, n, (3 * n + 1, 3)).astype(np.int32)
        vertex = rng.normal(size=(n, 3)).astype(np.float32)
        w = NR.face_weights(vertex, face)
        nv = np.zeros_like(vertex)
        for i in range(len(face)):
            nv[face[i]] += w[i]
        assert NR.accumulate(w, face, n).tobytes() == nv.tobytes()
    assert NR.vertex_normals(np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32)).tobytes() == np.zeros((4, 3), np.float32).tobytes()
