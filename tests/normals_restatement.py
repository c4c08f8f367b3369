"""numpy restatement of ``--use_normals``: the area-weighted vertex normals that datasets/scannet.py:394-420 of
the reference computes from a scan's mesh with a Python loop over the faces, and the place they take in the loaded cloud
(:457-458).  tests/test_normals_restatement.py holds it against tests/golden/normals.npz (made by the reference's own loader,
tools/make_normals_golden.py) bit for bit; the GPU tests use it for generated cases.

Everything is float32 and every line is one numpy operation per element, in the reference's association.  The loop
``nv[face[i]] += nf[i]`` is replaced by rounds: the corners are grouped by vertex, face order kept inside a group, and round r
adds every vertex's r-th incident face at once.  Each vertex therefore sees its own faces in ascending face index, which is all
the serial loop's result depends on.  A face that names a vertex twice is added twice here and once by numpy's fancy ``+=``; its
weight is +-0 for finite coordinates, so the sums are the same bits."""
import numpy as np

import color_aug_restatement as CA
import cuboid_restatement as CR
import scene_prep_restatement as SR

EPS = np.float32(1.0e-8)
HALF = np.float32(0.5)


def face_weights(vertex, face):
    """vertex float32 [n,3], face int [F,3] -> nf * area, float32 [F,3]"""
    vertex = np.asarray(vertex, np.float32)
    face = np.asarray(face)
    with np.errstate(all="ignore"):
        u = vertex[face[:, 1]] - vertex[face[:, 0]]
        v = vertex[face[:, 2]] - vertex[face[:, 0]]
        c0 = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        c1 = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        c2 = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        vec = np.stack([c0, c1, c2], 1)
        length = (np.sqrt((c0 * c0 + c1 * c1) + c2 * c2) + EPS)[:, None]
        return (vec / length) * (length * HALF)


def accumulate(weights, face, n, reverse=False):
    """-> float32 [n,3]: per vertex the sum of its corners' weight rows in ascending face order (descending with ``reverse``)"""
    face = np.asarray(face).astype(np.int64)
    nv = np.zeros((n, 3), np.float32)
    if len(face) == 0:
        return nv
    corner_vertex = face.reshape(-1)
    corner_face = np.repeat(np.arange(len(face)), 3)
    if reverse:
        corner_vertex, corner_face = corner_vertex[::-1], corner_face[::-1]
    order = np.argsort(corner_vertex, kind="stable")
    cv, cf = corner_vertex[order], corner_face[order]
    rank = np.arange(len(cv)) - np.searchsorted(cv, cv, side="left")   # the corner's place within its vertex's group
    by_round = np.argsort(rank, kind="stable")
    ends = np.cumsum(np.bincount(rank))
    with np.errstate(all="ignore"):
        for lo, hi in zip(np.concatenate([[0], ends[:-1]]), ends):
            sel = by_round[lo:hi]                                      # one corner per vertex: the fancy += adds each once
            nv[cv[sel]] += weights[cf[sel]]
    return nv


def normalise(nv):
    with np.errstate(all="ignore"):
        n0, n1, n2 = nv[:, 0], nv[:, 1], nv[:, 2]
        return nv / (np.sqrt((n0 * n0 + n1 * n1) + n2 * n2) + EPS)[:, None]


def vertex_normals(vertex, face, reverse=False):
    """the reference's ``vertex_normal(coords, faces)``: float32 [n,3]"""
    vertex = np.asarray(vertex, np.float32)[:, :3]
    return normalise(accumulate(face_weights(vertex, face), face, len(vertex), reverse))


def loader_scene(vert, ply_vertices, faces, boxes7, random, s):
    """the reference's ``__getitem__`` with ``use_color`` and ``use_normals`` from the loaded arrays (``vert``: the ``_vert.npy``
    array; ``ply_vertices`` / ``faces``: what ``read_plymesh`` returns) to ``point_clouds`` for the settings ``s``
    (color_aug_restatement.SETTINGS' keys and ``augment``)"""
    vert = np.asarray(vert, np.float32)
    normals = vertex_normals(ply_vertices, faces)
    boxes = np.asarray(boxes7)[:, :6]
    if not s["augment"]:
        cloud = np.concatenate([vert[:, :6], normals], 1)
        if s["use_height"]:
            cloud = CA.append_height_scene(cloud)
        pose = (False, False, 0.0, np.zeros(3), 1.0)
        return SR.prepare_scene(cloud, boxes.astype(np.float32), np.zeros(len(boxes), np.int64), *pose, np.zeros((1, 3)),
                                color_mean=float(s["color_mean"]), augment=False)["point_clouds"]
    cloud, _ = CA.color_augment_scene(vert[:, :6], random, **{k: v for k, v in s.items() if k != "augment"})
    cloud = np.concatenate([cloud, normals], 1)
    if s["use_height"]:
        cloud = CA.append_height_scene(cloud)
    choices = None
    if s["use_random_cuboid"]:
        got = CR.crop_and_sample_scene(cloud, boxes7, random, int(s["num_points"]), int(s["min_points"]))
        choices, boxes = got["rows"], np.asarray(boxes7)[got["keep_boxes"], :6]
    pose = CA.draw_pose(random, *s["ratios"])
    out = SR.prepare_scene(cloud, boxes.astype(np.float32), np.zeros(len(boxes), np.int64), *pose, np.zeros((1, 3)), choices=choices,
                           color_mean=float(s["color_mean"]))["point_clouds"]
    if s["coloraug_sunrgbd"]:
        CA.sunrgbd_scene(out, random)
    return out
