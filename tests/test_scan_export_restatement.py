"""CPU: the numpy restatement of the scan export (tests/scan_export_restatement.py) and the host tables of
v-detr_amd/scan_export.py against the fixture that the reference's own ``export`` and ``export_one_scan`` produced
(tests/golden/scan_export.npz, tools/make_scan_export_golden.py), bit for bit; the cases the fixture has to hold, re-asserted
so that a regenerated file cannot lose one; and the inputs ``scan_tables`` has to refuse."""
import os

import numpy as np
import pytest

import scan_export_restatement as SR
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "scan_export.npz")
CASES = ("single", "edge_m1", "edge", "edge_p1", "negative", "shared_seg", "empty_object", "unannotated", "donotcare", "identity")
INPUT_KEYS = ("mesh", "seg_indices", "group_object", "group_label", "group_seg_offsets", "group_segs", "map_names", "map_ids", "axis_align",
              "donotcare")
EXPORT_KEYS = ("ex_vertices", "ex_labels", "ex_instances", "ex_bboxes", "ex_object_ids", "ex_object_labels")
FILE_KEYS = ("vert", "sem_label", "ins_label", "bbox")
# raw categories -> nyu40 ids: every id of the label file's range that the cases use, several raw names per id as in the real file
LABEL_MAP = {"wall": 1, "floor": 2, "cabinet": 3, "kitchen cabinet": 3, "bed": 4, "chair": 5, "office chair": 5, "armchair": 5, "couch": 6,
             "table": 7, "coffee table": 7, "door": 8, "window": 9, "bookshelf": 10, "picture": 11, "counter": 12, "blinds": 13, "desk": 14,
             "shelf": 15, "curtain": 16, "dresser": 17, "pillow": 18, "mirror": 19, "refrigerator": 24, "shower curtain": 28, "toilet": 33,
             "sink": 34, "bathtub": 36, "trash can": 39, "lamp": 35, "box": 40, "unknown thing": 0}
_cache = {}


def golden():
    """-> {case name: {key: array}}; loaded once"""
    if not _cache:
        z = np.load(GOLDEN)
        for name in z["cases"]:
            _cache[str(name)] = {k.split(":", 1)[1]: z[k] for k in z.files if k.startswith(f"{name}:")}
    return _cache


def pack_inputs(scan, donotcare=()):
    """a scan (``make_scan``'s dict) as the arrays the fixture stores"""
    groups = scan["groups"]
    return {"mesh": scan["mesh"], "seg_indices": np.asarray(scan["seg_indices"], np.int32),
            "group_object": np.array([g["objectId"] for g in groups], np.int64),
            "group_label": np.array([g["label"] for g in groups], dtype="U32"),
            "group_seg_offsets": np.cumsum([0] + [len(g["segments"]) for g in groups]).astype(np.int64),
            "group_segs": np.array([s for g in groups for s in g["segments"]], np.int64),
            "map_names": np.array(list(scan["label_map"]), dtype="U32"), "map_ids": np.array(list(scan["label_map"].values()), np.int64),
            "axis_align": np.asarray(scan["axis_align"], np.float64).reshape(16), "donotcare": np.array(donotcare, np.int64)}


def inputs_of(c):
    """a fixture case -> (mesh, seg_indices list, segGroups, label_map, axis_align 16 floats)"""
    o, s = c["group_seg_offsets"], c["group_segs"]
    groups = [{"objectId": int(c["group_object"][i]), "label": str(c["group_label"][i]), "segments": s[o[i]:o[i + 1]].tolist()}
              for i in range(len(c["group_object"]))]
    label_map = {str(k): int(v) for k, v in zip(c["map_names"], c["map_ids"])}
    return c["mesh"], c["seg_indices"].tolist(), groups, label_map, c["axis_align"].tolist()


def make_scan(rng, n, K, *, cover=1.0, seg_size=8, labels=None, translation=None, centres=None):
    """a generated raw scan: ``n`` vertices in runs of about ``seg_size`` per segment with scattered raw segment ids, ``K``
    objects (every one owns a segment; needs n >= K) that cover about ``cover`` of the segments, an axis alignment as ScanNet
    writes it (a turn about z and a translation) -> dict mesh f32 [n,6], seg_indices, groups, label_map, axis_align [16]"""
    labels = list(LABEL_MAP) if labels is None else list(labels)
    cuts = np.unique(np.concatenate([[0], rng.choice(np.arange(1, n), min(n - 1, max(K - 1, n // seg_size)), replace=False)])) if n > 1 else np.array([0])
    S = len(cuts)
    assert S >= K
    raw_ids = rng.choice(4 * S + 7, S, replace=False)
    seg_of_vertex = raw_ids[np.searchsorted(cuts, np.arange(n), side="right") - 1]
    owner = np.where(rng.random(S) < cover, rng.integers(0, max(K, 1), S), -1)
    if K:
        owner[rng.permutation(S)[:K]] = np.arange(K)
    centres = rng.uniform([-3, -2.5, 0.2], [3, 2.5, 2.2], (max(K, 1), 3)) if centres is None else np.asarray(centres, np.float64)
    xyz = rng.uniform([-4, -3, 0], [4, 3, 3], (n, 3))
    vertex_owner = owner[np.searchsorted(cuts, np.arange(n), side="right") - 1]
    inside = vertex_owner >= 0
    xyz[inside] = centres[vertex_owner[inside]] + rng.normal(0, 0.3, (int(inside.sum()), 3))
    angle = rng.uniform(0, 2 * np.pi)
    t = rng.uniform(-5, 5, 3) if translation is None else np.asarray(translation, np.float64)
    m = np.array([[np.cos(angle), np.sin(angle), 0, t[0]], [-np.sin(angle), np.cos(angle), 0, t[1]], [0, 0, 1, t[2]], [0, 0, 0, 1]])
    raw = (xyz - t) @ m[:3, :3]                                          # the aligned cloud lands at xyz
    mesh = np.concatenate([raw, rng.integers(0, 256, (n, 3))], 1).astype(np.float32)
    groups = [{"objectId": k, "label": labels[int(rng.integers(len(labels)))], "segments": raw_ids[owner == k].tolist()} for k in rng.permutation(K)]
    groups = [{**g, "objectId": int(g["objectId"])} for g in groups]
    return {"mesh": mesh, "seg_indices": seg_of_vertex.tolist(), "groups": groups, "label_map": dict(LABEL_MAP), "axis_align": m.reshape(16).tolist()}


def zero_ties(c):
    """an object of the case has both +0 and -0 as the extreme of an axis: its box is then compared with ``==``, not by bits"""
    xyz, ins = c["ex_vertices"][:, :3], c["ex_instances"]
    for k in np.unique(ins[ins > 0]):
        p = xyz[ins == k]
        for extreme in (p.min(0), p.max(0)):
            at = (p == extreme) & (extreme == 0)
            if ((at & np.signbit(p)).any(0) & (at & ~np.signbit(p)).any(0)).any():
                return True
    return False


def cases_present(name, c):
    """the case ``name`` of the fixture holds what DESIGN.md 6.7 says it holds"""
    from vdetr_amd import _lib
    tile = _lib.VDETR_EXPORT_TILE
    mesh, seg, groups, label_map, matrix = inputs_of(c)
    n, boxes = len(mesh), c["ex_bboxes"]
    assert mesh.dtype == np.float32 and mesh.shape == (n, 6) and len(seg) == n and np.isfinite(mesh).all()
    assert c["ex_vertices"].dtype == np.float32 and c["ex_labels"].dtype == np.uint32 and c["ex_instances"].dtype == np.uint32 and boxes.dtype == np.float64
    # the fixture rule: on these inputs the reference's own float32 vertices are the stated evaluation, fused or not
    assert c["ex_vertices"][:, :3].tobytes() == SR.align(mesh, matrix).tobytes() == SR.align_fused(mesh, matrix).tobytes(), name
    assert c["ex_vertices"][:, 3:].tobytes() == mesh[:, 3:].tobytes()
    assert not zero_ties(c)                                            # no case needs the == exemption: everything is compared by bits
    kept = np.isin(boxes[:, 6], SR.OBJ_CLASS_IDS)
    assert c["bbox"].tobytes() == boxes[kept].tobytes()
    if name != "donotcare":
        assert len(c["donotcare"]) == 0 and c["vert"].tobytes() == c["ex_vertices"].tobytes()
    if name == "single":
        assert n == 1 and boxes.shape == (1, 7) and (boxes[0, 3:6] == 0).all() and (boxes[0, :3] == c["ex_vertices"][0, :3]).all()
    if name.startswith("edge"):
        assert n == tile + {"edge_m1": -1, "edge": 0, "edge_p1": 1}[name]
        everywhere = [k for k in range(1, len(boxes) + 1) if all((c["ex_instances"][t:t + tile] == k).any() for t in range(0, n, tile))]
        assert everywhere, "an object with vertices in every tile"
    if name == "negative":
        lo, hi = boxes[:, :3] - boxes[:, 3:6] / 2, boxes[:, :3] + boxes[:, 3:6] / 2
        full = boxes[:, 3:6].min(1) > 0
        assert ((hi < 0).all(1) & full).any() and ((lo < 0) & (hi > 0)).all(1).any() and (lo > 0).all(1).any()
        assert np.abs(np.reshape(matrix, (4, 4))[:3, 3]).max() == 1e3
    if name == "shared_seg":
        named = {}
        for g in groups:
            for s in g["segments"]:
                named.setdefault(s, []).append(g)
        assert any(len({label_map[g["label"]] for g in gs}) > 1 for gs in named.values()), "a segment under two labels"
        assert any(len(gs) > 1 and len({g["label"] for g in gs}) == 1 and len({g["objectId"] for g in gs}) > 1 for gs in named.values())
        first = {}
        for g in groups:
            first.setdefault(g["label"], g)
        assert any(not g["segments"] for g in first.values()), "a label's first object without segments of its own: only the alias saves it"
        assert len({g["objectId"] for g in groups}) < len(groups), "an object id named twice"
    if name == "empty_object":
        assert set(SR.OBJ_CLASS_IDS) <= set(boxes[:, 6].astype(int).tolist())
        others = ~kept & (boxes[:, 6] != 0)
        assert others.sum() >= 3 and (boxes[others, 3:6] > 0).all()
        assert (boxes == 0).all(1).any(), "an object whose vertices all went to a later object"
        assert len(boxes) <= 64 and np.diff(np.flatnonzero(kept)).max() > 1
    if name == "unannotated":
        covered = (c["ex_labels"] != 0).mean()
        assert 0.25 < covered < 0.42 and ((c["ex_labels"] != 0) == (c["ex_instances"] != 0)).all()
    if name == "donotcare":
        drop = np.isin(c["ex_labels"], c["donotcare"])
        assert len(c["donotcare"]) >= 2 and 0 < drop.sum() < n and drop[0] and not drop[-1]
        assert c["vert"].tobytes() == c["ex_vertices"][~drop].tobytes() and c["ins_label"].tobytes() == c["ex_instances"][~drop].tobytes()
        assert np.isin(boxes[:, 6], c["donotcare"]).any()
        assert (c["sem_label"] == 0).any() and c["sem_label"].max() > c["donotcare"].max()    # kept: unannotated rows, labels past the ids
    if name == "identity":
        assert np.array_equal(np.reshape(matrix, (4, 4)), np.eye(4)) and c["ex_vertices"].tobytes() == mesh.tobytes()


def test_fixture_holds_the_cases_of_the_design():
    g = golden()
    assert set(CASES) == set(g)
    for name in CASES:
        assert set(g[name]) == set(INPUT_KEYS + EXPORT_KEYS + FILE_KEYS), name
        cases_present(name, g[name])
    assert os.path.getsize(GOLDEN) < 400 * 1024


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_bit_for_bit(name):
    c = golden()[name]
    args = inputs_of(c)
    mesh, labels, instances, boxes, object_label = SR.export(*args)
    assert same(mesh, c["ex_vertices"]) and same(labels, c["ex_labels"]) and same(instances, c["ex_instances"]) and same(boxes, c["ex_bboxes"])
    assert sorted(object_label) == c["ex_object_ids"].tolist() and [int(object_label[k]) for k in sorted(object_label)] == c["ex_object_labels"].tolist()
    for got, key in zip(SR.export_one_scan(*args, donotcare_ids=c["donotcare"].tolist()), FILE_KEYS):
        assert same(got, c[key]), (name, key)


@pytest.mark.parametrize("name", CASES)
def test_scan_tables_leave_what_the_reference_leaves(name):
    from vdetr_amd.scan_export import scan_tables
    c = golden()[name]
    _, seg, groups, label_map, matrix = inputs_of(c)
    before = [list(g["segments"]) for g in groups]
    t = scan_tables(seg, groups, label_map, None if name == "identity" else matrix)
    assert [g["segments"] for g in groups] == before                   # the caller's lists are not extended
    assert t.seg_indices.dtype == np.int32 and t.seg_label.dtype == np.int32 and t.seg_object.dtype == np.int32
    assert np.array_equal(t.seg_ids[t.seg_indices], seg)
    assert np.array_equal(t.seg_label[t.seg_indices], c["ex_labels"]) and np.array_equal(t.seg_object[t.seg_indices], c["ex_instances"])
    assert t.num_instances == len(c["ex_bboxes"]) == len(t.object_label)
    assert t.object_label[c["ex_object_ids"] - 1].tolist() == c["ex_object_labels"].tolist()
    assert t.axis_align.dtype == np.float64 and t.axis_align.tobytes() == np.reshape(matrix, (4, 4)).tobytes()


def test_scan_tables_on_generated_scans_equal_the_restatement():
    from vdetr_amd.scan_export import scan_tables
    rng = np.random.default_rng(5)
    for n, K, cover in ((1, 1, 1.0), (40, 0, 0.0), (700, 9, 0.5), (1500, 300, 1.0)):
        s = make_scan(rng, n, K, cover=cover)
        if K > 2:
            s["groups"][1]["segments"] = s["groups"][1]["segments"] + s["groups"][0]["segments"][:1]      # a segment under two objects
        _, labels, instances, boxes, object_label = SR.export(s["mesh"], s["seg_indices"], s["groups"], s["label_map"], s["axis_align"])
        t = scan_tables(s["seg_indices"], s["groups"], s["label_map"], s["axis_align"])
        assert np.array_equal(t.seg_label[t.seg_indices], labels) and np.array_equal(t.seg_object[t.seg_indices], instances)
        assert t.num_instances == K == len(boxes) and t.object_label.tolist() == [int(object_label[k]) for k in range(1, K + 1)]


def test_scan_tables_refuse_what_the_reference_fails_on():
    from vdetr_amd import _lib
    from vdetr_amd.scan_export import scan_tables
    seg = [5, 5, 9, 9, 2]
    group = lambda i, label, segs: {"objectId": i, "label": label, "segments": segs}  # noqa: E731
    ok = scan_tables(seg, [group(0, "chair", [5]), group(1, "table", [9, 2])], LABEL_MAP)
    assert ok.num_instances == 2 and ok.axis_align.tobytes() == np.eye(4).tobytes()
    with pytest.raises(KeyError, match="7"):
        scan_tables(seg, [group(0, "chair", [5, 7])], LABEL_MAP)        # no vertex carries segment 7
    with pytest.raises(ValueError, match="exactly 1"):
        scan_tables(seg, [group(0, "chair", [5]), group(2, "table", [9])], LABEL_MAP)
    with pytest.raises(ValueError, match="exactly 1"):
        scan_tables(seg, [group(-1, "chair", [5])], LABEL_MAP)          # object id 0: the reference would write row -1
    with pytest.raises(KeyError, match="sofa bed"):
        scan_tables(seg, [group(0, "sofa bed", [5])], LABEL_MAP)
    with pytest.raises(KeyError):
        scan_tables(seg, [group(0, "chair", [])], LABEL_MAP)            # an object that ends without segments
    K = _lib.VDETR_EXPORT_MAX_INSTANCES
    many = list(range(K + 1))
    assert scan_tables(many, [group(i, "chair", [i]) for i in range(K)], LABEL_MAP).num_instances == K
    with pytest.raises(ValueError, match="VDETR_EXPORT_MAX_INSTANCES"):
        scan_tables(many, [group(i, "chair", [i]) for i in range(K + 1)], LABEL_MAP)
    with pytest.raises(ValueError, match="one integer per vertex"):
        scan_tables([[1, 2]], [], LABEL_MAP)
