"""The sparse key (csrc/sparse_key.h) without a GPU.

sparse_key_check.cpp, next to this file, runs the header itself on the host against restatements of its own: the codec at the
edges of every field, key order against (batch, x, y, z) order, the field move with offsets up to INT_MAX and INT_MIN (no carry,
-1 exactly outside, -1 for a negative key), the lower bound and the look-up against std::lower_bound.  Built with the address
and undefined-behaviour sanitizers: a stand-alone program, nothing is loaded into Python.  The keys it prints for a fixed list of
coordinates are then held against the two Python statements of the layout, ``sparse_ops.pack_keys`` and the oracle's.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import sparse_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "v-detr_amd", "csrc")


def _host_compiler():
    for name in ("g++", "c++", "clang++"):
        cxx = shutil.which(name)
        if cxx:
            return cxx
    raise AssertionError("no host C++ compiler (g++, c++, clang++) on PATH")


def test_header_on_the_host_against_the_restatements(tmp_path):
    from vdetr_amd import sparse_ops as S
    exe = tmp_path / "sparse_key_check"
    cmd = [_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(HERE, "sparse_key_check.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    # (the program is linked with the sanitizer runtime itself; where the environment preloads another library first, the
    # runtime's link-order check would refuse to start it)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = ":".join(x for x in (env.get("ASAN_OPTIONS"), "verify_asan_link_order=0") if x)
    ran = subprocess.run([str(exe), "4000"], capture_output=True, text=True, env=env)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    lines = ran.stdout.splitlines()
    assert lines[-1].startswith("sparse key ok: 4000 random pairs"), ran.stdout

    # the fixed coordinate list: row b x y z | key, its batch, the floor of its scene, the origin site of its scene
    rows = np.array([[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("row ")], dtype=np.int64)
    assert rows.shape == (16, 8)
    coords, keys, batch, floor, origin = rows[:, :4], rows[:, 4], rows[:, 5], rows[:, 6], rows[:, 7]
    assert int(coords[:, 1:].min()) == -32768 and int(coords[:, 1:].max()) == 32767 and int(coords[:, 0].max()) == 32767
    assert np.array_equal(O.pack_keys_np(coords), keys)
    assert np.array_equal(S.pack_keys(torch.from_numpy(coords)).numpy(), keys)
    assert np.array_equal(S.unpack_keys(torch.from_numpy(keys)).numpy(), coords.astype(np.int32))
    assert np.array_equal(O.unpack_keys_np(keys), coords)
    assert np.array_equal(S.key_batch(torch.from_numpy(keys)).numpy(), batch) and np.array_equal(batch, coords[:, 0])
    last = int(coords[:, 0].max())  # 32767: the floors of scenes 0 .. 32767 (the next one would not fit 64 bits)
    floors, origins = S.scene_floor_keys(last, "cpu"), S.origin_keys(last + 1, "cpu")
    assert floors.dtype == torch.int64 and floors.shape == (last + 1,) and origins.dtype == torch.int64 and origins.shape == (last + 1,)
    assert np.array_equal(floors.numpy()[coords[:, 0]], floor)
    assert np.array_equal(origins.numpy()[coords[:, 0]], origin)
    # ... the floors are what scene_segments searches for: the rows of every scene of a sorted key vector
    few = np.sort(keys[coords[:, 0] <= 300])
    seg = S.scene_segments(torch.from_numpy(few), 301).numpy()
    assert seg.dtype == np.int32 and np.array_equal(np.diff(seg), np.bincount(few >> 48, minlength=301)) and seg[-1] == len(few) == 12


# one statement of the header at a time, edited in a copy of it as text
MUTANTS = {
    "bias": ("kKeyBias = 32768", "kKeyBias = 32767"),
    "batch shift": ("kKeyBatchShift = 48", "kKeyBatchShift = 47"),
    "x shift": ("kKeyXShift = 32", "kKeyXShift = 31"),
    "field end": ("kKeyFieldEnd = 65536", "kKeyFieldEnd = 65535"),
    "negative key of key_shift": ("const bool ok = key >= 0 && x >= 0", "const bool ok = x >= 0"),
    "lower bound comparison": ("if (keys[mid] < key)", "if (keys[mid] <= key)"),
    "row tested by key_find": ("keys[lo] == key", "keys[lo - 1] == key"),
}


@pytest.mark.parametrize("what", sorted(MUTANTS))
def test_host_check_catches_an_edited_header(tmp_path, what):
    """the check is not vacuous: with one statement changed the program fails"""
    good, bad = MUTANTS[what]
    src = open(os.path.join(CSRC, "sparse_key.h")).read()
    assert src.count(good) == 1, good
    (tmp_path / "sparse_key.h").write_text(src.replace(good, bad))
    exe = tmp_path / "sparse_key_bad"
    cmd = [_host_compiler(), "-std=c++17", "-O1", "-I", str(tmp_path), os.path.join(HERE, "sparse_key_check.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe), "50"], capture_output=True, text=True)
    assert ran.returncode == 1 and "sparse key check failed" in ran.stderr, ran.stdout + ran.stderr
