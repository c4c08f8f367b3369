"""The dropout generator (csrc/drop_stream.h) without a GPU.

First the numpy restatement (drop_stream_restatement.py), which tests/test_gpu_drop_stream.py holds the kernels' masks to, is
pinned to known answers: fmix32 as in MurmurHash3, and words of the keyed and the flat form computed apart from the library.
Then drop_stream_check.cpp, next to this file, runs the header itself on the host against the same answers and against a model
of its own: every hoisted form the kernels use (prefix once and a word per key, the `second` / `shift` selection of a head's draw,
pair words), the fold of the device state, the path without dropout.  Built with the address and undefined-behaviour sanitizers:
a stand-alone program, nothing is loaded into Python.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import drop_stream_restatement as R
from norm_cases import drop_threshold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "v-detr_amd", "csrc")
SEED, OFFSET = 0x01234567D746CDEE, 0x100000009


def test_restatement_known_answers():
    assert int(R.fmix32(1)) == 0x514E28B7 and int(R.fmix32(0xDEADBEEF)) == 0x0DE5C6A9
    g = R.stream(SEED, OFFSET)
    assert [int(v) for v in g] == [0xD746CDEE, 0x01234567, 9, 1]
    pre = R.prefix(g, 5, 1)
    assert (int(pre), int(R.word(pre, 3)), int(R.successor(R.word(pre, 3)))) == (0x6B7DE35E, 0x25B29DB6, 0x497B87EE)
    pre = R.prefix(g, 9, 129)
    assert (int(pre), int(R.word(pre, 17)), int(R.successor(R.word(pre, 17)))) == (0xF4DF84C5, 0xA4235674, 0x7AF32DE2)
    x = R.flat(g, 1000)
    assert (int(x), int(R.successor(x))) == (0xF2B2F064, 0x1E4E30E9)
    assert [drop_threshold(p) for p in (0.1, 0.3, 1e-6, 0.99999)] == [6554, 19661, 1, 65535]


def test_restatement_fold_and_masks_from_the_words():
    """the device state folds as seed ^= state.seed, offset += state.offset with the carry; each mask function picks the draws of the
    words above for its coordinates"""
    state = (0xFEDCBA9876543210, 0xFFFFFFFF)
    g = R.stream(SEED, OFFSET, state)
    assert [int(v) for v in g] == [0xD746CDEE ^ 0x76543210, 0x01234567 ^ 0xFEDCBA98, 8, 2]
    g, t = R.stream(SEED, OFFSET), drop_threshold(0.3)
    x, y = 0x25B29DB6, 0x497B87EE  # row 5, word 3: channels 12 .. 15
    assert R.keep_add_ln(6, 16, 0.3, g)[5, 12:].tolist() == [(x & 0xFFFF) >= t, (x >> 16) >= t, (y & 0xFFFF) >= t, (y >> 16) >= t]
    # channel 5, pair word 3: elements 6 and 7 of the channel's B N = 2 x 4 values, i.e. (b 1, i 2) and (b 1, i 3)
    assert R.keep_bn(2, 6, 4, 0.3, g)[1, 5, 2:].tolist() == [(x & 0xFFFF) >= t, (x >> 16) >= t]
    x, y = 0xF2B2F064, 0x1E4E30E9  # float4 number 1000
    assert R.keep_flat(4004, 0.3, g)[4000:].tolist() == [(x & 0xFFFF) >= t, (x >> 16) >= t, (y & 0xFFFF) >= t, (y >> 16) >= t]
    x, y = 0xA4235674, 0x7AF32DE2  # q 9, b 2, head group 1 (heads 4 .. 7), key 17
    m = R.keep_attention(3, 8, 10, 18, 0.3, g)
    assert m[2, 4:, 9, 17].tolist() == [(x & 0xFFFF) >= t, (x >> 16) >= t, (y & 0xFFFF) >= t, (y >> 16) >= t]
    assert m.shape == (3, 8, 10, 18) and R.keep_flat(8, 0.0, g).all()
    assert abs(float(np.mean(R.keep_add_ln(64, 256, 0.3, g))) - (65536 - t) / 65536) < 0.02


def _host_compiler():
    for name in ("g++", "c++", "clang++"):
        cxx = shutil.which(name)
        if cxx:
            return cxx
    raise AssertionError("no host C++ compiler (g++, c++, clang++) on PATH")


def test_header_on_the_host_against_the_model(tmp_path):
    exe = tmp_path / "drop_stream_check"
    cmd = [_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(HERE, "drop_stream_check.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    # (the program is linked with the sanitizer runtime itself; where the environment preloads another library first, the
    # runtime's link-order check would refuse to start it)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = ":".join(x for x in (env.get("ASAN_OPTIONS"), "verify_asan_link_order=0") if x)
    ran = subprocess.run([str(exe), "4000"], capture_output=True, text=True, env=env)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("drop stream ok: 4000 random cases"), ran.stdout


# one constant of the generator at a time, edited in a copy of the header as text
MUTANTS = {
    "major multiplier": ("0x9E3779B1u", "0x9E3779B3u"),
    "minor multiplier": ("0x27D4EB2Fu", "0x27D4EB2Du"),
    "word multiplier": ("0x165667B1u", "0x165667B3u"),
    "successor increment": ("0x9E3779B9u", "0x9E3779BBu"),
    "fmix32 multiplier": ("0xC2B2AE35u", "0xC2B2AE37u"),
    "fmix32 shift": ("x ^= x >> 13;", "x ^= x >> 14;"),
    "rate rounding": ("65536.0 + 0.5", "65536.0"),
    "fold of the offset": ("o += rng_state[1];", "o ^= rng_state[1];"),
}


@pytest.mark.parametrize("what", sorted(MUTANTS))
def test_host_check_catches_an_edited_constant(tmp_path, what):
    """the check is not vacuous: with one constant changed the program fails"""
    good, bad = MUTANTS[what]
    src = open(os.path.join(CSRC, "drop_stream.h")).read()
    assert src.count(good) >= 1, good
    (tmp_path / "drop_stream.h").write_text(src.replace(good, bad))
    exe = tmp_path / "drop_stream_bad"
    cmd = [_host_compiler(), "-std=c++17", "-O1", "-I", str(tmp_path), os.path.join(HERE, "drop_stream_check.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe), "50"], capture_output=True, text=True)
    assert ran.returncode == 1 and "drop stream check failed" in ran.stderr, ran.stdout + ran.stderr
