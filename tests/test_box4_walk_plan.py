"""The routing of attn_bwd_box4.hip's quad walk (csrc/box4_walk.h: parity word, flushing half, quad cut) on the host.

box4_walk_check.cpp, next to this file, walks end masks through the very functions the kernel calls and holds them to a
slot-by-slot model: every slot in exactly one half of the tile and flushed from it, never two live groups in one half, every
group flushed once and in slot order into a half that was empty when it entered.  All 16 end patterns of a quad x both
incoming parities, and a few thousand random masks.  Built with the address and undefined-behaviour sanitizers: a stand-alone
program, nothing is loaded into Python.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _host_compiler():
    for name in ("g++", "c++", "clang++"):
        cxx = shutil.which(name)
        if cxx:
            return cxx
    raise AssertionError("no host C++ compiler (g++, c++, clang++) on PATH")


def test_walk_routing_against_the_slot_model(tmp_path):
    exe = tmp_path / "box4_walk_check"
    cmd = [_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "v-detr_amd", "csrc"), os.path.join(HERE, "box4_walk_check.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    # (the program is linked with the sanitizer runtime itself; where the environment preloads another library first, the
    # runtime's link-order check would refuse to start it)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = ":".join(x for x in (env.get("ASAN_OPTIONS"), "verify_asan_link_order=0") if x)
    ran = subprocess.run([str(exe), "4000"], capture_output=True, text=True, env=env)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("box4 walk ok:"), ran.stdout
    assert int(ran.stdout.split()[3]) >= 4000 + 16 * 2


def test_walk_check_catches_a_missing_cut(tmp_path):
    """the model is not vacuous: with the quad cut taken out (a one-line edit of a copy of the header) groups g and g + 2 meet in a half and the program fails"""
    src = open(os.path.join(ROOT, "v-detr_amd", "csrc", "box4_walk.h")).read()
    good = "return in2 ? __builtin_ctz(in2) : -1;"
    assert src.count(good) == 1
    (tmp_path / "box4_walk.h").write_text(src.replace(good, "return (void)in2, -1;"))
    exe = tmp_path / "box4_walk_bad"
    cmd = [_host_compiler(), "-std=c++17", "-O1", "-I", str(tmp_path), os.path.join(HERE, "box4_walk_check.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe), "50"], capture_output=True, text=True)
    assert ran.returncode == 1 and "two live groups in one half" in ran.stderr
