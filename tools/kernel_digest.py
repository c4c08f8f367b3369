#!/usr/bin/env python3
"""Per-kernel digest of the gfx950 code objects of a libvdetr_hip.so: which kernels a change added, removed or altered.

    python tools/kernel_digest.py LIB            # one line per kernel: instructions, registers, LDS, scratch
    python tools/kernel_digest.py PARENT BRANCH  # kernels gone / new / changed between two builds; exit status 1 if any is
                                                 # new or changed

A kernel's digest is the sha1 of its disassembled instruction text (addresses, `//` comments and the padding after the last
instruction stripped) plus the resource figures of its metadata note (VGPRs, SGPRs, LDS, scratch, spills).  A refactor of the
host half of the library must leave every surviving kernel's digest as it was.  Needs no GPU."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ARCH = "gfx950"
_LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
_FIGURES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
            ".vgpr_spill_count", ".sgpr_spill_count")


def _tool(name):
    path = os.path.join(_LLVM, name)
    return path if os.path.exists(path) else shutil.which(name) or name


def _figures(notes):
    """{kernel symbol: {figure: value}} out of the AMDGPU metadata that `llvm-readelf --notes` prints"""
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
        block = "  - .agpr_count:" + block
        name = re.search(r"^\s*\.name:\s*(\S+)", block, re.M)
        if name:
            out[name.group(1).strip("'\"")] = {k: int(v) for k, v in re.findall(r"^\s*-?\s*(\.[a-z_]+):\s*(\d+)\s*$", block, re.M) if k in _FIGURES}
    return out


def digest(lib):
    """{kernel symbol: (sha1 of the instruction text, instruction count, resource figures)}"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, "lib.so")
        shutil.copy(lib, copy)
        subprocess.check_call([_tool("llvm-objdump"), "--offloading", copy], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=tmp)
        for f in sorted(os.listdir(tmp)):
            if ARCH not in f:
                continue
            obj = os.path.join(tmp, f)
            figures = _figures(subprocess.run([_tool("llvm-readelf"), "--notes", obj], capture_output=True, text=True).stdout)
            asm = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", obj], capture_output=True, text=True).stdout
            name, h, n = None, None, 0
            for line in asm.splitlines() + ["0 <>:"]:
                m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
                if m:
                    if name:
                        out[name] = (h.hexdigest(), n, figures.get(name, {}))
                    name, h, n = m.group(1), hashlib.sha1(), 0
                    continue
                body = line.split("//")[0].strip()
                if name and body and body != "..." and "file format" not in body and not body.startswith("Disassembly of"):
                    h.update(body.encode() + b"\n")
                    n += 1
    if not out:
        raise SystemExit(f"no {ARCH} kernel found in {lib}")
    return out


def _fmt(fig):
    return " ".join(f"{k[1:]}={fig[k]}" for k in _FIGURES if k in fig)


def main(argv):
    if len(argv) not in (2, 3):
        raise SystemExit(__doc__)
    a = digest(argv[1])
    if len(argv) == 2:
        print(f"{len(a)} kernels, {os.path.getsize(argv[1])} bytes")
        for k in sorted(a):
            print(a[k][1], k, _fmt(a[k][2]))
        return 0
    b = digest(argv[2])
    gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    code = sorted(k for k in a if k in b and a[k][:2] != b[k][:2])
    res = sorted(k for k in a if k in b and a[k][2] != b[k][2])
    print(f"parent {len(a)} kernels / {os.path.getsize(argv[1])} bytes, branch {len(b)} / {os.path.getsize(argv[2])}: "
          f"gone {len(gone)}, new {len(new)}, code changed {len(code)}, resources changed {len(res)}")
    for k in gone:
        print("GONE", a[k][1], k)
    for k in new:
        print("NEW", b[k][1], k)
    for k in code:
        print("CODE", a[k][1], b[k][1], k)
    for k in res:
        print("RESOURCES", k, "|", _fmt(a[k][2]), "->", _fmt(b[k][2]))
    return 1 if new or code or res else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
