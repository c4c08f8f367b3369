"""Builds ``lib/libvdetr_hip.so`` (gfx950 code objects + the C-ABI of include/vdetr_hip.h) with hipcc.

hipcc cross-compiles without a GPU, so this runs in the CPU-only build container; the resulting shared
object travels to the GPU box with the repo snapshot (it is git-ignored, not gpurun-ignored).
"""
import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libvdetr_hip.so")
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-ffp-contract=off", f"--offload-arch={ARCH}"]
FLAGS += os.environ.get("VDETR_EXTRA_HIPCC_FLAGS", "").split()  # extra compiler flags (-DVDETR_SQDIST_ORDER=1 ...); part of the fingerprint


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _fingerprint():
    h = hashlib.sha256((" ".join(FLAGS) + "|noslp:" + ",".join(NO_SLP)).encode())
    root = os.path.dirname(HERE)
    for f in sorted(os.listdir(CSRC)) + [os.path.join(root, "include", "vdetr_hip.h")]:
        p = f if os.path.isabs(f) else os.path.join(CSRC, f)
        with open(p, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


# Packed fp32 multiply / fma whose SECOND source is high-broadcast: op_sel[1] = 1 (the low result lane reads the high
# register of the source pair) together with op_sel_hi[1] = 1 (so does the high lane; 1 is the default when op_sel_hi is not
# printed), e.g. `v_pk_mul_f32 v[0:1], v[2:3], v[4:5] op_sel:[0,1]` — what hipcc emits for `float2 * float2[1]`.  A round-2
# kernel built around that form produced wrong sums on MI355X / ROCm 7.2 and right ones with scalar multiplies (DESIGN.md
# 4.4b).  tools/probes/pk_opsel_probe.hip has since shown that the hardware executes every op_sel form of v_pk_mul / add /
# fma_f32 exactly (16-wave workgroups on every CU, LDS traffic around them, 0 mismatches), so the encoding alone is not the
# cause and the real one is still unknown; until it is, the form the failing kernel used stays out of the library.
# (Other broadcast forms, e.g. the first source high-broadcast in attn_fwd_kernel, are covered by the parity tests.)
_PACKED = r"\b(v_pk_(?:mul|fma)_f32)\b([^\n/]*)"
NO_SLP = ("criterion.hip", "heads.hip", "rowblock_pos.hip")  # -fno-slp-vectorize: their scalar float code was being packed into the form above


def _hi_broadcast(operands, src=1):
    import re
    sel = re.search(r"op_sel:\[([01,]+)\]", operands)
    if not sel:
        return False
    lo = [int(v) for v in sel.group(1).split(",")]
    hi_m = re.search(r"op_sel_hi:\[([01,]+)\]", operands)
    hi = [int(v) for v in hi_m.group(1).split(",")] if hi_m else [1] * len(lo)
    return len(lo) > src and lo[src] == 1 and hi[src] == 1


def check_code_objects(lib, verbose=False):
    """Disassembles every gfx950 code object of `lib` and raises if a hazardous packed-math encoding is present."""
    import re
    import tempfile
    cands = [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-objdump"), shutil.which("llvm-objdump"),
             "/opt/rocm/lib/llvm/bin/llvm-objdump"]
    hipcc = shutil.which("hipcc")
    if hipcc:  # a ROCm found through PATH only: its llvm sits next to bin/
        cands.append(os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "llvm-objdump"))
    objdump = next((c for c in cands if c and os.path.exists(c)), None)
    if objdump is None:
        # attn_bwd_box4.hip's in-flight atomic result is only safe because this scan proves that nothing touches its register
        # before the wait: a build that cannot be checked is not shipped (VDETR_SKIP_CODE_CHECK=1 overrides, at the builder's risk)
        if os.environ.get("VDETR_SKIP_CODE_CHECK") == "1":
            print("[vdetr build] llvm-objdump not found: code objects NOT checked (VDETR_SKIP_CODE_CHECK=1)", file=sys.stderr)
            return 0
        raise RuntimeError("llvm-objdump not found (looked in $ROCM_PATH/lib/llvm/bin, PATH and next to hipcc): the code-object "
                           "check cannot run; set ROCM_PATH, or VDETR_SKIP_CODE_CHECK=1 to build unchecked")
    hits, nobj = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, "lib.so")
        shutil.copy(lib, copy)
        subprocess.check_call([objdump, "--offloading", copy], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=tmp)
        for f in sorted(os.listdir(tmp)):
            if ARCH not in f:
                continue
            nobj += 1
            asm = subprocess.run([objdump, "-d", os.path.join(tmp, f)], capture_output=True, text=True).stdout
            kernel = "?"
            pending = None  # (register number, kernel) of an asm `global_atomic_add vN, v[a:b], vM, off` whose result is in flight
            for line in asm.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
                if m:
                    kernel, pending = m.group(1), None
                    continue
                m = re.search(_PACKED, line)
                if m and _hi_broadcast(m.group(2)):
                    hits.append(f"{kernel}: {m.group(1)}{m.group(2).rstrip()}")
                # The table-gradient kernels draw their next query with a returning atomic written as asm, so that nothing waits
                # for it at once (attn_bwd_box4.hip).  The compiler does not know that its destination register is still in flight:
                # nothing may touch that register before the `s_waitcnt vmcnt(0)` that precedes its one use.
                a = re.search(r"\bglobal_atomic_add\s+v(\d+),\s*v\[\d+:\d+\],\s*v\d+,\s*off", line)
                if a:
                    pending = int(a.group(1))
                elif pending is not None:
                    if re.search(r"s_waitcnt[^\n]*vmcnt\(0\)", line):
                        pending = None
                    else:
                        body = line.split("//")[0]
                        regs = {int(r) for r in re.findall(r"\bv(\d+)\b", body)}
                        for lo, hi in re.findall(r"\bv\[(\d+):(\d+)\]", body):
                            regs.update(range(int(lo), int(hi) + 1))
                        if pending in regs:
                            hits.append(f"{kernel}: v{pending} (result of an asm atomic still in flight) touched by: {body.strip()[:80]}")
                            pending = None
    if nobj == 0:
        raise RuntimeError(f"no {ARCH} code object found in {lib}")
    if hits:
        raise RuntimeError("code-object check failed (packed fp32 multiply with a high-broadcast second source, DESIGN.md 4.4b; or a "
                           "register of an in-flight asm atomic touched early, attn_bwd_box4.hip):\n  " + "\n  ".join(hits[:20]))
    if verbose:
        print(f"checked {nobj} {ARCH} code objects: no v_pk_mul/fma_f32 with a high-broadcast second source")
    return nobj


def build(force=False, verbose=False):
    """Compile if the sources changed since the last build.  Returns the path of the shared object."""
    os.makedirs(LIBDIR, exist_ok=True)
    stamp = os.path.join(LIBDIR, ".fingerprint")
    fp = _fingerprint()
    if not force and os.path.exists(LIB) and os.path.exists(stamp) and open(stamp).read() == fp:
        return LIB
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libvdetr_hip.so")
    objs = []
    procs = []
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    for src in sources():
        obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        extra = ["-fno-slp-vectorize"] if os.path.basename(src) in NO_SLP else []
        cmd = [hipcc, *FLAGS, *extra, "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{out.decode()}")
        if verbose and out:
            print(out.decode())
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB, *objs]
    subprocess.check_call(cmd)
    check_code_objects(LIB, verbose)
    with open(stamp, "w") as fh:
        fh.write(fp)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
