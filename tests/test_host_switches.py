"""The package's environment switches are a fixed, documented set: an A/B path whose loser was never kept does not come back
through a new VDETR_* read without this list (and INTEGRATION.md §7b) changing with it.  The native library has none at all."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEPT = {
    # parity references that tests flip
    "VDETR_BWD_KERNEL", "VDETR_BWD_FUSED", "VDETR_SELF_FWD", "VDETR_DEFER_COMBINE", "VDETR_KV_PREPACK", "VDETR_ROWBLOCK",
    "VDETR_ROWBLOCK_BWD", "VDETR_FFN0_FUSED", "VDETR_HEADS_FUSED", "VDETR_POS_FUSED", "VDETR_DEFER_HEADS", "VDETR_CPB_FUSED",
    "VDETR_BWD_ASYNC_TABLE",
    # read by bench.py / the side-grid sweep
    "VDETR_FWD_KERNEL", "VDETR_BWD_ASYNC_GRID",
    # safety: the rocblas_sgemm_batched path
    "VDETR_PTR_BATCH",
    # not A/B switches
    "VDETR_TS_PROBE", "VDETR_CACHE_DIR", "VDETR_TUNABLEOP_SAVE", "VDETR_EXTRA_HIPCC_FLAGS", "VDETR_SKIP_CODE_CHECK",
    # backbone execution modes (each is a case of tests/test_gpu_sparse.py)
    "VDETR_SP_MODE", "VDETR_SP_IM2COL",
}

_READ = re.compile(r"""os\.(?:environ\.get\(|environ\[|getenv\()\s*["'](VDETR_[A-Z0-9_]+)["']""")


def _names_read():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "v-detr_amd", "*.py")):
        with open(path) as fh:
            names.update(_READ.findall(fh.read()))
    return names


def test_package_reads_exactly_the_kept_switches():
    names = _names_read()
    assert names == KEPT, f"read but not kept: {sorted(names - KEPT)}; kept but not read: {sorted(KEPT - names)}"


def test_kept_switches_are_documented():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        doc = fh.read()
    missing = sorted(n for n in KEPT if not re.search(re.escape(n) + r"(?![A-Z0-9_])", doc))
    assert not missing, f"not in INTEGRATION.md: {missing}"


def test_native_library_reads_no_environment():
    """v-detr_amd/csrc: no getenv and no VDETR_AB(name, default) site, in code or comment: every launch decision of the library is
    written out, and vdetr_ab_switches() returns 0 unconditionally."""
    paths = sorted(glob.glob(os.path.join(ROOT, "v-detr_amd", "csrc", "*")))
    assert len(paths) > 20, paths
    hits = []
    for path in paths:
        with open(path, errors="replace") as fh:
            for no, line in enumerate(fh, 1):
                if "getenv" in line or "VDETR_AB" in line:
                    hits.append(f"{os.path.basename(path)}:{no}: {line.strip()[:100]}")
    assert not hits, "\n".join(hits)
