"""The C-ABI library loads on a CPU-only box and exports exactly the symbols
include/gulon_hip.h declares (no compute calls here)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols(hooks=False):
    """Entry points include/gulon_hip.h declares: the product's, or (hooks=True) only those under GULON_TEST_HOOKS."""
    txt = open(os.path.join(ROOT, "include", "gulon_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    guarded = "".join(re.findall(r"#ifdef GULON_TEST_HOOKS(.*?)#endif", txt, flags=re.S))
    if hooks:
        txt = guarded
    else:
        txt = re.sub(r"#ifdef GULON_TEST_HOOKS.*?#endif", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gulon_[a-z0-9_]+)\s*\(", txt)))


def test_header_matches_binding_table():
    from gulon_amd import native
    assert _header_symbols() == sorted(native.SIGNATURES)


def test_library_exports_every_declared_symbol():
    from gulon_amd import native
    assert os.path.exists(native.LIB_PATH), "run `make` / __graft_entry__.build() first"
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    missing = [s for s in _header_symbols() if s not in exported]
    assert not missing, missing
    extra = sorted(s for s in exported if s.startswith("gulon_") and s not in _header_symbols())
    assert not extra, extra
    L = native.lib()
    assert L.gulon_abi_version() == 3


def test_product_library_carries_no_test_hooks():
    """Self-tests are in libgulon_hip_testhooks.so only."""
    from gulon_amd import native
    hooks = _header_symbols(hooks=True)
    assert hooks == sorted(native.TEST_HOOK_SIGNATURES) and len(hooks) == 7
    def exported(path):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        return {l.split()[-1] for l in out.splitlines() if " T " in l}
    prod, hk = exported(native.LIB_PATH), exported(native.HOOKS_LIB_PATH)
    assert not [s for s in prod if "selftest" in s]
    assert set(hooks) <= hk and {s for s in prod if s.startswith("gulon_")} <= hk
    sym = subprocess.check_output(["nm", "-C", native.LIB_PATH], text=True)
    assert "update_fused" not in sym                       # the dropped fused k-means update stays out of the product


def test_host_only_entry_points_match_oracle(oracle):
    """Coder / subvectors are host integer logic inside the library: compare with the oracle."""
    import gulon_amd as g
    for d, m in [(50, 25), (128, 16), (300, 32), (1024, 64), (7, 3)]:
        fr, un = g.subvector_bounds(d, m)
        ofr, oun = oracle.subvectors(d, m)
        assert fr.tolist() == ofr.tolist() and un.tolist() == oun.tolist()
    rng = np.random.default_rng(0)
    for k in (1, 2, 4, 5, 16, 17, 256, 257, 1024, 4096, 65536):
        w = g.width_for_clusters(k)
        assert w == oracle.coder_width_for_clusters(k)
        idx = rng.integers(0, k, 37).astype(np.int32)
        c = g.Coder(w, 37)
        code = c.build_code(idx)
        assert np.array_equal(code, oracle.coder_build(w, idx))
        assert np.array_equal(c.get_indices(code), idx)
    with pytest.raises(ValueError):
        g.width_for_clusters(65537)                      # "too many clusters"
    with pytest.raises(ValueError):
        g.Coder(3, 5)                                    # "unsupported width"


def test_product_path_has_no_oracle_import():
    """gulon_amd must never import or call anything under oracle/."""
    pkg = os.path.join(ROOT, "gulon_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f
                assert "gulon_oracle" not in txt and "go_" + "kmeans" not in txt, f


def test_filter_kernels_keep_their_code_words_in_registers():
    """Every instantiation of the quantized filter's kernel compiles without scratch memory.  (Round 2 refactored its
    inner loop into a lambda that overwrote a captured code word: the multi-word forms -- m = 32, 48, 64 ... -- then kept
    that word in scratch, 32 bytes per lane, and BASELINE config 5 ran 13 % slower until a profile showed it.)"""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
           os.path.join(ROOT, "gulon_amd", "csrc", "filter.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    name, seen, spilled = None, 0, []
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and "filter_kernel" in name:
            seen += 1
            if int(m.group(1)) != 0:
                spilled.append((name, int(m.group(1))))
    assert seen >= 24, seen
    assert not spilled, spilled
