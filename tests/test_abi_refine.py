"""The refine entry points (csrc/refine.hip) in the header, the binding table and the product library, and the kernel's
resource use: no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gulon_refine_topk", "gulon_refine_topk_dev")


def test_refine_symbols_are_declared_bound_and_exported():
    from gulon_amd import native
    header = open(os.path.join(ROOT, "include", "gulon_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    L = native.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", header), name
        assert name in native.SIGNATURES and name in exported
        assert getattr(L, name).argtypes == native.SIGNATURES[name][1]
    # the device form: the host form's eleven arguments and the stream
    assert len(native.SIGNATURES["gulon_refine_topk"][1]) == 11
    assert len(native.SIGNATURES["gulon_refine_topk_dev"][1]) == 12
    assert L.gulon_abi_version() == 3


def test_package_exports_the_refined_index():
    import gulon_amd as g
    from gulon_amd import refine
    assert g.RefinedIndex is refine.RefinedIndex and g.refine_topk is refine.refine_topk
    assert callable(g.WordIndex.refined)
    for name in ("batch_query", "query", "batch_query_by_words", "query_by_word", "batch_query_raw"):
        assert callable(getattr(g.RefinedIndex, name)), name


def test_refine_kernels_use_no_scratch():
    """Both forms of refine_topk_kernel -- the tile loader, the register heap and the LDS heap with their replay -- keep
    everything in registers and LDS."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
           os.path.join(ROOT, "gulon_amd", "csrc", "refine.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    name, scratch = None, {}
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and "refine_topk_kernel" in name:
            scratch[name] = int(m.group(1))
    assert len(scratch) == 2, scratch
    assert set(scratch.values()) == {0}, scratch
