"""The index-view entry points (csrc/subset.hip) in the header, the binding table and the product library, and the
kernels' resource use: no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gulon_index_select_rows", "gulon_index_select_mask", "gulon_index_select_mask_dev", "gulon_index_view_size",
           "gulon_index_view_rows", "gulon_index_view_rows_dev", "gulon_index_view_batch_query",
           "gulon_index_view_batch_query_dev", "gulon_index_view_map_rows_dev")
KERNELS = ("mask_to_rows_count", "mask_to_rows_groups", "mask_to_rows_scatter", "gather_codesILi16E", "gather_codesILi4E",
           "gather_wcodes", "compose_map_kernel", "map_rows_kernel")


def test_subset_symbols_are_declared_bound_and_exported():
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
    # the view queries take what the plain ones take
    for form in ("batch_query", "batch_query_dev"):
        assert len(native.SIGNATURES["gulon_index_view_" + form][1]) == len(native.SIGNATURES["gulon_index_" + form][1])
    assert L.gulon_abi_version() == 3


def test_subset_is_in_the_makefile():
    assert "$(CSRC)/subset.hip" in open(os.path.join(ROOT, "Makefile")).read()


def test_subset_kernels_use_no_scratch():
    """The mask scan, the two gathers (both code-word widths) and the maps keep everything in registers and LDS."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
           os.path.join(ROOT, "gulon_amd", "csrc", "subset.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    name, scratch = None, {}
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    assert len(scratch) == len(KERNELS), scratch
    for k in KERNELS:
        assert sum(k in name for name in scratch) == 1, (k, sorted(scratch))
    assert set(scratch.values()) == {0}, scratch
