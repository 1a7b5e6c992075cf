"""The exact-index entry points (csrc/exact.hip) in the header, the binding table and the product library, and the
kernels' resource use: no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gulon_exact_index_create", "gulon_exact_index_destroy", "gulon_exact_index_batch_query",
           "gulon_exact_index_batch_query_dev", "gulon_exact_index_query_rows", "gulon_exact_index_query_rows_dev",
           "gulon_exact_index_tuning", "gulon_exact_index_stats")
KERNELS = ("exact_passILb1E", "exact_passILb0E", "exact_tauE", "exact_tau_allE", "exact_selectE", "exact_screenE",
           "exact_fill_emptyE", "exact_gather_rowsE", "exact_gather_queriesE", "exact_scatter_answersE")


def test_exact_symbols_are_declared_bound_and_exported():
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
    assert L.gulon_abi_version() == 3                        # purely additive


def test_exact_is_in_the_makefile():
    assert "$(CSRC)/exact.hip" in open(os.path.join(ROOT, "Makefile")).read()


def kernel_scratch(source):
    """{mangled kernel name: scratch bytes per lane} of one file of csrc, compiled for the device only."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
           os.path.join(ROOT, "gulon_amd", "csrc", source), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    name, scratch = None, {}
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    return scratch


def test_exact_kernels_use_no_scratch():
    """The distance tile with its sixteen accumulators and the per-wave append, the two radix selects and the LDS sort
    keep everything in registers."""
    scratch = kernel_scratch("exact.hip")
    assert len(scratch) == len(KERNELS), scratch
    for k in KERNELS:
        assert sum(k in name for name in scratch) == 1, (k, sorted(scratch))
    assert set(scratch.values()) == {0}, scratch


@pytest.mark.parametrize("source,kernels", [
    ("knn.hip", ("knn_kernelE",)),
    ("cosmul.hip", ("cosmul_exact_scanILi1E", "cosmul_exact_scanILi2E", "cosmul_exact_scanILi4E",
                    "cosmul_exact_scanILi8E", "cosmul_flat_scanILi4E", "cosmul_flat_scanILi16E"))])
def test_tile_and_list_users_use_no_scratch(source, kernels):
    """The other callers of the distance tile (exact.hpp) and of the WaveList helpers (common.hpp): sixteen accumulators
    beside up to sixteen lists, at 124 and 127 of the 128 registers that two waves per SIMD allow, spill nothing."""
    scratch = kernel_scratch(source)
    for k in kernels:
        hits = [name for name in scratch if k in name]
        assert len(hits) == 1, (k, sorted(scratch))
        assert scratch[hits[0]] == 0, (hits[0], scratch)
