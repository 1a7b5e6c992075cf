"""The index-update entry points (csrc/update.hip) in the header, the binding table and the product library, and the
kernels' resource use: no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gulon_index_encode_dataset", "gulon_index_merge", "gulon_index_get_codes")
KERNELS = ("store_codesILi16E", "store_codesILi4E", "store_wcodes", "merge_codesILi16E", "merge_codesILi4E",
           "merge_wcodes", "unblock_codes", "unblock_wcodes")


def test_update_symbols_are_declared_bound_and_exported():
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
    assert L.gulon_abi_version() == 3                        # purely additive, as for views


def test_update_is_in_the_makefile():
    assert "$(CSRC)/update.hip" in open(os.path.join(ROOT, "Makefile")).read()


def test_update_kernels_use_no_scratch():
    """The stores of fresh assignments, the two-source gathers (both code-word widths) and the un-blocking read keep
    everything in registers."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
           os.path.join(ROOT, "gulon_amd", "csrc", "update.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
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
