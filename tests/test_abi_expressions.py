"""The expression entry points (csrc/compose.hip) in the header, the binding table and the product library, the names
the package exports, and the kernels' resource use: no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gulon_index_compose_rows", "gulon_index_compose_rows_dev", "gulon_grouped_index_compose_rows",
           "gulon_grouped_index_compose_rows_dev", "gulon_index_query_terms", "gulon_index_query_terms_dev",
           "gulon_grouped_index_query_terms", "gulon_grouped_index_query_terms_dev")


def test_expression_symbols_are_declared_bound_and_exported():
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
    # a device form: the host form's arguments and the stream
    for name in SYMBOLS[::2]:
        assert len(native.SIGNATURES[name + "_dev"][1]) == len(native.SIGNATURES[name][1]) + 1, name
    # the argument counts of the header's declarations
    for name in SYMBOLS:
        args = re.search(r"\bint32_t\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len(args.split(",")) == len(native.SIGNATURES[name][1]), name
    assert L.gulon_abi_version() == 3


def test_package_exports_the_expression_names():
    import gulon_amd as g
    from gulon_amd import expressions
    for name in ("Expression", "Term", "compose_reference", "parse_expression", "partition_by_operands"):
        assert getattr(g, name) is getattr(expressions, name) and name in g.__all__
    for cls, names in ((g.PQIndex, ("compose_rows", "batch_query_terms")),
                       (g.SortedIndex, ("batch_query_expressions", "compose_rows")),
                       (g.GroupedIndex, ("batch_query_expressions", "compose_rows")),
                       (g.WordIndex, ("batch_query_expressions", "query_expression")),
                       (g.RefinedIndex, ("batch_query_expressions", "query_expression"))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)


def test_expression_kernels_use_no_scratch():
    """Every form of compose_rows_kernel keeps its running sums in registers (the widest holds 64 of them per thread),
    and drop_rows_kernel compacts with ballots alone."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
           os.path.join(ROOT, "gulon_amd", "csrc", "compose.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    name, scratch = None, {}
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and ("compose_rows_kernel" in name or "drop_rows_kernel" in name):
            scratch[name] = int(m.group(1))
    assert len([n for n in scratch if "compose_rows_kernel" in n]) == 4, scratch
    assert len([n for n in scratch if "drop_rows_kernel" in n]) == 1, scratch
    assert set(scratch.values()) == {0}, scratch
