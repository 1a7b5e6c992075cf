"""The entry point of the grouped index's offset queries (csrc/grouped_offset.hip) in the header, the binding
table and the product library; the header's stream contract untouched by it; the source in the Makefile, compiled without
test hooks and free of scratch; the methods the package gains.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import stream_contract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gulon_amd", "csrc")
NAME = "gulon_grouped_index_query_offset"
KERNEL = "grouped_offset_scan"


def test_symbol_is_declared_bound_and_exported():
    from gulon_amd import native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gulon_hip.h")).read(), flags=re.S)
    plain = re.sub(r"#ifdef GULON_TEST_HOOKS.*?#endif", "", header, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    L = native.lib()
    args = re.search(r"\bint32_t\s+" + NAME + r"\s*\(([^)]*)\)", plain).group(1)
    assert len(args.split(",")) == len(native.SIGNATURES[NAME][1]) == 11
    assert NAME in exported and getattr(L, NAME).argtypes == native.SIGNATURES[NAME][1]
    assert L.gulon_abi_version() == 3
    assert not [n for n in native.TEST_HOOK_SIGNATURES if "grouped_index_query_offset" in n]


def test_the_stream_contract_of_the_header_is_unchanged():
    """The host form only: no stream parameter, no _dev name, no d_ pointer -- with or without the declaration the
    header's stream entry points (40) and its stream-less device-pointer entry points are the same."""
    text = stream_contract.header_text()
    without = re.sub(r"int32_t\s+" + NAME + r"\s*\([^)]*\)\s*;", "", text)
    assert without != text
    assert stream_contract.stream_entry_points(text) == stream_contract.stream_entry_points(without)
    assert len(stream_contract.stream_entry_points(text)) == 40
    assert stream_contract.device_pointer_entry_points_without_stream(text) \
        == stream_contract.device_pointer_entry_points_without_stream(without)
    args = re.search(NAME + r"\s*\(([^)]*)\)", text).group(1)
    assert "stream" not in args and not re.search(r"\bd_\w+", args)


def test_source_is_in_the_makefile_without_hooks():
    make = open(os.path.join(ROOT, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    hdrs = re.search(r"^HDRS = (.*)$", make, flags=re.M).group(1).split()
    assert "$(CSRC)/grouped_offset.hip" in srcs
    assert "$(CSRC)/grouped_offset.hpp" in hdrs
    assert "grouped_offset" not in re.search(r"^HOOKED = (.*)$", make, flags=re.M).group(1).split()
    for name in ("grouped_offset.hip", "grouped_offset.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "GULON_TEST_HOOKS" not in text and "getenv" not in text, name


def test_the_kernel_is_in_the_new_file_only():
    text = open(os.path.join(CSRC, "grouped_offset.hip")).read()
    assert re.search(r"__global__[^;{]*\b" + KERNEL + r"\(", text)
    others = [f for f in sorted(os.listdir(CSRC)) if f != "grouped_offset.hip" and
              re.search(r"__global__[^;{]*\b" + KERNEL + r"\(", open(os.path.join(CSRC, f)).read())]
    assert not others, others
    for shared in ("group_pair_table(", "wave_offer(", "launch_merge("):       # the pieces it is put together from
        assert shared in text, shared
    grouped = open(os.path.join(CSRC, "grouped.hip")).read()
    assert "launch_grouped_offset(" in grouped and "check_offset_host(" in grouped and "coarse_stage(c, /*all_literal=*/true)" in grouped


def test_the_kernel_has_two_instantiations_and_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
           os.path.join(CSRC, "grouped_offset.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    name, scratch, lds = None, {}, {}
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and name:
            lds[name] = int(m.group(1))
    assert len(scratch) == 2 and all(KERNEL in n for n in scratch), scratch      # VEC = 4 and VEC = 16
    assert not any(scratch.values()) and not any(lds.values()), (scratch, lds)   # (its LDS is the launch's, as gq_group_scan's)


def test_a_null_handle_is_an_argument_error_before_the_device():
    from gulon_amd import native
    f, i = np.zeros(4, np.float32), np.zeros(4, np.int32)
    assert native.lib().gulon_grouped_index_query_offset(None, f, 1, 1, 0, 1, f, None, i, f, i) \
        == native.ERR_INVALID_ARGUMENT


def test_the_package_gains_the_methods_and_keeps_its_refusals():
    import gulon_amd as g
    from gulon_amd import cli, csls
    assert callable(g.GroupedIndex.batch_query_offset_raw) and callable(g.GroupedIndex.batch_query_offset)
    grouped = g.GroupedIndex.__new__(g.GroupedIndex)             # no handle behind it: only its type is looked at
    assert csls._vector_side(grouped) == ("grouped", grouped)
    with pytest.raises(ValueError, match="the source of csls_offsets is an exact index"):
        g.csls_offsets(grouped, grouped)
    with pytest.raises(NotImplementedError):
        csls._vector_side(object())
    assert cli.TranslateConfig("i", "s") == cli.TranslateConfig("i", "s", None, None, "nn", 10, 10, (1, 5, 10), False,
                                                                None, False, None)
