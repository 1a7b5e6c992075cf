"""The entry points of the offset queries and of the mean similarity (csrc/offset.hip) in the header, the
binding table and the product library; the source in the Makefile, compiled without test hooks, and its scan kernels
free of scratch; the names the package exports.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERIES = ("gulon_exact_index_query_offset", "gulon_index_query_offset")
SYMBOLS = tuple(name + form for name in QUERIES + ("gulon_mean_similarity",) for form in ("", "_dev"))


def test_symbols_are_declared_bound_and_exported():
    from gulon_amd import native
    header = open(os.path.join(ROOT, "include", "gulon_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    plain = re.sub(r"#ifdef GULON_TEST_HOOKS.*?#endif", "", header, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    L = native.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", plain), name
        assert name in native.SIGNATURES and name in exported
        assert getattr(L, name).argtypes == native.SIGNATURES[name][1]
        args = re.search(r"\bint32_t\s+" + name + r"\s*\(([^)]*)\)", plain).group(1)
        assert len(args.split(",")) == len(native.SIGNATURES[name][1]), name
    counts = {n: len(native.SIGNATURES[n][1]) for n in SYMBOLS}
    assert [counts[n] for n in QUERIES] == [9, 11] and counts["gulon_mean_similarity"] == 6
    for name in QUERIES + ("gulon_mean_similarity",):                # a device form: the host form's arguments and the stream
        assert counts[name + "_dev"] == counts[name] + 1
    assert L.gulon_abi_version() == 3
    assert not [n for n in native.TEST_HOOK_SIGNATURES if "offset" in n or "mean_sim" in n]


def test_source_is_in_the_makefile_without_hooks():
    make = open(os.path.join(ROOT, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "$(CSRC)/offset.hip" in srcs and os.path.exists(os.path.join(ROOT, "gulon_amd", "csrc", "offset.hip"))
    assert "$(CSRC)/offset.hpp" in re.search(r"^HDRS = (.*)$", make, flags=re.M).group(1).split()
    assert "offset" not in re.search(r"^HOOKED = (.*)$", make, flags=re.M).group(1).split()
    assert "GULON_TEST_HOOKS" not in open(os.path.join(ROOT, "gulon_amd", "csrc", "offset.hip")).read()


def test_the_kernels_are_in_the_new_file_and_read_no_new_environment():
    csrc = os.path.join(ROOT, "gulon_amd", "csrc")
    text = open(os.path.join(csrc, "offset.hip")).read()
    for kernel in ("offset_exact_scan", "offset_flat_scan", "mean_similarity_kernel"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\(", text), kernel
        others = [f for f in sorted(os.listdir(csrc)) if f != "offset.hip" and kernel in open(os.path.join(csrc, f)).read()]
        assert not others, (kernel, others)
    assert "getenv" not in text
    for shared in ("exact_tile(", "wave_offer(", "merge_wave_lists<", "launch_merge(", "launch_build_tables(",
                   "knn_row_chunks("):                              # the pieces it is put together from
        assert shared in text, shared


def test_the_kernels_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
           os.path.join(ROOT, "gulon_amd", "csrc", "offset.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    name, scratch = None, {}
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    # the exact scan; the flat scan at 1, 2, 4 and 8 query slots for 4-byte and 16-byte code words; the reduction
    assert len([n for n in scratch if "offset_exact_scan" in n]) == 1
    assert len([n for n in scratch if "offset_flat_scan" in n]) == 8
    assert len([n for n in scratch if "mean_similarity_kernel" in n]) == 1
    assert len(scratch) == 10 and not any(scratch.values()), scratch


def test_null_handles_and_limits_are_argument_errors_before_the_device():
    from gulon_amd import native
    L = native.lib()
    assert L.gulon_exact_index_query_offset_dev(None, None, 0, 1, None, None, None, None, None, None) \
        == native.ERR_INVALID_ARGUMENT
    assert L.gulon_index_query_offset_dev(None, None, 0, 1, 0, 0, None, None, None, None, None, None) \
        == native.ERR_INVALID_ARGUMENT
    assert L.gulon_mean_similarity_dev(None, None, -1, 1, 1, None, None) == native.ERR_INVALID_ARGUMENT
    assert L.gulon_mean_similarity_dev(None, None, 0, 0, 1, None, None) == native.ERR_INVALID_ARGUMENT
    assert L.gulon_mean_similarity_dev(None, None, 0, 12, 10, None, None) == native.OK      # nothing to do


def test_package_exports_the_names():
    import gulon_amd as g
    from gulon_amd import cli, csls
    for name in ("DeviceOffsets", "TranslationReport", "csls_offsets", "evaluate_dictionary", "mean_similarity",
                 "mean_similarity_reference", "offset_query_reference", "read_dictionary", "translate_words",
                 "translation_scores"):
        assert getattr(g, name) is getattr(csls, name) and name in g.__all__
    for cls in (g.ExactIndex, g.PQIndex, g.SortedIndex, g.WordIndex, g.ExactWordIndex):
        assert callable(cls.batch_query_offset_raw) and callable(cls.batch_query_offset), cls
    assert cli.TranslateConfig("i", "s") == cli.TranslateConfig("i", "s", None, None, "nn", 10, 10, (1, 5, 10), False,
                                                                None, False, None)
