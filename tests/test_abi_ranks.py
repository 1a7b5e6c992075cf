"""The entry points of the rank queries (csrc/rank.hip) in the header, the binding table and the product
library; what they leave alone in the header's stream contract; the source in the Makefile, compiled without test hooks
and its kernels free of scratch; the names the package exports.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import stream_contract as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gulon_amd", "csrc")
SYMBOLS = ("gulon_exact_index_query_rank", "gulon_index_query_rank")


def test_symbols_are_declared_bound_and_exported():
    from gulon_amd import native
    header = re.sub(r"/\*.*?\*/", "", sc.header_text(), flags=re.S)
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
    assert [len(native.SIGNATURES[n][1]) for n in SYMBOLS] == [11, 13]
    assert L.gulon_abi_version() == 3
    assert not [n for n in native.TEST_HOOK_SIGNATURES if "query_rank" in n]
    assert not [n for n in native.SIGNATURES if "query_rank" in n and n not in SYMBOLS]      # no device forms yet


def test_the_stream_contract_of_the_header_is_untouched():
    text = sc.header_text()
    without = text
    for name in SYMBOLS:
        without, cut = re.subn(r"\bint32_t\s+" + name + r"\s*\([^)]*\)\s*;", "", without)
        assert cut == 1, name
    assert len(sc.stream_entry_points(text)) == 40
    assert sc.stream_entry_points(text) == sc.stream_entry_points(without)
    assert sc.device_pointer_entry_points_without_stream(text) == sc.device_pointer_entry_points_without_stream(without)
    for name in SYMBOLS:                                             # host pointers, and the comment says where they run
        args = re.search(r"\bint32_t\s+" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert "stream" not in args and not re.search(r"\bd_\w+", args)
        assert any("null stream" in " ".join(c.split()) for c in sc.comments_naming(text, name)), name


def test_source_is_in_the_makefile_without_hooks():
    make = open(os.path.join(ROOT, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "$(CSRC)/rank.hip" in srcs and os.path.exists(os.path.join(CSRC, "rank.hip"))
    assert "$(CSRC)/rank.hpp" in re.search(r"^HDRS = (.*)$", make, flags=re.M).group(1).split()
    assert "rank" not in re.search(r"^HOOKED = (.*)$", make, flags=re.M).group(1).split()
    text = open(os.path.join(CSRC, "rank.hip")).read()
    assert "GULON_TEST_HOOKS" not in text and "getenv" not in text
    for kernel in ("rank_exact_gold", "rank_exact_scan", "rank_flat_gold", "rank_flat_scan", "rank_finish"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\(", text), kernel
        others = [f for f in sorted(os.listdir(CSRC)) if f != "rank.hip" and kernel in open(os.path.join(CSRC, f)).read()]
        assert not others, (kernel, others)
    for shared in ("exact_tile(", "knn_row_chunks(", "launch_build_tables(", "offset_flat_shape(", "offset_flat_max_e(",
                   "flat_slot_bytes(", "check_flat(", "StreamOrder"):      # the pieces it is put together from
        assert shared in text, shared
    for dropped in ("WaveList", "wave_offer", "merge_wave_lists", "launch_merge", "atomicAdd"):   # a counter, not a list
        assert dropped not in text, dropped
    moved = open(os.path.join(CSRC, "offset.hpp")).read()                # the slot and shape rules are shared, not copied
    for name in ("flat_slot_bytes", "offset_flat_max_e", "offset_flat_shape", "check_flat"):
        assert re.search(r"\b" + name + r"\([^;{]*\)\s*\{", moved), name
        assert not re.search(r"\b" + name + r"\([^;{]*\)\s*\{", open(os.path.join(CSRC, "offset.hip")).read()), name


def test_the_kernels_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
           os.path.join(CSRC, "rank.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
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
    # the two exact kernels; the flat scan at 1, 2, 4 and 8 query slots and the flat gold keys, for 4-byte and 16-byte
    # code words; the finish
    assert len([n for n in scratch if "rank_exact_gold" in n]) == 1
    assert len([n for n in scratch if "rank_exact_scan" in n]) == 1
    assert len([n for n in scratch if "rank_flat_scan" in n]) == 8
    assert len([n for n in scratch if "rank_flat_gold" in n]) == 2
    assert len([n for n in scratch if "rank_finish" in n]) == 1
    assert len(scratch) == 13 and not any(scratch.values()), scratch
    assert not any(v for n, v in lds.items() if "rank_flat_scan" in n), lds      # the flat scan's LDS is the launch's


def test_null_handles_are_argument_errors_before_the_device():
    from gulon_amd import native
    L = native.lib()
    f, i = np.zeros(1, np.float32), np.zeros(1, np.int32)
    for b in (0, 1):
        assert L.gulon_exact_index_query_rank(None, f, b, None, None, i, i, i, i, f, None) == native.ERR_INVALID_ARGUMENT
        assert L.gulon_index_query_rank(None, f, b, 0, 0, None, None, i, i, i, i, f, None) == native.ERR_INVALID_ARGUMENT


def test_package_exports_the_names():
    import gulon_amd as g
    from gulon_amd import cli, ranks
    for name in ("RankReport", "evaluate_dictionary_ranks", "rank_query_reference"):
        assert getattr(g, name) is getattr(ranks, name) and name in g.__all__
    for cls in (g.ExactIndex, g.PQIndex, g.SortedIndex, g.WordIndex, g.ExactWordIndex):
        assert callable(cls.batch_query_rank_raw), cls
    assert cli.TranslateConfig("i", "s").ranks is False
    assert cli.TranslateConfig.__dataclass_fields__["ranks"] is list(cli.TranslateConfig.__dataclass_fields__.values())[-1]
