"""The entry points of the similarity work (csrc/pairs.hip) in the header, the binding table and the product library; the
source in the Makefile and its kernels free of scratch; the names the package exports; the size limit of the rank sums,
which is checked before the device is touched.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = ("gulon_index_pair_distances", "gulon_grouped_index_pair_distances", "gulon_dataset_pair_distances")
SYMBOLS = tuple(name + form for name in PAIRS + ("gulon_rank_sums",) for form in ("", "_dev"))


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
    # a device form: the host form's arguments and the stream
    counts = {n: len(native.SIGNATURES[n][1]) for n in SYMBOLS}
    assert [counts[n] for n in PAIRS] == [5, 5, 5] and counts["gulon_rank_sums"] == 6
    for name in PAIRS + ("gulon_rank_sums",):
        assert counts[name + "_dev"] == counts[name] + 1
    assert L.gulon_abi_version() == 3 and not [n for n in native.TEST_HOOK_SIGNATURES if "pair" in n or "rank" in n]


def test_source_is_in_the_makefile():
    make = open(os.path.join(ROOT, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "$(CSRC)/pairs.hip" in srcs and os.path.exists(os.path.join(ROOT, "gulon_amd", "csrc", "pairs.hip"))
    assert "pairs" not in re.search(r"^HOOKED = (.*)$", make, flags=re.M).group(1).split()


def test_the_kernels_are_in_the_new_file_and_say_which_group_rule_they_use():
    csrc = os.path.join(ROOT, "gulon_amd", "csrc")
    text = open(os.path.join(csrc, "pairs.hip")).read()
    for kernel in ("index_pair_distances_kernel", "dataset_pair_distances_kernel", "rank_sums_kernel"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\(", text), kernel
        others = [f for f in sorted(os.listdir(csrc)) if f != "pairs.hip" and kernel in open(os.path.join(csrc, f)).read()]
        assert not others, (kernel, others)
    head = text[:text.index("#include")]
    assert "lookup_base" in head and "NOT group_centroid" in head
    assert "lookup_base(" in text and "group_centroid(" not in text and "tile_load<64" in text


def test_the_kernels_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
           os.path.join(ROOT, "gulon_amd", "csrc", "pairs.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    name, scratch = None, {}
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    # flat and grouped; 16-byte and 4-byte row loads; the rank sums
    assert len([n for n in scratch if "index_pair_distances_kernel" in n]) == 2
    assert len([n for n in scratch if "dataset_pair_distances_kernel" in n]) == 2
    assert len([n for n in scratch if "rank_sums_kernel" in n]) == 1
    assert len(scratch) == 5 and not any(scratch.values()), scratch


def test_more_than_two_to_the_twenty_pairs_are_refused_before_the_device():
    """n <= 2^20 keeps every sum below 2^60; the check precedes every HIP call, so it is seen without a GPU."""
    from gulon_amd import native
    from gulon_amd.similarity import MAX_PAIRS, rank_sums
    assert MAX_PAIRS == 1 << 20
    x = np.zeros(MAX_PAIRS + 1, np.float32)
    with pytest.raises(ValueError, match=r"\[0, 1048576\], got 1048577"):
        rank_sums(x, x)
    with pytest.raises(ValueError, match=r"got 1048577"):
        rank_sums(x, x, np.zeros(MAX_PAIRS + 1, np.int32), 3)
    L = native.lib()
    assert L.gulon_rank_sums_dev(None, None, None, MAX_PAIRS + 1, 1, None, None) == native.ERR_INVALID_ARGUMENT
    assert L.gulon_rank_sums_dev(None, None, None, -1, 1, None, None) == native.ERR_INVALID_ARGUMENT
    for name in PAIRS:                                            # a null handle is an argument error, not a crash
        assert getattr(L, name + "_dev")(None, None, None, 0, None, None) == native.ERR_INVALID_ARGUMENT


def test_package_exports_the_names():
    import gulon_amd as g
    from gulon_amd import similarity
    for name in ("SimilarityReport", "evaluate_pairs", "read_pairs", "pair_distance_reference", "rank_sums",
                 "rank_sums_reference", "spearman"):
        assert getattr(g, name) is getattr(similarity, name) and name in g.__all__
    for cls in (g.PQIndex, g.PQIndexView, g.SortedIndex, g.GroupedIndex, g.ExactIndex):
        assert callable(cls.pair_distances) and callable(cls.pair_distances_dev), cls
    for cls in (g.WordIndex, g.ExactWordIndex):
        assert callable(cls.distances)
    from gulon_amd import cli
    assert cli.SimilarityConfig("i", "p") == cli.SimilarityConfig("i", "p", False, None, False)
