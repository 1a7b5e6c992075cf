"""The entry point of the log-sum-exp queries (csrc/logsumexp.hip) in the header, the binding table and the
product library; what it leaves alone in the header's stream contract; the source in the Makefile, compiled without test
hooks and its kernels free of scratch and of atomics; the argument checks that need no device; the names the package
exports.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import stream_contract as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gulon_amd", "csrc")
SYMBOL = "gulon_exact_index_query_logsumexp"


def test_symbol_is_declared_bound_and_exported():
    from gulon_amd import native
    header = re.sub(r"/\*.*?\*/", "", sc.header_text(), flags=re.S)
    plain = re.sub(r"#ifdef GULON_TEST_HOOKS.*?#endif", "", header, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    L = native.lib()
    args = re.search(r"\bint32_t\s+" + SYMBOL + r"\s*\(([^)]*)\)", plain).group(1)
    assert [" ".join(a.split()) for a in args.split(",")] == [
        "gulon_exact_index *idx", "const float *queries", "int32_t b", "float beta", "const int32_t *exclude",
        "double *out_lse", "int32_t *out_terms"]
    assert SYMBOL in native.SIGNATURES and SYMBOL in exported
    res, argtypes = native.SIGNATURES[SYMBOL]
    assert res is C.c_int32 and len(argtypes) == 7 and argtypes[3] is C.c_float
    assert getattr(L, SYMBOL).argtypes == argtypes
    assert L.gulon_abi_version() == 3
    assert len(native.TEST_HOOK_SIGNATURES) == 7 and not [n for n in native.TEST_HOOK_SIGNATURES if "logsumexp" in n]
    assert [n for n in native.SIGNATURES if "logsumexp" in n] == [SYMBOL]                    # no device form yet


def test_the_stream_contract_of_the_header_is_untouched():
    text = sc.header_text()
    without, cut = re.subn(r"\bint32_t\s+" + SYMBOL + r"\s*\([^)]*\)\s*;", "", text)
    assert cut == 1
    assert len(sc.stream_entry_points(text)) == 40
    assert sc.stream_entry_points(text) == sc.stream_entry_points(without)
    assert sc.device_pointer_entry_points_without_stream(text) == sc.device_pointer_entry_points_without_stream(without)
    args = re.search(r"\bint32_t\s+" + SYMBOL + r"\s*\(([^)]*)\)", text).group(1)
    assert "stream" not in args and not re.search(r"\bd_\w+", args)
    comment = " ".join(" ".join(c.split()) for c in sc.comments_naming(text, SYMBOL))
    for said in ("null stream", "fixed order", "No atomics", "NOT pinned across batch shapes", "taken as given",
                 "row_offsets[y] = (float)((2 / beta) * L(y))", "-inf"):
        assert said in comment, said


def test_source_is_in_the_makefile_without_hooks():
    make = open(os.path.join(ROOT, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "$(CSRC)/logsumexp.hip" in srcs and os.path.exists(os.path.join(CSRC, "logsumexp.hip"))
    assert "$(CSRC)/logsumexp.hpp" in re.search(r"^HDRS = (.*)$", make, flags=re.M).group(1).split()
    assert "logsumexp" not in re.search(r"^HOOKED = (.*)$", make, flags=re.M).group(1).split()
    text = open(os.path.join(CSRC, "logsumexp.hip")).read()
    assert "GULON_TEST_HOOKS" not in text and "getenv" not in text
    for kernel in ("logsumexp_exact_scan", "logsumexp_finish"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\(", text), kernel
    for shared in ("exact_tile(", "exact_passes(", "finite_key(", "__ballot(", "__popcll(", "__shfl_xor("):
        assert shared in text, shared
    for absent in ("atomicAdd", "__hip_atomic", "expf(", "__expf", "logf("):      # a fixed order, and binary64 throughout
        assert absent not in text, absent


def test_the_kernels_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
           os.path.join(CSRC, "logsumexp.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    name, scratch = None, {}
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    assert len([n for n in scratch if "logsumexp_exact_scan" in n]) == 1
    assert len([n for n in scratch if "logsumexp_finish" in n]) == 1
    assert len(scratch) == 2 and not any(scratch.values()), scratch


def test_argument_checks_that_need_no_device():
    from gulon_amd import native
    L = native.lib()
    f, d, i = np.zeros(1, np.float32), np.zeros(1, np.float64), np.zeros(1, np.int32)
    for b in (0, 1):
        assert L.gulon_exact_index_query_logsumexp(None, f, b, 30.0, None, d, i.ctypes.data) == native.ERR_INVALID_ARGUMENT
        assert "index is null" in native.last_error()


def test_package_exports_the_names():
    import gulon_amd as g
    from gulon_amd import cli, csls, ranks, softmax
    for name in ("logsumexp_reference", "isf_offsets_from", "isf_probabilities"):
        assert getattr(g, name) is getattr(softmax, name) and name in g.__all__
    assert g.isf_offsets is csls.isf_offsets and "isf_offsets" in g.__all__
    for cls in (g.ExactIndex, g.ExactWordIndex):
        assert callable(cls.batch_query_logsumexp), cls
    import inspect
    for fn, tail in ((csls.translate_words, ["beta", "sources"]), (csls.evaluate_dictionary, ["beta", "sources"]),
                     (ranks.evaluate_dictionary_ranks, ["beta", "sources"])):
        params = inspect.signature(fn).parameters
        assert list(params)[-2:] == tail and params["beta"].default == 30.0 and params["sources"].default is None
    assert list(inspect.signature(csls.isf_offsets).parameters) == ["target", "source", "beta", "sources"]
    assert cli.IsfTranslateConfig("i", "s").beta == 30.0 and cli.IsfTranslateConfig("i", "s").isf_sources is None
