"""The entry points of the 3CosMul work (csrc/cosmul.hip, csrc/exact.hip) in the header, the binding table and the product
library; the source in the Makefile; the names the package exports.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gulon_exact_index_query_cosmul", "gulon_exact_index_query_cosmul_dev", "gulon_index_query_cosmul",
           "gulon_index_query_cosmul_dev")


def test_symbols_are_declared_bound_and_exported():
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
        args = re.search(r"\bint32_t\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len(args.split(",")) == len(native.SIGNATURES[name][1]), name
    # the *_query_terms arguments minus extra, the two flags and out_flags, plus normalize; the exact _dev form also d_err
    counts = {n: len(native.SIGNATURES[n][1]) for n in native.SIGNATURES}
    assert counts["gulon_exact_index_query_cosmul"] == counts["gulon_exact_index_query_terms"] - 3
    assert counts["gulon_exact_index_query_cosmul_dev"] == counts["gulon_exact_index_query_terms_dev"] - 3 + 1
    assert counts["gulon_index_query_cosmul"] == counts["gulon_index_query_terms"] - 3
    assert counts["gulon_index_query_cosmul_dev"] == counts["gulon_index_query_terms_dev"] - 3
    assert L.gulon_abi_version() == 3


def test_shape_hooks_are_in_the_hooks_library_only():
    """gulon_selftest_cosmul_{flat,exact}_shape: declared under GULON_TEST_HOOKS, bound with the header's argument
    counts, exported by libgulon_hip_testhooks.so and not by the product; cosmul.hip is compiled with hooks."""
    from gulon_amd import native
    header = open(os.path.join(ROOT, "include", "gulon_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    guarded = "".join(re.findall(r"#ifdef GULON_TEST_HOOKS(.*?)#endif", header, flags=re.S))
    plain = re.sub(r"#ifdef GULON_TEST_HOOKS.*?#endif", "", header, flags=re.S)
    def exported(path):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        return {l.split()[-1] for l in out.splitlines() if " T " in l}
    prod, hooks = exported(native.LIB_PATH), exported(native.HOOKS_LIB_PATH)
    for name in ("gulon_selftest_cosmul_flat_shape", "gulon_selftest_cosmul_exact_shape"):
        args = re.search(r"\bint32_t\s+" + name + r"\s*\(([^)]*)\)", guarded).group(1)
        assert len(args.split(",")) == len(native.TEST_HOOK_SIGNATURES[name][1]), name
        assert name not in plain and name not in native.SIGNATURES
        assert name in hooks and name not in prod
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "cosmul" in re.search(r"^HOOKED = (.*)$", make, flags=re.M).group(1).split()


def test_source_is_in_the_makefile():
    make = open(os.path.join(ROOT, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    hdrs = re.search(r"^HDRS = (.*)$", make, flags=re.M).group(1).split()
    assert "$(CSRC)/cosmul.hip" in srcs and os.path.exists(os.path.join(ROOT, "gulon_amd", "csrc", "cosmul.hip"))
    assert "$(CSRC)/cosmul.hpp" in hdrs and os.path.exists(os.path.join(ROOT, "gulon_amd", "csrc", "cosmul.hpp"))


def test_operands_are_dropped_by_the_one_kernel():
    """cosmul.hip drops the term rows with compose.hip's kernel: it launches launch_drop and defines no kernel of its own
    for it."""
    text = open(os.path.join(ROOT, "gulon_amd", "csrc", "cosmul.hip")).read()
    assert "launch_drop(" in text and "drop_rows_kernel" not in text.replace("compose.hip's kernel", "")


def test_package_exports_the_names():
    import gulon_amd as g
    from gulon_amd import expressions
    for name in ("COSMUL_EPS", "cosmul_reference"):
        assert getattr(g, name) is getattr(expressions, name) and name in g.__all__
    for cls in (g.ExactIndex, g.PQIndex, g.SortedIndex):
        assert callable(cls.batch_query_cosmul_raw) and callable(cls.batch_query_cosmul)
        assert "descending" in cls.batch_query_cosmul.__doc__
    for cls in (g.WordIndex, g.ExactWordIndex):
        assert callable(cls.batch_query_cosmul) and callable(cls.query_cosmul)
    import inspect
    assert inspect.signature(g.evaluate_analogies).parameters["method"].default == "add"
