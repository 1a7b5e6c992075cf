"""The entry points of the analogies work (csrc/dataset_compose.hip, csrc/exact.hip, csrc/analogy.hip) in the header, the
binding table and the product library; their sources in the Makefile; the names the package exports.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gulon_dataset_compose_rows", "gulon_dataset_compose_rows_dev", "gulon_exact_index_query_terms",
           "gulon_exact_index_query_terms_dev", "gulon_analogy_counts", "gulon_analogy_counts_dev")


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
    # a device form: the host form's arguments and the stream; the dataset's compose also takes the error word
    assert [len(native.SIGNATURES[n][1]) for n in SYMBOLS] == [8, 10, 13, 14, 12, 13]
    assert L.gulon_abi_version() == 3


def test_sources_are_in_the_makefile():
    make = open(os.path.join(ROOT, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    hdrs = re.search(r"^HDRS = (.*)$", make, flags=re.M).group(1).split()
    for name in ("dataset_compose.hip", "analogy.hip", "compose.hip", "exact.hip"):
        assert "$(CSRC)/" + name in srcs and os.path.exists(os.path.join(ROOT, "gulon_amd", "csrc", name)), name
    assert "$(CSRC)/compose.hpp" in hdrs


def test_drop_rows_kernel_has_one_definition():
    """The exact index drops operands with compose.hip's kernel, declared in compose.hpp: no second one."""
    csrc = os.path.join(ROOT, "gulon_amd", "csrc")
    defined = [f for f in sorted(os.listdir(csrc))
               if re.search(r"void drop_rows_kernel\([^;{]*\)\s*\{", open(os.path.join(csrc, f)).read())]
    assert defined == ["compose.hip"]
    assert "launch_drop(" in open(os.path.join(csrc, "exact.hip")).read()


def test_package_exports_the_names():
    import gulon_amd as g
    from gulon_amd import analogies
    for name in ("AnalogyReport", "evaluate_analogies", "read_questions"):
        assert getattr(g, name) is getattr(analogies, name) and name in g.__all__
    for cls, names in ((g.ExactIndex, ("compose_rows", "batch_query_expressions_raw", "batch_query_expressions")),
                       (g.ExactWordIndex, ("resolve_expressions", "batch_query_expressions", "query_expression"))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
