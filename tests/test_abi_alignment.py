"""The alignment entry points (csrc/alignment.hip) are declared, bound and exported, and the Python names
are public.  No compute calls here."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gulon_dataset_pair_moment", "gulon_dataset_pair_moment_dev", "gulon_mutual_rows", "gulon_mutual_rows_dev")
NAMES = ("pair_moment", "pair_moment_reference", "mutual_rows", "mutual_rows_reference", "seed_alignment",
         "induce_matches", "train_alignment")


def test_symbols_are_declared_bound_and_exported():
    from gulon_amd import native
    header = open(os.path.join(ROOT, "include", "gulon_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in SYMBOLS:
        assert re.search(r"\bint32_t %s\s*\(" % s, header), s
        assert s in native.SIGNATURES and s in exported, s
        assert getattr(native.lib(), s).restype is native._i32
    # the lists of the pair moment are counted in 64 bits, and both forms answer into host memory
    for s in SYMBOLS[:2]:
        args = native.SIGNATURES[s][1]
        assert len(args) == 7 and args[4] is native.C.c_int64 and args[5] is native._f64p
    assert len(native.SIGNATURES["gulon_mutual_rows"][1]) == 5 and len(native.SIGNATURES["gulon_mutual_rows_dev"][1]) == 6


def test_the_abi_version_and_the_hooks_are_untouched():
    from gulon_amd import native
    assert native.lib().gulon_abi_version() == 3 and len(native.TEST_HOOK_SIGNATURES) == 7
    assert not [s for s in native.TEST_HOOK_SIGNATURES if "moment" in s or "mutual" in s]


def test_python_names_are_public():
    import gulon_amd as g
    from gulon_amd import alignment
    for name in NAMES:
        assert name in g.__all__ and getattr(g, name) is getattr(alignment, name), name
