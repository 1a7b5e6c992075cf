"""The environment switches of the native library, the ScanTuning keys and the table "Environment switches" of
DESIGN.md section 7 must name the same variables, and the scripts may only set variables that exist."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gulon_amd", "csrc")
PYTHON_SIDE = {"GULON_HIP_LIB", "GULON_SHARED_BOUNDS", "GULON_HOST_PROFILE"}   # and GULON_BENCH_*


def _read(path):
    return open(path, encoding="utf-8", errors="replace").read()


def _sources():
    return {f: _read(os.path.join(CSRC, f)) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp"))}


def _table():
    doc = _read(os.path.join(ROOT, "DESIGN.md"))
    sec = doc[doc.index("### Environment switches"):doc.index("## 8. ")]
    rows = {}
    for line in sec.splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        m = re.fullmatch(r"`(GULON_[A-Z0-9_]+)`", cells[0]) if line.startswith("|") else None
        if m:
            assert m.group(1) not in rows, m.group(1)
            rows[m.group(1)] = cells[1]
    return rows


def _scan_tuning_keys():
    src = _read(os.path.join(CSRC, "index_handle.hip"))
    body = re.search(r"ScanTuning::ScanTuning\(\) \{\s*static const char \*keys\[\] = \{(.*?)\};", src, re.S).group(1)
    return set(re.findall(r'"(GULON_[A-Z0-9_]+)"', body))


def test_native_switches_and_tuning_keys_are_the_documented_ones():
    srcs = _sources()
    native = set()
    for name, src in srcs.items():
        native |= set(re.findall(r'getenv\("(GULON_[A-Z0-9_]+)"\)', src))
        # every other getenv is ScanTuning's loop over its key list
        other = re.findall(r'getenv\((?!"GULON_)[^)]*\)', src)
        assert other == (["getenv(k)"] if name == "index_handle.hip" else []), (name, other)
    keys = _scan_tuning_keys()
    table = _table()
    assert len(keys) >= 10 and not keys & native
    assert set(table) == native | keys, (sorted((native | keys) - set(table)), sorted(set(table) - native - keys))
    assert {n for n, kind in table.items() if kind == "`ScanTuning`"} == keys


def test_every_switch_that_changes_a_path_is_named_by_a_gpu_test():
    """A ScanTuning key, a switch that turns a fast path off, a knob of the exact index, a testing or a debugging switch
    that no GPU test names is a path nobody runs: section 7 promises that results do not depend on the former and that
    the latter can be used to bisect.  GULON_HOST_CONTEXTS changes how concurrent host calls share workspaces, so it
    counts as well."""
    kinds = {"`ScanTuning`", "fast path off", "exact index", "testing", "debugging"}
    # GULON_RCCL_LIB only names the file dlopen tries first; the sharded index either loads RCCL or reports that it
    # cannot, and no result depends on which name worked
    exempt = {"GULON_RCCL_LIB"}
    table = _table()
    assert set(table.values()) - kinds == {"configuration"}, set(table.values())
    must = {n for n, kind in table.items() if kind in kinds} | {"GULON_HOST_CONTEXTS"}
    assert not must & exempt and exempt < set(table)
    tests_dir = os.path.join(ROOT, "tests")
    text = "\n".join(_read(os.path.join(tests_dir, f)) for f in sorted(os.listdir(tests_dir))
                     if f.startswith("test_gpu_") and f.endswith(".py"))
    named = set(re.findall(r"\bGULON_[A-Z0-9_]+\b", text))
    assert not must - named, sorted(must - named)


def test_scripts_set_only_existing_variables():
    known = set(_table()) | PYTHON_SIDE
    bad = []
    for d, dirs, files in os.walk(os.path.join(ROOT, "scripts")):
        dirs[:] = [x for x in dirs if x != "__pycache__"]
        for f in files:
            if not f.endswith((".sh", ".py", ".hip", ".md")):
                continue
            path = os.path.join(d, f)
            # (an environment assignment or keyword argument; not a compiler definition such as -DGULON_FILTER_GLB=4)
            for name in re.findall(r"(?<![\w-])(GULON_[A-Z0-9_]+)=", _read(path)):
                if name not in known and not name.startswith("GULON_BENCH_"):
                    bad.append((os.path.relpath(path, ROOT), name))
    assert not bad, bad
