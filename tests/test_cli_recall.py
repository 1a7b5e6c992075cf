"""`python -m gulon_amd test` without a device: argument handling, java.lang.Float.toString, the SummaryStats fold and
the eps cutoff of Tests.recallOf against restatements written here, and the command's output through cli.main's
`recall=` seam."""
import io
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from gulon_amd import cli
from gulon_amd import tests_recall as tr

F = np.float32


def _run(argv, recall):
    out = io.BytesIO()
    code = cli.main(argv, stdout=out, recall=recall)
    return code, out.getvalue().decode("utf-8")


def test_arguments_defaults_and_long_names():
    seen = []

    def stub(config, write, load):
        seen.append(config)
        return {}
    assert _run(["test", "-v", "vec.txt", "-i", "index.bin"], stub) == (0, "")
    assert _run(["test", "--vectors", "v", "--index", "i", "--sample", "7", "--error", "0.25"], stub)[0] == 0
    assert _run(["test", "-i", "i", "-v", "v", "-s", "1", "-e", "0"], stub)[0] == 0
    assert seen[0] == cli.RecallConfig("vec.txt", "index.bin", 1000, 0.0)
    assert seen[1] == cli.RecallConfig("v", "i", 7, 0.25)
    assert seen[2] == cli.RecallConfig("v", "i", 1, 0.0)
    assert isinstance(seen[1].epsilon, np.float32)               # Opts.option[Float]
    _run(["test", "-v", "v", "-i", "i", "-e", "0.1"], stub)
    assert seen[3].epsilon == F(0.1) and float(seen[3].epsilon) != 0.1


@pytest.mark.parametrize("argv,message", [
    (["test", "-v", "v", "-i", "i", "-s", "0"], "must be greater than 0"),
    (["test", "-v", "v", "-i", "i", "--sample", "-3"], "must be greater than 0"),
    (["test", "-v", "v", "-i", "i", "-e", "-0.5"], "must be non-negative"),
    (["test", "-v", "v", "-i", "i", "--error", "NaN"], "must be non-negative"),
    (["test", "-i", "i"], "-v/--vectors"),
    (["test", "-v", "v"], "-i/--index"),
    (["test", "-v", "v", "-i", "i", "-s", "many"], "invalid integer"),
])
def test_arguments_rejected_with_exit_code_2(argv, message, capsys):
    def stub(config, write, load):
        raise AssertionError("the command must not run")
    with pytest.raises(SystemExit) as e:
        cli.main(argv, stdout=io.BytesIO(), recall=stub)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def _f32(bits):
    return np.uint32(bits).view(np.float32)


@pytest.mark.parametrize("value,text", [
    (F(1.0), "1.0"), (F(0.5), "0.5"), (F(0.1), "0.1"), (F(1.0) / F(3.0), "0.33333334"), (F(0.001), "0.001"),
    (F(1.0e-4), "1.0E-4"), (F(9999999.0), "9999999.0"), (F(1.0e7), "1.0E7"), (_f32(0x00800000), "1.17549435E-38"),
    (F("nan"), "NaN"), (F(0.0), "0.0"),
    # further values of the JDK's documentation and of this command's range
    (F("inf"), "Infinity"), (F("-inf"), "-Infinity"), (F(-0.0), "-0.0"), (_f32(0x7F7FFFFF), "3.4028235E38"),
    (_f32(1), "1.4E-45"), (F(100.0), "100.0"), (F(0.999), "0.999"), (F(0.0625), "0.0625"), (F(-2.5), "-2.5"),
    (F(12345678.0), "1.2345678E7"), (F(9.999999e-4), "9.999999E-4"), (F(0.2) + F(0.1), "0.3"), (F(0.7) * F(0.7), "0.48999998"),
])
def test_float_to_string_known_answers(value, text):
    assert tr.java_float_to_string(value) == text


def test_float_to_string_is_the_shortest_that_reads_back():
    """Every output reads back as the same binary32, and no decimal with fewer digits (two at least) does."""
    rng = np.random.default_rng(5)
    bits = np.r_[rng.integers(1, 0x7F800000, 3000), rng.integers(0x3A000000, 0x3F800001, 3000)].astype(np.uint32)
    for v in bits.view(np.float32):
        text = tr.java_float_to_string(v)
        assert F(float(text)) == v, (v, text)
        mantissa = text.replace("-", "").split("E")[0].replace(".", "").strip("0")
        n = len(mantissa)
        assert "." in text and n <= 9
        if n > 2 and int(v.view(np.uint32)) & 0x7FFFFF:          # not a power of two (their interval is the JDK's own)
            shorter = np.format_float_scientific(v, precision=n - 2, unique=False)
            assert F(float(shorter)) != v, (v, text, shorter)


def _fold_restated(xs):
    """SummaryStats.++ folded from the left over SummaryStats(1, x, 0), every operation rounded to binary32 through
    struct (no numpy scalars): an independent restatement of MathUtils.scala:9-20."""
    def r(x):
        return struct.unpack("f", struct.pack("f", x))[0]
    count, mean, s = 0, 0.0, 0.0
    for x in xs:
        x = r(float(x))
        if count == 0:
            count, mean, s = 1, x, 0.0
            continue
        n = count + 1
        d = r(mean - x)
        new_mean = r(mean + r(r(r(1.0) / r(float(n))) * r(x - mean)))
        s = r(r(s + 0.0) + r(r(r(r(d * d) * r(float(count))) * 1.0) / r(float(n))))
        count, mean = n, new_mean
    return count, mean, s


def test_summary_stats_fold_matches_the_restatement():
    rng = np.random.default_rng(2)
    for size in (0, 1, 2, 3, 10, 1000):
        xs = (rng.integers(0, 11, size) / 10).astype(np.float32)
        got = tr.fold(xs)
        count, mean, s = _fold_restated(xs)
        assert got.count == count
        assert F(got.mean).view(np.uint32) == F(mean).view(np.uint32)
        assert F(got.s).view(np.uint32) == F(s).view(np.uint32)
        if count:
            assert F(got.std_dev).view(np.uint32) == F(math.sqrt(float(F(s) / F(count)))).view(np.uint32)
    empty = tr.fold([])
    assert (empty.count, empty.mean, empty.s) == (0, 0, 0) and math.isnan(empty.std_dev)   # 0f / 0 on the JVM
    one = tr.fold([F(0.3)])
    assert (one.count, one.mean, one.s, one.std_dev) == (1, F(0.3), 0, 0)


def test_summary_stats_fold_depends_on_the_order():
    xs = np.asarray([0.1, 0.7, 0.3, 0.9, 0.2], np.float32)
    a, b = tr.fold(xs), tr.fold(xs[[4, 2, 0, 3, 1]])
    assert a.count == b.count == 5
    assert (F(a.mean).view(np.uint32), F(a.s).view(np.uint32)) != (F(b.mean).view(np.uint32), F(b.s).view(np.uint32))
    assert (a.count, float(a.mean), float(a.s)) == _fold_restated(xs)
    assert (b.count, float(b.mean), float(b.s)) == _fold_restated(xs[[4, 2, 0, 3, 1]])


def test_combine_of_two_larger_stats():
    """++ with that.count > 1 (MathUtils.scala:15-19): n, the weighted mean, s + s + d^2 * count * count / n."""
    a, b = tr.fold(np.asarray([0.5, 1.0], np.float32)), tr.fold(np.asarray([0.0, 0.25, 0.5], np.float32))
    c = a.combine(b)
    d = F(a.mean - b.mean)
    assert c.count == 5
    assert c.mean == F(a.mean + F(F(F(3) / F(5)) * F(b.mean - a.mean)))
    assert c.s == F(F(a.s + b.s) + F(F(F(F(d * d) * F(2)) * F(3)) / F(5)))
    assert a.combine(tr.SummaryStats()) is a and tr.SummaryStats().combine(b) is b


def test_cutoff_is_the_double_precision_formula():
    v = np.asarray([0.0, 1.0, 2.0, 0.3, 123.456, 1e-30, 3e38, np.inf, np.nan, 7.0], np.float32)
    assert tr.cutoff(v, 0.0).view(np.uint32).tolist() == v.view(np.uint32).tolist()      # eps == 0f: untouched
    for eps in (0.1, 0.5, 1e-7, 3.0):
        got = tr.cutoff(v, F(eps))
        factor = float(F(1.0) + F(eps))                            # 1f + eps is a float sum
        for x, g in zip(v.tolist(), got):
            if math.isnan(x):
                assert math.isnan(g)
                continue
            r = math.sqrt(x) * factor                              # doubles
            want = r * r
            want32 = F(np.inf) if want > 3.4028235677973366e38 else F(want)
            assert F(g).view(np.uint32) == want32.view(np.uint32), (x, eps)
    # crafted: the float sum 1f + eps differs from the double sum, and the result shows it
    x, eps = F(2.0), F(5e-8)                                 # below half an ulp of 1f: 1f + eps == 1f
    assert float(F(1.0) + eps) != 1.0 + float(eps)
    assert tr.cutoff([x], eps)[0] == F((math.sqrt(2.0) * float(F(1.0) + eps)) ** 2)
    assert tr.cutoff([x], eps)[0] != F((math.sqrt(2.0) * (1.0 + float(eps))) ** 2)


def test_command_prints_the_result_lines_in_ascending_k():
    stats = {100: tr.SummaryStats(4, F(0.25), F(0.01)), 1: tr.SummaryStats(4, F(1.0), F(0.0)),
             10: tr.SummaryStats(4, F(1.0) / F(3.0), F(2.0 ** -28))}   # 1000: kept by no query, not in the map

    def stub(config, write, load):
        write("\u001b[36mRUNNING:\u001b[0m Calculating recall of index\n")
        return stats
    code, text = _run(["test", "-v", "v", "-i", "i"], stub)
    assert code == 0
    assert text.split("\n") == ["\u001b[36mRUNNING:\u001b[0m Calculating recall of index",
                                "R@1: 1.0 +/- 0.0",
                                "R@10: 0.33333334 +/- 3.0517578E-5",     # sqrt(2^-28 / 4) = 2^-15
                                "R@100: 0.25 +/- 0.05",
                                ""]


def test_recall_of_with_a_stub_evaluator_folds_in_query_order_and_drops_unkept_k():
    """Tests.recall_of over stubs (no device): one index query per group of queries at the largest k they kept, the
    word -> row resolution, the fold in query order, and a k no query kept is absent."""
    class KeyIndex:
        def lookup(self, word):
            return {"a": 2, "b": 0, "c": 1}.get(word)

    class Vectors:
        key_index, matrix, size = KeyIndex(), "matrix", 3

    class StubIndex:
        words, size = ["c", "a", "b", "absent"], 4

        def batch_query_raw(self, k, vectors):
            assert k == 3
            rows = np.asarray([[0, 1, 2], [2, 1, -1], [1, -1, -1]], np.int32)[:len(vectors)]
            return rows, None, (rows >= 0).sum(axis=1), np.asarray([0, 1, 5], np.int32)[:len(vectors)]
    calls = []

    def evaluate(matrix, queries, rows, ks, cutoffs):
        calls.append((matrix, rows.tolist(), ks.tolist(), cutoffs.copy()))
        return np.asarray([[1, 1, 3], [0, 1, 2], [1, 1, 1]], np.int32)
    queries = np.zeros((3, 2), np.float32)
    kth = np.asarray([[1, 2, 3, np.nan], [1, 2, 3, np.nan], [1, 2, 3, np.nan]], np.float32)
    tests = tr.Tests(Vectors(), queries, (1, 2, 3, 1000), kth, np.asarray([3, 3, 3]))
    got = tests.recall_of(StubIndex(), eps=0.0, evaluate=evaluate)
    assert sorted(got) == [1, 2, 3]                                # 1000 was kept by no query
    assert calls[0][0] == "matrix" and calls[0][2] == [1, 2, 3]
    assert calls[0][1] == [[1, 2, 0], [0, 2, -1], [2, -1, -1]]     # index rows -> the vectors' rows, by word
    assert calls[0][3].tolist() == [[1, 2, 3]] * 3
    for j, k in enumerate((1, 2, 3)):
        want = _fold_restated(np.asarray([[1, 1, 3], [0, 1, 2], [1, 1, 1]], np.float32)[:, j] / F(k))
        assert (got[k].count, float(got[k].mean), float(got[k].s)) == want
    assert got.flagged == 1 and got.flagged_queries == (1,)        # query 2's tie was replayed exactly

    class Lacking(StubIndex):
        def batch_query_raw(self, k, vectors):
            rows, d, c, f = super().batch_query_raw(k, vectors)
            rows[0, 0] = 3
            return rows, d, c, f
    with pytest.raises(LookupError, match="'absent'"):
        tests.recall_of(Lacking(), evaluate=evaluate)


def test_recall_kernel_uses_no_scratch():
    """Both forms of recall_counts_kernel keep their per-k cutoffs and counts in registers."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fvisibility=hidden", "-I" + os.path.join(root, "include"), "--cuda-device-only", "-c",
           os.path.join(root, "gulon_amd", "csrc", "recall.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    name, scratch = None, {}
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and "recall_counts_kernel" in name:
            scratch[name] = int(m.group(1))
    assert len(scratch) == 2, scratch
    assert set(scratch.values()) == {0}, scratch
