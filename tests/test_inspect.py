"""Index diagnostics, the host side (gulon_amd/inspect.py, the `inspect` command): IndexReport arithmetic from hand-made
arrays, reference_quality, and the command's argument handling and printing through the `inspect=` hook.  No GPU."""
import io
import math

import numpy as np
import pytest

from gulon_amd import cli
from gulon_amd.inspect import IndexReport, entropy_bits, reference_quality, worst_rows


def test_entropy_used_counts_and_shares():
    k = 8
    hist = np.array([[5] * k,                         # uniform: log2 k bits, every centroid used
                     [40] + [0] * (k - 1),            # one centroid: 0 bits
                     [20, 10, 10, 0, 0, 0, 0, 0]], np.int64)
    rep = IndexReport.from_arrays(12, "l2", "sorted", hist)
    assert (rep.n, rep.d, rep.m, rep.k, rep.metric, rep.form, rep.groups) == (40, 12, 3, k, "l2", "sorted", 0)
    assert rep.centroids_used == [8, 1, 3]
    assert rep.largest_share == [1 / 8, 1.0, 0.5]
    assert rep.entropy[0] == pytest.approx(3.0, abs=1e-12) and rep.entropy[1] == 0.0
    assert rep.entropy[2] == pytest.approx(1.5, abs=1e-12)           # 1/2, 1/4, 1/4
    assert entropy_bits(np.zeros(4)) == 0.0
    assert rep.mean_row_error is None and rep.relative_error is None and rep.worst is None
    assert rep.group_size_min is None and rep.group_size_median is None and rep.group_size_max is None


def test_group_sizes():
    hist = np.array([[3, 7]], np.int64)
    rep = IndexReport.from_arrays(4, "cosine", "grouped", hist, group_sizes=[0, 4, 0, 5, 1])
    assert (rep.groups, rep.group_size_min, rep.group_size_median, rep.group_size_max) == (5, 0, 1.0, 5)
    assert rep.lines()[1] == "groups: 5, rows per group min 0 / median 1 / max 5"


def test_errors_relative_error_and_worst_rows():
    err = np.array([1.0, 4.0, 0.5, 4.0, 2.0, 4.0], np.float32)
    nrm = np.array([10.0, 20.0, 5.0, 40.0, 20.0, 60.0], np.float32)
    qerr = np.array([6.0, 9.5], np.float64)
    hist = np.array([[6, 0], [2, 4]], np.int64)
    words = [f"w{i}" for i in range(6)]
    rep = IndexReport.from_arrays(4, "l2", "sorted", hist, None, err, nrm, qerr, worst=4, words=words)
    assert rep.mean_row_error == 15.5 / 6
    assert rep.relative_error == 15.5 / 155.0
    assert rep.quantizer_mean_error == [1.0, 9.5 / 6]
    # largest error first, equal errors in ascending row order
    assert rep.worst == [(1, 4.0, "w1"), (3, 4.0, "w3"), (5, 4.0, "w5"), (4, 2.0, "w4")]
    assert worst_rows(err, 100).tolist() == [1, 3, 5, 4, 0, 2]
    assert worst_rows(err, 0).tolist() == []
    no_words = IndexReport.from_arrays(4, "l2", "sorted", hist, None, err, nrm, qerr, worst=1)
    assert no_words.worst == [(1, 4.0, None)]


def test_reference_quality_is_the_float32_left_to_right_sum():
    rng = np.random.default_rng(7)
    e = (rng.random(5000) * 1000).astype(np.float32)
    s = np.float32(0)
    for x in e:
        s = np.float32(s + x)
    got = reference_quality(e)
    assert isinstance(got, np.float32) and got.view(np.uint32) == s.view(np.uint32)
    assert got != np.float32(math.fsum(e.tolist()))        # the order matters at this length: not a rounded exact sum
    assert reference_quality(np.zeros(0, np.float32)) == 0


# ---- the command -----------------------------------------------------------------------------------------------------
def _report(with_vectors):
    hist = np.array([[2, 2, 0, 0], [1, 1, 1, 1]], np.int64)
    if not with_vectors:
        return IndexReport.from_arrays(6, "cosine", "sorted", hist)
    err = np.array([0.25, 1.0, 0.5, 0.125], np.float32)
    return IndexReport.from_arrays(6, "cosine", "sorted", hist, None, err, np.full(4, 1.0, np.float32),
                                   np.array([1.0, 0.875]), worst=2, words=["a", "b", "c", "d"])


class _FakeIndex:
    metric = "cosine"

    def __init__(self):
        self.calls = []

    def inspect(self, vectors=None, worst=10):
        self.calls.append((vectors, worst))
        return _report(vectors is not None)


def _run(argv, **hooks):
    out = io.BytesIO()
    rc = cli.main(argv, stdout=out, **hooks)
    return rc, out.getvalue().decode("utf-8").splitlines()


def test_cli_inspect_hook_receives_the_parsed_arguments():
    seen = []

    def hook(config, load, vectors):
        seen.append(config)
        return _report(config.vectors is not None)

    rc, lines = _run(["inspect", "-i", "index.bin"], inspect=hook, load=lambda p: None)
    assert rc == 0 and seen == [cli.InspectConfig("index.bin", None, 10)]
    assert lines == ["index: sorted, metric cosine, 4 rows, d = 6, m = 2, k = 4",
                     "quantizer 0: 2 of 4 centroids used, largest share 0.5000, entropy 1.000 of 2.000 bits",
                     "quantizer 1: 4 of 4 centroids used, largest share 0.2500, entropy 2.000 of 2.000 bits"]
    rc, lines = _run(["inspect", "-i", "index.bin", "-v", "vec.txt", "--worst", "2"], inspect=hook, load=lambda p: None)
    assert seen[-1] == cli.InspectConfig("index.bin", "vec.txt", 2)
    assert lines[3:] == ["mean row error: 0.46875", "relative error: 0.46875", "quantizer 0: mean error 0.25",
                         "quantizer 1: mean error 0.21875", "worst: b (row 1): 1", "worst: c (row 2): 0.5"]
    _run(["inspect", "-i", "index.bin", "-v", "vec.txt"], inspect=hook, load=lambda p: None)
    assert seen[-1].worst == 10


def test_cli_inspect_default_runs_through_the_loader():
    index, read = _FakeIndex(), []

    def vectors(path, normalize):
        read.append((path, normalize))
        return "VECTORS"

    rc, lines = _run(["inspect", "-i", "x.bin"], load=lambda p: index, vectors=vectors)
    assert rc == 0 and index.calls == [(None, 10)] and read == [] and len(lines) == 3
    rc, lines = _run(["inspect", "-i", "x.bin", "-v", "v.txt", "-w", "3"], load=lambda p: index, vectors=vectors)
    assert index.calls[-1] == ("VECTORS", 3) and read == [("v.txt", True)]      # a cosine index: read normalised
    assert len(lines) == 9


@pytest.mark.parametrize("argv", [["inspect", "-i", "x.bin", "-w", "3"],            # -w without -v
                                  ["inspect"], ["inspect", "-v", "v.txt"],         # no -i
                                  ["inspect", "-i", "x.bin", "-v", "v.txt", "-w", "0"]])
def test_cli_inspect_rejects(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(argv, stdout=io.BytesIO(), load=lambda p: _FakeIndex(), inspect=lambda *a: _report(False))
    assert e.value.code == 2
    capsys.readouterr()
