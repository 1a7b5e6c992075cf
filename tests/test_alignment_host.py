"""The host side of alignment (gulon_amd/alignment.py): the two numpy references on hand-written cases and
the argument handling of `align` and of `translate -a`.  No GPU."""
import io
from types import SimpleNamespace

import numpy as np
import pytest

from gulon_amd import cli
from gulon_amd.alignment import (MOMENT_ROWS, identical_pairs, mutual_rows_reference, pair_moment_reference,
                                 seed_alignment)
from gulon_amd.rotation import Rotation


def test_pair_moment_reference_by_hand():
    a = np.array([[1, 2], [3, 4], [5, 6]], np.float32)
    b = np.array([[1, 0, -1], [2, 2, 2]], np.float32)
    out, used = pair_moment_reference(a, b, [0, 2], [1, 0])
    assert used == 2 and out.dtype == np.float64 and out.shape == (2, 3)
    assert out.tolist() == [[2 + 5, 2, 2 - 5], [4 + 6, 4, 4 - 6]]
    # the skip rule: a negative row on EITHER side, whatever the other side holds
    out, used = pair_moment_reference(a, b, [0, -1, 2, 1, -7], [1, 0, 0, -1, -1])
    assert used == 2 and out.tolist() == [[7, 2, -3], [10, 4, -2]]
    # duplicates count every time, in any order
    out, used = pair_moment_reference(a, b, [1, 1, 1, 0], [0, 0, 0, 0])
    assert used == 4 and out.tolist() == [[10, 0, -10], [14, 0, -14]]
    out, used = pair_moment_reference(a, b, [], [])
    assert used == 0 and out.tolist() == [[0, 0, 0], [0, 0, 0]]
    for ra, rb in (([0], [0, 1]), ([3], [0]), ([0], [2])):
        with pytest.raises(ValueError):
            pair_moment_reference(a, b, ra, rb)


def test_pair_moment_reference_sums_in_chunks_by_position():
    """1 + v - v + 1 with v = 1e18: the 1s vanish beside v (an ulp of 128).  In chunks of MOMENT_ROWS positions
    (1 + v) + (-v + 1) = 0; one chain over the list gives ((1 + v) - v) + 1 = 1; the exact sum is 2."""
    v = float(np.float32(1e18))
    a = np.zeros((MOMENT_ROWS + 2, 1), np.float32)
    a[0], a[MOMENT_ROWS - 1], a[MOMENT_ROWS], a[MOMENT_ROWS + 1] = 1, v, -v, 1
    b = np.ones((1, 1), np.float32)
    rows = np.arange(len(a))
    out, used = pair_moment_reference(a, b, rows, np.zeros(len(a), np.int64))
    assert used == len(a) and out.tolist() == [[0.0]]
    chain = 0.0
    for x in a[:, 0].astype(np.float64):
        chain += x
    assert chain == 1.0
    # a skipped pair keeps its position: the list is not compacted before it is cut.  Row 0 moved one place up behind
    # a skipped pair, the chunks are unchanged: (skip + 1 + ... + v) + (-v + 1) = 0 ...
    shifted = np.concatenate([[-1], [0], rows[2:]])
    out, used = pair_moment_reference(a, b, shifted, np.zeros(len(a), np.int64))
    assert used == len(a) - 1 and out.tolist() == [[0.0]]
    # ... where the compacted list would have -v in the first chunk: ((1 + v) - v) + (1) = 1
    out, _ = pair_moment_reference(a, b, shifted[1:], np.zeros(len(a) - 1, np.int64))
    assert out.tolist() == [[1.0]]


def test_mutual_rows_reference_by_hand():
    fwd = [2, 0, -1, 7, 1, 3]            # row 2 has no answer, row 3 answers out of range
    bwd = [1, 5, 0, 5]                   # 0 <-> 2 and 1 <-> 0 are mutual; 4 -> 1 -> 5 and 5 -> 3 -> 5: 5 <-> 3 is mutual
    out = mutual_rows_reference(fwd, bwd)
    assert out.dtype == np.int32 and out.tolist() == [2, 0, -1, -1, -1, 3]
    assert mutual_rows_reference([0, 0], [1]).tolist() == [-1, 0]          # one-sided: only the row the target chose
    assert mutual_rows_reference([], [0]).tolist() == [] and mutual_rows_reference([0, 1], []).tolist() == [-1, -1]
    assert mutual_rows_reference([0], [-1]).tolist() == [-1]


def side(words, dimension=3, matrix=True):
    return SimpleNamespace(words=list(words), key_index=None, dimension=dimension, matrix=object() if matrix else None)


def test_identical_pairs_and_the_checks_of_the_seed():
    source, target = side(["the", "a", "taxi", "the", "radio"]), side(["le", "radio", "taxi", "a"])
    assert identical_pairs(source, target) == [("a", "a"), ("taxi", "taxi"), ("radio", "radio")]
    with pytest.raises(ValueError, match="dimensions"):
        seed_alignment(side(["a"], 3), side(["a"], 4), [("a", "a")])
    with pytest.raises(ValueError, match="without rows"):
        seed_alignment(side([], 0, matrix=False), side(["a"]), [])
    with pytest.raises(ValueError, match="none of the 2 dictionary pairs"):
        seed_alignment(source, target, [("the", "la"), ("chat", "le")])


def _usage_error(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(argv, stdout=io.BytesIO())
    assert e.value.code == 2
    return capsys.readouterr().err


def test_align_argument_errors(capsys):
    base = ["align", "-s", "en.vec", "-t", "fr.vec", "-o", "en-fr.map"]
    assert "exactly one of -d/--dictionary and --identical" in _usage_error(base, capsys)
    assert "exactly one of -d/--dictionary and --identical" in _usage_error(base + ["-d", "d.txt", "--identical"], capsys)
    assert "-t/--target" in _usage_error(["align", "-s", "en.vec", "-o", "m", "--identical"], capsys)
    assert "-o/--output" in _usage_error(["align", "-s", "en.vec", "-t", "fr.vec", "--identical"], capsys)
    assert "must not be negative" in _usage_error(base + ["--identical", "--rounds", "-1"], capsys)
    assert "at least 1" in _usage_error(base + ["--identical", "--max-rank", "0"], capsys)
    assert "at least 1" in _usage_error(base + ["--identical", "-n", "0"], capsys)


def test_align_hands_its_configuration_on():
    seen = []

    def align(config, write):
        seen.append(config)
        write("seed: 3 pairs, skipped 1\n")
    out = io.BytesIO()
    assert cli.main(["align", "-s", "en.vec", "-t", "fr.vec", "-d", "en-fr.txt", "-o", "en-fr.map"], stdout=out,
                    align=align) == 0
    assert seen[-1] == cli.AlignConfig("en.vec", "fr.vec", "en-fr.map", "en-fr.txt", False, 5, 15000, 10, False)
    assert out.getvalue() == b"seed: 3 pairs, skipped 1\n"
    assert cli.main(["align", "-s", "en.vec", "-t", "fr.vec", "--identical", "-o", "m", "--rounds", "0", "--max-rank", "99",
                     "-n", "3", "--lowercase"], stdout=io.BytesIO(), align=align) == 0
    assert seen[-1] == cli.AlignConfig("en.vec", "fr.vec", "m", None, True, 0, 99, 3, True)


def test_align_reports_its_errors(tmp_path, capsys):
    config = ["align", "-s", "en.vec", "-t", "fr.vec", "-o", str(tmp_path / "m")]
    assert cli.main(config + ["-d", str(tmp_path / "nowhere.txt")], stdout=io.BytesIO()) == 1
    assert "nowhere.txt" in capsys.readouterr().err
    bad = tmp_path / "dict.txt"
    bad.write_text("a b\nonly\n")
    assert cli.main(config + ["-d", str(bad)], stdout=io.BytesIO()) == 1
    assert "line 2" in capsys.readouterr().err
    good = tmp_path / "good.txt"
    good.write_text("the le\n")

    def unreadable(path):
        raise FileNotFoundError(2, "No such file or directory", path)
    with pytest.raises(cli.AlignError, match="en.vec: No such file"):
        cli.run_align(cli.AlignConfig("en.vec", "fr.vec", "m", str(good)), lambda text: None, vectors=unreadable)
    sides = {"en.vec": side(["the"], 3), "fr.vec": side(["le"], 4), "fr3.vec": side(["la"], 3)}
    with pytest.raises(cli.AlignError, match="3 dimensions, the target 4"):
        cli.run_align(cli.AlignConfig("en.vec", "fr.vec", "m", str(good)), lambda text: None, vectors=sides.get)
    with pytest.raises(cli.AlignError, match="none of the 1 dictionary pairs"):                     # an empty seed
        cli.run_align(cli.AlignConfig("en.vec", "fr3.vec", "m", str(good)), lambda text: None, vectors=sides.get)
    with pytest.raises(cli.AlignError, match="none of the 0 dictionary pairs"):
        cli.run_align(cli.AlignConfig("en.vec", "fr3.vec", "m", None, True), lambda text: None, vectors=sides.get)


def test_translate_hands_the_alignment_on():
    seen = []

    def translate(config, write, load, vectors):
        seen.append(config)
    base = ["translate", "-i", "t.idx", "-s", "s.txt", "-e", "dict.txt"]
    assert cli.main(base + ["-a", "en-fr.map", "-R", "t.rot"], stdout=io.BytesIO(), translate=translate) == 0
    assert seen[-1] == cli.TranslateConfig("t.idx", "s.txt", None, "dict.txt", "nn", 10, 10, (1, 5, 10), False, None, False,
                                           "t.rot", "en-fr.map")
    assert cli.main(base + ["--alignment", "m"], stdout=io.BytesIO(), translate=translate) == 0
    assert seen[-1].alignment == "m" and seen[-1].rotation is None
    assert cli.main(base, stdout=io.BytesIO(), translate=translate) == 0
    assert seen[-1].alignment is None
    # the new field is the last one: the configurations written before it existed compare as they did
    assert seen[-1] == cli.TranslateConfig("t.idx", "s.txt", None, "dict.txt", "nn", 10, 10, (1, 5, 10), False, None, False,
                                           None)


def test_translate_refuses_a_map_of_another_dimension(tmp_path, capsys):
    dictionary = tmp_path / "dict.txt"
    dictionary.write_text("the le\n")
    Rotation.identity(2).save(tmp_path / "two.map")
    index = SimpleNamespace(metric="cosine")
    read = []

    def vectors(path, normalize):
        read.append((path, normalize))
        return SimpleNamespace(words=["the"], dimension=3, matrix=None, key_index=None)
    base = ["translate", "-i", "t.idx", "-s", "s.txt", "-e", str(dictionary)]
    assert cli.main(base + ["-a", str(tmp_path / "two.map")], stdout=io.BytesIO(), load=lambda path: index,
                    vectors=vectors) == 1
    assert "a map of dimension 2 for source vectors of dimension 3" in capsys.readouterr().err
    assert read == [("s.txt", True)]
    assert cli.main(base + ["-a", str(tmp_path / "nowhere.map")], stdout=io.BytesIO(), load=lambda path: index,
                    vectors=vectors) == 1
    assert "nowhere.map" in capsys.readouterr().err
    with pytest.raises(cli.TranslateError, match="map of dimension 2"):
        cli.run_translate(cli.TranslateConfig("t.idx", "s.txt", None, str(dictionary), alignment=str(tmp_path / "two.map")),
                          lambda text: None, lambda path: index, vectors)
