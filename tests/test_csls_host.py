"""The host side of the offset queries and of CSLS translation (gulon_amd/csls.py): the two numpy references
on hand-written cases, the dictionary reader, the report's arithmetic, and the argument handling of `translate`.  No GPU."""
import io

import numpy as np
import pytest

from conftest import bits
from gulon_amd import cli
from gulon_amd.csls import (TranslationReport, mean_similarity_reference, offset_query_reference, read_dictionary,
                            resolve_dictionary, score_lists, translation_scores)

INF = np.inf


def test_offset_reference_orders_by_key_then_row():
    dist = np.array([[1.0, 0.5, 0.25, 0.5, 2.0]], np.float32)
    off = np.array([0.0, 0.25, 0.5, 0.25, 0.0], np.float32)      # keys 1, .75, .75, .75, 2: rows 1, 2, 3 tie
    oi, ok, oc = offset_query_reference(dist, off, 4)
    assert oi.tolist() == [[1, 2, 3, 0]] and ok.tolist() == [[0.75, 0.75, 0.75, 1.0]] and oc.tolist() == [4]
    assert oi.dtype == np.int32 and ok.dtype == np.float32 and oc.dtype == np.int32


def test_offset_reference_excludes_masks_and_pads():
    dist = np.array([[1.0, 0.5, 0.25, 0.5, 2.0], [0.0, 3.0, 1.0, 1.0, 1.0]], np.float32)
    off = np.array([0.0, 0.25, INF, 0.25, 0.0], np.float32)      # row 2 is masked
    oi, ok, oc = offset_query_reference(dist, off, 5, exclude=[1, -1])
    assert oi.tolist() == [[3, 0, 4, -1, -1], [0, 4, 3, 1, -1]] and oc.tolist() == [3, 4]
    assert ok[0].tolist() == [0.75, 1.0, 2.0, INF, INF] and ok[1].tolist() == [0.0, 1.0, 1.25, 3.25, INF]
    # row ids other than the column numbers; the excluded row is named by id
    oi, _, oc = offset_query_reference(dist, off, 2, exclude=[13, 10], rows=[10, 11, 12, 13, 14])
    assert oi.tolist() == [[11, 10], [14, 13]] and oc.tolist() == [2, 2]


def test_offset_reference_keeps_only_finite_keys():
    dist = np.array([[INF, 1.0, np.nan, 3e38, 1.0, 0.5]], np.float32)
    off = np.array([0.0, -INF, 0.0, 3e38, np.nan, -0.0], np.float32)   # inf, -inf, nan, overflow to inf, nan, 0.5
    oi, ok, oc = offset_query_reference(dist, off, 3)
    assert oi.tolist() == [[5, -1, -1]] and oc.tolist() == [1] and ok[0, 0] == 0.5 and np.isposinf(ok[0, 1:]).all()
    none = offset_query_reference(np.zeros((2, 3), np.float32), np.full(3, INF, np.float32), 2)
    assert none[0].tolist() == [[-1, -1]] * 2 and none[2].tolist() == [0, 0]


def test_offset_reference_adds_once_in_binary32():
    d, o = np.float32(1.0), np.float32(2.0 ** -24)               # the sum rounds back to 1 in binary32
    _, ok, _ = offset_query_reference([[d]], [o], 1)
    assert bits(ok)[0, 0] == bits(np.float32(1.0)) and np.float64(d) + np.float64(o) != 1.0
    with pytest.raises(ValueError):
        offset_query_reference(np.zeros((1, 3), np.float32), np.zeros(2, np.float32), 1)
    with pytest.raises(ValueError):
        offset_query_reference(np.zeros((2, 3), np.float32), np.zeros(3, np.float32), 1, exclude=[0])


def test_mean_similarity_reference_by_hand():
    dist = np.array([[0.0, 1.0, 2.0, 4.0], [0.5, 0.5, 0.5, 0.5], [1.0, 1.0, 1.0, 1.0]], np.float32)
    # similarities 1, .5, 0, -1
    assert mean_similarity_reference(dist, [4, 2, 0], 10).tolist() == [0.125, 0.75, 0.0]      # K > kin: the counts decide
    assert mean_similarity_reference(dist, [4, 2, 0], 2).tolist() == [0.75, 0.75, 0.0]
    assert mean_similarity_reference(dist, None, 3).tolist() == [0.5, 0.75, 0.5]
    assert mean_similarity_reference(dist, None, 20).tolist() == [0.125, 0.75, 0.5]
    assert mean_similarity_reference(dist, [9, 9, 9], 20).tolist() == [0.125, 0.75, 0.5]     # never past the list
    out = mean_similarity_reference(dist, [1, 1, 1], 1)
    assert out.dtype == np.float32 and out.tolist() == [1.0, 0.75, 0.5]
    with pytest.raises(ValueError):
        mean_similarity_reference(dist, None, 0)


def test_mean_similarity_reference_rounds_every_step():
    d = np.array([[0.2, 0.6, 1.4]], np.float32)
    s = [np.float32(np.float32(1) - np.float32(np.float32(0.5) * x)) for x in d[0]]
    want = np.float32(np.float32(np.float32(s[0] + s[1]) + s[2]) / np.float32(3))
    assert bits(mean_similarity_reference(d, None, 3))[0] == bits(want)


def test_translation_scores():
    keys = np.array([[0.5, 1.0, INF], [0.25, 0.25, 2.0]], np.float32)
    got = translation_scores(keys, [0.25, 0.5])
    assert got.dtype == np.float32 and got[0].tolist() == [1.25, 0.75, -INF] and got[1].tolist() == [1.25, 1.25, -0.5]
    assert translation_scores(keys[0], 0.25).tolist() == [1.25, 0.75, -INF]


def test_read_dictionary():
    lines = ["the le", "the la", "", "cat\tchat", "  Dog   Chien  "]
    assert read_dictionary(lines) == [("the", "le"), ("the", "la"), ("cat", "chat"), ("Dog", "Chien")]
    assert read_dictionary(lines, lowercase=True)[-1] == ("dog", "chien")
    assert read_dictionary([]) == []
    for bad in ("one", "one two three"):
        with pytest.raises(ValueError, match="line 2"):
            read_dictionary(["a b", bad])


class Words:
    def __init__(self, words):
        self.rows = {w: i for i, w in enumerate(words)}

    def row_of(self, word):
        return self.rows.get(word)


def test_report_arithmetic_with_several_gold_translations():
    source, target = Words(["the", "cat", "dog", "owl"]), Words(["le", "la", "chat", "chien", "hibou"])
    pairs = [("the", "le"), ("the", "la"), ("cat", "chat"), ("dog", "chien"), ("fox", "renard"), ("owl", "chouette"),
             ("emu", "le")]
    rows, gold, skipped = resolve_dictionary(target, source, pairs)
    assert rows == [0, 1, 2] and gold == [{0, 1}, {2}, {3}] and skipped == 3        # owl lost its only translation
    lists = np.array([[4, 1, 0], [0, 1, 2], [0, 1, 2]], np.int32)                  # la second; chat third; chien never
    assert score_lists(lists, [3, 3, 3], gold, (1, 2, 3)) == {1: 0, 2: 1, 3: 2}
    assert score_lists(lists, [3, 2, 3], gold, (1, 2, 3)) == {1: 0, 2: 1, 3: 1}      # beyond a list's count nothing hits
    report = TranslationReport((1, 2, 3), "csls", len(rows), skipped, score_lists(lists, [3, 3, 3], gold, (1, 2, 3)))
    assert report.precision(1) == 0 and report.precision(2) == 1 / 3 and report.precision(3) == 2 / 3
    assert report.lines() == ["csls: @1 0.0000 @2 0.3333 @3 0.6667 (n = 3, skipped 3)"]
    empty = TranslationReport((1, 5), "nn", 0, 2, {1: 0, 5: 0})
    assert empty.precision(5) == 0.0 and empty.line() == "nn: @1 0.0000 @5 0.0000 (n = 0, skipped 2)"


def test_evaluate_checks_before_it_asks_anything():
    from gulon_amd.csls import evaluate_dictionary

    class Side(Words):
        def __init__(self, words, dimension, metric):
            super().__init__(words)
            self.dimension, self.metric = dimension, metric
    with pytest.raises(ValueError, match="method"):
        evaluate_dictionary(Side([], 3, "cosine"), Side([], 3, "cosine"), [], method="mnn")
    with pytest.raises(ValueError, match="dimensions"):
        evaluate_dictionary(Side([], 3, "cosine"), Side([], 4, "cosine"), [])
    with pytest.raises(ValueError, match="cosine"):
        evaluate_dictionary(Side([], 3, "l2"), Side([], 3, "cosine"), [], method="csls")
    with pytest.raises(ValueError, match="ks"):
        evaluate_dictionary(Side([], 3, "cosine"), Side([], 3, "cosine"), [], ks=(5, 1))
    report = evaluate_dictionary(Side(["le"], 3, "l2"), Side(["the"], 3, "l2"), [("a", "le"), ("the", "b")])
    assert (report.asked, report.skipped, report.hits) == (0, 2, {1: 0, 5: 0, 10: 0})


def _usage_error(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(argv, stdout=io.BytesIO())
    assert e.value.code == 2
    return capsys.readouterr().err


def test_translate_argument_errors(capsys):
    base = ["translate", "-i", "target.idx", "-s", "source.txt"]
    assert "invalid choice: 'mnn'" in _usage_error(base + ["--method", "mnn", "words.txt"], capsys)
    assert "exactly one of" in _usage_error(base, capsys)
    assert "exactly one of" in _usage_error(base + ["-e", "dict.txt", "words.txt"], capsys)
    assert "-s/--source" in _usage_error(["translate", "-i", "target.idx", "words.txt"], capsys)
    assert "--exact needs" in _usage_error(base + ["--exact", "words.txt"], capsys)
    assert "only applicable with --exact" in _usage_error(base + ["-v", "target.txt", "words.txt"], capsys)
    assert "not applicable with -R" in _usage_error(base + ["-v", "t.txt", "--exact", "-R", "r.rot", "words.txt"], capsys)
    assert "at least 1" in _usage_error(base + ["-k", "0", "words.txt"], capsys)
    assert "invalid integer" in _usage_error(base + ["-k", "1,5", "words.txt"], capsys)      # depths go with -e
    assert "ascending" in _usage_error(base + ["-k", "5,1", "-e", "dict.txt"], capsys)
    assert "at least 1" in _usage_error(base + ["-n", "0", "words.txt"], capsys)


def test_translate_hands_its_configuration_on():
    seen = []

    def translate(config, write, load, vectors):
        seen.append(config)
        if config.dictionary is not None:
            return TranslationReport(config.ks, config.method, 3, 1, {k: 1 for k in config.ks})
        write("the: le,la\n")
        return None
    out = io.BytesIO()
    assert cli.main(["translate", "-i", "t.idx", "-s", "s.txt", "--method", "csls", "-n", "7", "-k", "3", "--lowercase",
                     "-R", "t.rot", "words.txt"], stdout=out, translate=translate) == 0
    assert seen[-1] == cli.TranslateConfig("t.idx", "s.txt", "words.txt", None, "csls", 7, 3, (1, 5, 10), True, None,
                                           False, "t.rot")
    assert out.getvalue() == b"the: le,la\n"
    out = io.BytesIO()
    assert cli.main(["translate", "-i", "t.idx", "-s", "s.txt", "-e", "dict.txt", "-k", "1,2", "-v", "t.txt", "--exact"],
                    stdout=out, translate=translate) == 0
    assert seen[-1] == cli.TranslateConfig("t.idx", "s.txt", None, "dict.txt", "nn", 10, 10, (1, 2), False, "t.txt", True,
                                           None)
    assert out.getvalue() == b"nn: @1 0.3333 @2 0.3333 (n = 3, skipped 1)\n"
    out = io.BytesIO()
    assert cli.main(["translate", "-i", "t.idx", "-s", "s.txt", "-e", "dict.txt"], stdout=out, translate=translate) == 0
    assert seen[-1].ks == (1, 5, 10) and seen[-1].neighbours == 10


def test_translate_reports_an_unreadable_file(tmp_path, capsys):
    assert cli.main(["translate", "-i", "t.idx", "-s", "s.txt", str(tmp_path / "nowhere.txt")], stdout=io.BytesIO()) == 1
    assert "nowhere.txt" in capsys.readouterr().err
    bad = tmp_path / "dict.txt"
    bad.write_text("a b\nonly\n")
    assert cli.main(["translate", "-i", "t.idx", "-s", "s.txt", "-e", str(bad)], stdout=io.BytesIO()) == 1
    assert "line 2" in capsys.readouterr().err
