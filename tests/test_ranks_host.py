"""The host side of the rank queries (gulon_amd/ranks.py): the numpy reference against
csls.offset_query_reference at k = n and on hand-written cases, the report's arithmetic, and the argument handling of
`translate --ranks`.  No GPU."""
import io

import numpy as np
import pytest

from conftest import bits
from gulon_amd import cli
from gulon_amd.csls import TranslationReport, offset_query_reference
from gulon_amd.ranks import RankReport, gold_lists, rank_query_reference

INF = np.inf


def test_reference_is_the_position_in_the_offset_query_at_full_depth():
    rng = np.random.default_rng(3)
    b, n = 23, 61
    dist = rng.integers(0, 6, (b, n)).astype(np.float32) * np.float32(0.25)       # few values: equal keys occur
    offsets = np.array([0.0, 0.25, 0.5, INF], np.float32)[rng.integers(0, 4, n)]
    ids = np.arange(100, 100 + n)
    exclude = np.where(np.arange(b) % 3 == 0, ids[rng.integers(0, n, b)], -1)
    gold = [ids[rng.integers(0, n, q % 4)].tolist() for q in range(b)]            # 0 .. 3 rows, with repeats
    gold[5] = [7, 100 + n]                                                          # rows that are no column
    rank, row, key, total = rank_query_reference(dist, offsets, gold, exclude, rows=ids)
    oi, ok, oc = offset_query_reference(dist, offsets, n, exclude, rows=ids)
    seen = set()
    for q in range(b):
        assert total[q] == oc[q]
        at = [j for j in range(oc[q]) if oi[q, j] in gold[q]]
        if not at:
            assert (rank[q], row[q]) == (-1, -1) and np.isposinf(key[q])
            seen.add("none")
        else:
            assert (rank[q], row[q]) == (at[0], oi[q, at[0]]) and bits(key[q]) == bits(ok[q, at[0]])
            seen.add("tie" if at[0] and ok[q, at[0] - 1] == ok[q, at[0]] else "plain")
    assert seen == {"none", "tie", "plain"}
    assert rank[5] == -1 and rank.dtype == row.dtype == total.dtype == np.int32 and key.dtype == np.float32


def test_reference_by_hand():
    dist = np.array([[1.0, 0.5, 0.5, 2.0, 0.25],
                     [np.nan] * 5], np.float32)
    offsets = np.array([0.0, 0.5, 0.5, INF, 1.0], np.float32)
    # keys of query 0: 1.0, 1.0, 1.0, inf, 1.25 -- rows 0, 1, 2 tie and the row id decides
    got = rank_query_reference(dist, offsets, [[2, 4], [0]])
    assert [a.tolist() for a in got] == [[2, -1], [2, -1], [1.0, INF], [4, 0]]
    got = rank_query_reference(dist, offsets, [[4, 2, 1], [0]], exclude=[1, -1])  # the best is not the first entry
    assert [a.tolist() for a in got] == [[1, -1], [2, -1], [1.0, INF], [3, 0]]
    got = rank_query_reference(dist[:1], offsets, [[3]])                           # a masked gold row
    assert [a.tolist() for a in got] == [[-1], [-1], [INF], [4]]
    got = rank_query_reference(dist[:1], offsets, [[1]], exclude=[1])              # the excluded gold row
    assert [a.tolist() for a in got] == [[-1], [-1], [INF], [3]]
    got = rank_query_reference(dist[:1], offsets, [[]])                            # an empty list
    assert [a.tolist() for a in got] == [[-1], [-1], [INF], [4]]
    got = rank_query_reference(dist[:1], None, [[0]])                              # no offsets: + 0
    assert [a.tolist() for a in got] == [[3], [0], [1.0], [5]]
    with pytest.raises(ValueError):
        rank_query_reference(dist, offsets, [[0]])
    with pytest.raises(ValueError):
        rank_query_reference(dist, offsets[:-1], [[0], [0]])


def test_reference_signed_zeros_are_equal_and_the_addition_is_one_binary32_rounding():
    dist = np.array([[0.0, 0.0, 1.0]], np.float32)
    offsets = np.array([0.0, -0.0, -1.0], np.float32)                               # keys +0, +0 (0 + -0), 0: all equal
    rank, row, key, total = rank_query_reference(dist, offsets, [[2]])
    assert (rank[0], row[0], total[0]) == (2, 2, 3)
    dist = np.array([[-0.0, 0.0]], np.float32)                                      # -0 + -0 = -0, and -0 == +0
    rank, row, key, _ = rank_query_reference(dist, np.array([-0.0, 0.0], np.float32), [[1]])
    assert (rank[0], row[0]) == (1, 1)
    rank, row, key, _ = rank_query_reference(dist, np.array([-0.0, 0.0], np.float32), [[0]])
    assert (rank[0], row[0]) == (0, 0) and bits(key)[0] == 0x80000000
    # 1 + 2^-24 rounds to 1 in binary32 (ties to even), so the two rows tie and the id decides; in binary64 row 0 would
    # come second
    dist = np.array([[1.0, 1.0]], np.float32)
    offsets = np.array([2.0 ** -24, 0.0], np.float32)
    rank, row, key, _ = rank_query_reference(dist, offsets, [[0]])
    assert (rank[0], row[0]) == (0, 0) and bits(key)[0] == bits(np.float32(1.0))
    big = np.array([[3e38, 1.0]], np.float32)                                       # the sum overflows: no candidate
    rank, _, _, total = rank_query_reference(big, np.array([3e38, 0.0], np.float32), [[0]])
    assert (rank[0], total[0]) == (-1, 1)


def test_gold_lists_in_csr_form():
    off, rows = gold_lists([[3, 1], [], (5,)], 3)
    assert off.tolist() == [0, 2, 2, 3] and rows.tolist() == [3, 1, 5] and off.dtype == rows.dtype == np.int32
    off, rows = gold_lists([], 0)
    assert off.tolist() == [0] and rows.size == 0
    with pytest.raises(ValueError):
        gold_lists([[1]], 2)


def test_report_arithmetic_by_hand():
    report = RankReport((1, 5, 100), "csls", 6, 2, np.array([0, 0, 3, 99, -1, 7]))
    assert report.unranked == 1 and report.ranked.tolist() == [0, 0, 3, 99, 7]
    assert report.mrr == pytest.approx((1 + 1 + 1 / 4 + 1 / 100 + 0 + 1 / 8) / 6, rel=1e-12)
    assert report.median_rank == 4.0 and report.mean_rank == pytest.approx((1 + 1 + 4 + 100 + 8) / 5)
    assert [report.hits(k) for k in (1, 4, 8, 99, 100, 1000)] == [2, 3, 4, 4, 5, 5]
    assert report.precision(5) == pytest.approx(3 / 6)
    assert report.line() == ("csls ranks: mrr 0.3975 median 4 mean 22.80 @1 0.3333 @5 0.5000 @100 0.8333 "
                             "(n = 6, unranked 1, skipped 2)")
    assert report.lines() == [report.line()]
    report.precision_report = TranslationReport((1, 5), "csls", 6, 2, {1: 2, 5: 3})
    assert report.lines() == ["csls: @1 0.3333 @5 0.5000 (n = 6, skipped 2)", report.line()]
    even = RankReport((1,), "nn", 2, 0, np.array([0, 1]))
    assert even.median_rank == 1.5 and " median 1.5 " in even.line()
    empty = RankReport((1, 5), "nn", 0, 3)
    assert (empty.mrr, empty.median_rank, empty.mean_rank, empty.hits(5), empty.unranked) == (0.0, 0.0, 0.0, 0, 0)
    assert empty.line() == "nn ranks: mrr 0.0000 median 0 mean 0.00 @1 0.0000 @5 0.0000 (n = 0, unranked 0, skipped 3)"
    none_ranked = RankReport((1,), "nn", 2, 0, np.array([-1, -1]))
    assert (none_ranked.mrr, none_ranked.median_rank, none_ranked.unranked) == (0.0, 0.0, 2)


def test_evaluate_checks_before_it_asks_anything():
    from gulon_amd.ranks import evaluate_dictionary_ranks

    class Side:
        def __init__(self, words, dimension, metric):
            self.words, self.dimension, self.metric = words, dimension, metric

        def row_of(self, w):
            return self.words.index(w) if w in self.words else None
    with pytest.raises(ValueError, match="unknown method"):
        evaluate_dictionary_ranks(Side([], 3, "l2"), Side([], 3, "l2"), [], method="mnn")
    with pytest.raises(ValueError, match="dimensions"):
        evaluate_dictionary_ranks(Side([], 3, "l2"), Side([], 4, "l2"), [])
    with pytest.raises(ValueError, match="cosine"):
        evaluate_dictionary_ranks(Side([], 3, "l2"), Side([], 3, "cosine"), [], method="csls")
    with pytest.raises(ValueError, match="ks"):
        evaluate_dictionary_ranks(Side([], 3, "cosine"), Side([], 3, "cosine"), [], ks=(5, 1))


def test_wrapped_indexes_refuse():
    from gulon_amd.grouped import GroupedIndex
    from gulon_amd.rotation import RotatedWordIndex
    from gulon_amd.word_index import RestrictedWordIndex
    for cls in (GroupedIndex, RotatedWordIndex, RestrictedWordIndex):
        with pytest.raises(NotImplementedError, match="rank queries"):
            cls.batch_query_rank_raw(None, np.zeros((1, 3), np.float32), [[0]])


def _usage_error(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(argv, stdout=io.BytesIO())
    assert e.value.code == 2
    return capsys.readouterr().err


def test_ranks_argument_errors(capsys):
    base = ["translate", "-i", "target.idx", "-s", "source.txt"]
    assert "--ranks is only applicable with -e" in _usage_error(base + ["--ranks", "words.txt"], capsys)
    assert "ascending" in _usage_error(base + ["--ranks", "-k", "100,64", "-e", "dict.txt"], capsys)


def test_translate_hands_the_flag_on():
    seen = []

    def translate(config, write, load, vectors):
        seen.append(config)
        report = RankReport(config.ks, config.method, 4, 1, np.array([0, 2, 70, -1]))
        report.precision_report = TranslationReport(config.ks, config.method, 4, 1, {k: report.hits(k) for k in config.ks})
        return report if config.ranks else report.precision_report
    out = io.BytesIO()
    argv = ["translate", "-i", "t.idx", "-s", "s.txt", "--method", "csls", "-e", "dict.txt", "-k", "1,64,100"]
    assert cli.main(argv + ["--ranks"], stdout=out, translate=translate) == 0
    assert seen[-1] == cli.TranslateConfig("t.idx", "s.txt", None, "dict.txt", "csls", 10, 10, (1, 64, 100), False, None,
                                           False, None, None, True)
    assert out.getvalue() == (b"csls: @1 0.2500 @64 0.5000 @100 0.7500 (n = 4, skipped 1)\n"
                              b"csls ranks: mrr 0.3369 median 3 mean 25.00 @1 0.2500 @64 0.5000 @100 0.7500 "
                              b"(n = 4, unranked 1, skipped 1)\n")
    out = io.BytesIO()
    assert cli.main(argv, stdout=out, translate=translate) == 0                     # without the flag: one line, as before
    assert seen[-1].ranks is False and seen[-1] == cli.TranslateConfig("t.idx", "s.txt", None, "dict.txt", "csls", 10, 10,
                                                                       (1, 64, 100))
    assert out.getvalue() == b"csls: @1 0.2500 @64 0.5000 @100 0.7500 (n = 4, skipped 1)\n"
