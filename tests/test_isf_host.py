"""The host side of the inverted softmax (gulon_amd/softmax.py, csls.py, ranks.py, cli.py): the numpy
reference on hand-made matrices, the offsets and probabilities behind L, the checks that come before anything is asked
of a device, and the `translate` command's new options."""
import io
import math

import numpy as np
import pytest

from gulon_amd import cli
from gulon_amd.csls import METHODS, TranslationReport
from gulon_amd.softmax import isf_offsets_from, isf_probabilities, logsumexp_reference


# ---- the reference ----------------------------------------------------------------------------------------------------------

def test_copies_at_distance_zero_give_log_n():
    for n in (1, 2, 7, 1000):
        L, terms = logsumexp_reference(np.zeros((2, n), np.float32), 30.0)
        assert terms.tolist() == [n, n] and terms.dtype == np.int32 and L.dtype == np.float64
        assert L.tolist() == [math.log(n)] * 2


def test_the_reference_by_hand():
    dist = np.array([[0.0, 0.5, 2.0], [1.0, 1.0, 1.0]], np.float32)
    L, terms = logsumexp_reference(dist, 4.0)                    # z = -2 d
    assert terms.tolist() == [3, 3]
    assert abs(L[0] - math.log(1.0 + math.exp(-1.0) + math.exp(-4.0))) < 1e-15
    assert abs(L[1] - (math.log(3) - 2.0)) < 1e-15


def test_a_masked_column_and_an_excluded_row():
    dist = np.array([[0.0, np.inf, 0.0, np.nan], [0.0, 0.0, 0.0, 0.0]], np.float32)
    L, terms = logsumexp_reference(dist, 30.0)
    assert terms.tolist() == [2, 4] and L.tolist() == [math.log(2), math.log(4)]
    L, terms = logsumexp_reference(dist, 30.0, exclude=[12, 13], rows=[10, 11, 12, 13])
    assert terms.tolist() == [1, 3] and L.tolist() == [0.0, math.log(3)]
    L, terms = logsumexp_reference(dist, 30.0, exclude=[-1, 2])  # without rows: the column number
    assert terms.tolist() == [2, 3]


def test_no_terms_and_underflow():
    dist = np.array([[np.inf, np.nan], [0.0, np.inf], [1e4, 2e4]], np.float32)
    L, terms = logsumexp_reference(dist, 30.0, exclude=[-1, 0, -1])
    assert terms.tolist() == [0, 0, 2] and np.isneginf(L).all()  # the last: both terms underflow to 0
    L, terms = logsumexp_reference(np.zeros((0, 3), np.float32), 30.0)
    assert L.shape == (0,) and terms.shape == (0,)
    for bad in ((np.zeros(3), 30.0, None, None), (np.zeros((2, 3)), 30.0, [1], None), (np.zeros((2, 3)), 30.0, None, [1, 2]),
                (np.zeros((2, 3)), 0.0, None, None), (np.zeros((2, 3)), float("nan"), None, None)):
        with pytest.raises(ValueError):
            logsumexp_reference(*bad)


def test_beta_is_taken_in_binary32():
    dist = np.array([[0.25, 1.5]], np.float32)
    beta = 0.1                                                   # not a float32: the entry point sees float32(0.1)
    scale = -0.5 * float(np.float32(beta))
    assert logsumexp_reference(dist, beta)[0][0] == math.log(math.fsum(np.exp(dist[0].astype(np.float64) * scale).tolist()))


# ---- offsets and probabilities ----------------------------------------------------------------------------------------------

def test_offsets_from():
    L = np.array([math.log(5), -3.25, -np.inf, 7.0])
    off = isf_offsets_from(L, [5, 2, 0, 9], 30.0)
    assert off.dtype == np.float32 and off.shape == (4,)
    assert off[0] == np.float32((2.0 / 30.0) * math.log(5)) and off[1] == np.float32((2.0 / 30.0) * -3.25)
    assert np.isposinf(off[2]) and off[3] == np.float32(14.0 / 30.0)
    assert np.isposinf(isf_offsets_from([123.0], [0], 30.0)[0])  # no term: masked, whatever L says
    with pytest.raises(ValueError, match=r"L\[1\].*beta too large for these distances"):
        isf_offsets_from([0.0, -np.inf], [3, 3], 30.0)
    with pytest.raises(ValueError, match="beta too large for these distances"):
        isf_offsets_from([np.nan], [1], 30.0)
    with pytest.raises(ValueError, match="beta"):
        isf_offsets_from([0.0], [1], -1.0)
    with pytest.raises(ValueError):
        isf_offsets_from([0.0, 1.0], [1], 30.0)


def test_probabilities_sum_to_one_over_the_sources():
    rng = np.random.default_rng(3)
    dist = (rng.random((40, 6)) * 2).astype(np.float32)          # [sources][targets]
    beta = 10.0
    L, terms = logsumexp_reference(dist.T, beta)                 # per target over the sources
    off = (2.0 / beta) * L                                       # in float64: the identity itself
    p = isf_probabilities(dist.astype(np.float64) + off[None, :], beta)
    assert p.shape == (40, 6) and np.allclose(p.sum(axis=0), 1.0, rtol=0, atol=1e-12)
    assert isf_probabilities(np.array([np.inf], np.float32), beta)[0] == 0.0
    assert isf_probabilities(np.float32(0.5), 4.0) == np.exp(-1.0)
    with pytest.raises(ValueError, match="beta"):
        isf_probabilities([0.0], 0.0)


# ---- the checks before anything is asked --------------------------------------------------------------------------------------

def test_methods():
    assert METHODS == ("nn", "csls", "isf")


class Words:
    def __init__(self, words, dimension, metric):
        self.rows = {w: i for i, w in enumerate(words)}
        self.dimension, self.metric = dimension, metric

    def row_of(self, word):
        return self.rows.get(word)


def test_evaluations_check_before_they_ask_anything():
    from gulon_amd.csls import evaluate_dictionary, translate_words
    from gulon_amd.ranks import evaluate_dictionary_ranks
    for evaluate in (evaluate_dictionary, evaluate_dictionary_ranks):
        with pytest.raises(ValueError, match="method"):
            evaluate(Words([], 3, "cosine"), Words([], 3, "cosine"), [], method="invsm")
        with pytest.raises(ValueError, match="dimensions"):
            evaluate(Words([], 3, "cosine"), Words([], 4, "cosine"), [], method="isf")
        with pytest.raises(ValueError, match="cosine"):
            evaluate(Words([], 3, "l2"), Words([], 3, "cosine"), [], method="isf", beta=10.0, sources=5)
    with pytest.raises(ValueError, match="cosine"):
        translate_words(Words([], 3, "l2"), Words([], 3, "cosine"), ["a"], 3, "isf", beta=10.0)
    # a dictionary without an askable word computes no offsets: the new keywords are accepted and nothing is asked
    report = evaluate_dictionary(Words(["le"], 3, "cosine"), Words(["the"], 3, "cosine"), [("a", "le")], (1, 5), "isf", 10,
                                 beta=10.0, sources=1)
    assert (report.method, report.asked, report.skipped) == ("isf", 0, 1)


def stub_exact(rows, cols, metric, frm=0, until=None):
    """An ExactIndex without a handle: what isf_offsets reads before it asks the device anything."""
    from gulon_amd.exact import ExactIndex

    class Matrix:
        pass
    ix = object.__new__(ExactIndex)
    ix.matrix, ix.metric, ix._h = Matrix(), metric, None
    ix.matrix.rows, ix.matrix.cols = rows, cols
    ix.frm, ix.until = frm, rows if until is None else until
    return ix


def test_isf_offsets_checks_before_anything_is_launched():
    from gulon_amd.csls import isf_offsets
    target, source = stub_exact(10, 4, "cosine"), stub_exact(8, 4, "cosine")
    for beta in (0.0, -30.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="beta"):
            isf_offsets(target, source, beta)
    for sources in (0, -1, 9):
        with pytest.raises(ValueError, match=r"sources = .* outside \[1, 8\]"):
            isf_offsets(target, source, 30.0, sources)
    with pytest.raises(ValueError, match="cosine"):
        isf_offsets(stub_exact(10, 4, "l2"), source)
    with pytest.raises(ValueError, match="dimensions"):
        isf_offsets(stub_exact(10, 5, "cosine"), source)
    with pytest.raises(NotImplementedError):
        isf_offsets(target, object())                            # no index at all
    with pytest.raises(ValueError, match="beta"):
        stub_exact(8, 4, "l2").batch_query_logsumexp(np.zeros((1, 4), np.float32), 0.0)


def test_normalize_rows_has_the_bits_of_normalize():
    from gulon_amd.exact import normalize_rows
    from gulon_amd.index import normalize
    rng = np.random.default_rng(9)
    for d in (1, 3, 32, 33):
        q = (rng.standard_normal((20, d)) * 3).astype(np.float32)
        assert np.array_equal(normalize_rows(q).view(np.uint32), np.stack([normalize(r) for r in q]).view(np.uint32))


# ---- the command --------------------------------------------------------------------------------------------------------------

def _usage_error(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(argv, stdout=io.BytesIO())
    assert e.value.code == 2
    return capsys.readouterr().err


def test_translate_argument_errors(capsys):
    base = ["translate", "-i", "target.idx", "-s", "source.txt"]
    for method in ([], ["--method", "nn"], ["--method", "csls"]):
        assert "--beta is only applicable with --method isf" in _usage_error(base + method + ["--beta", "10", "w.txt"], capsys)
        assert "--isf-sources is only applicable with --method isf" in \
            _usage_error(base + method + ["--isf-sources", "10", "-e", "d.txt"], capsys)
    isf = base + ["--method", "isf"]
    for bad in ("0", "-3", "nan", "inf", "ten"):
        assert "--beta" in _usage_error(isf + ["--beta", bad, "w.txt"], capsys)
    for bad in ("0", "-3", "1.5"):
        assert "--isf-sources" in _usage_error(isf + ["--isf-sources", bad, "w.txt"], capsys)
    assert "only applicable with -e" in _usage_error(isf + ["--ranks", "w.txt"], capsys)


def test_translate_hands_its_configuration_on():
    seen = []

    def translate(config, write, load, vectors):
        seen.append(config)
        if config.dictionary is not None:
            return TranslationReport(config.ks, config.method, 3, 1, {k: 1 for k in config.ks})
        write("the: le,la\n")
        return None
    old = ("t.idx", "s.txt", "words.txt", None, "isf", 10, 3, (1, 5, 10), False, None, False, None, None, False)
    out = io.BytesIO()
    assert cli.main(["translate", "-i", "t.idx", "-s", "s.txt", "--method", "isf", "-k", "3", "words.txt"], stdout=out,
                    translate=translate) == 0
    assert seen[-1] == cli.IsfTranslateConfig(*old) == cli.IsfTranslateConfig(*old, 30.0, None)
    assert isinstance(seen[-1], cli.TranslateConfig) and (seen[-1].beta, seen[-1].isf_sources) == (30.0, None)
    assert out.getvalue() == b"the: le,la\n"
    out = io.BytesIO()
    assert cli.main(["translate", "-i", "t.idx", "-s", "s.txt", "--method", "isf", "--beta", "12.5", "--isf-sources", "400",
                     "-e", "dict.txt", "--ranks"], stdout=out, translate=translate) == 0
    assert seen[-1] == cli.IsfTranslateConfig("t.idx", "s.txt", None, "dict.txt", "isf", 10, 10, (1, 5, 10), False, None,
                                              False, None, None, True, 12.5, 400)
    assert out.getvalue() == b"isf: @1 0.3333 @5 0.3333 @10 0.3333 (n = 3, skipped 1)\n"
    # the new fields come last, and the configurations of the other methods are what they were
    names = list(cli.IsfTranslateConfig.__dataclass_fields__)
    assert names[-2:] == ["beta", "isf_sources"] and names[:-2] == list(cli.TranslateConfig.__dataclass_fields__)
    assert cli.main(["translate", "-i", "t.idx", "-s", "s.txt", "--method", "csls", "-n", "7", "words.txt"],
                    stdout=io.BytesIO(), translate=translate) == 0
    assert type(seen[-1]) is cli.TranslateConfig
    assert seen[-1] == cli.TranslateConfig("t.idx", "s.txt", "words.txt", None, "csls", 7, 10, (1, 5, 10), False, None,
                                           False, None, None, False)
    assert (seen[-1].beta, seen[-1].isf_sources) == (30.0, None)  # what run_translate reads for nn and csls


def test_report_lines():
    from gulon_amd.ranks import RankReport
    report = TranslationReport((1, 5), "isf", 4, 2, {1: 1, 5: 3})
    assert report.lines() == ["isf: @1 0.2500 @5 0.7500 (n = 4, skipped 2)"]
    ranks = RankReport((1, 100), "isf", 4, 2, np.array([0, 3, -1, 70]), report)
    assert ranks.lines() == [report.line(), "isf ranks: mrr 0.3160 median 4 mean 25.33 @1 0.2500 @100 0.7500 "
                                            "(n = 4, unranked 1, skipped 2)"]


def test_isf_sources_are_counted_in_file_order():
    """sorted() leaves behind the line every row came from, and --isf-sources N names the rows of the first N lines."""
    from gulon_amd.word_vectors import DeviceWordVectors
    read = DeviceWordVectors(["the", "of", "and", "a", "zebra", "aardvark"], None)       # by falling frequency
    in_word_order = read.sorted()
    assert in_word_order.words == ["a", "aardvark", "and", "of", "the", "zebra"]
    assert in_word_order.file_rows.tolist() == [3, 5, 2, 1, 0, 4]
    assert cli._frequent_rows(None, in_word_order) is None
    assert cli._frequent_rows(3, in_word_order).tolist() == [2, 3, 4]            # the, of, and -- not a, aardvark, and
    assert cli._frequent_rows(6, in_word_order).tolist() == [0, 1, 2, 3, 4, 5]
    assert cli._frequent_rows(3, read) == 3                                      # file order kept: the first 3 rows
    for bad in (0, 7):
        with pytest.raises(ValueError, match="isf-sources"):
            cli._frequent_rows(bad, in_word_order)


def test_sources_are_checked_before_anything_is_made():
    from gulon_amd.csls import _checked_sources
    src = stub_exact(10, 4, "cosine", 2, 8)
    assert _checked_sources(src, None) is None and _checked_sources(src, np.int64(6)) == 6
    assert _checked_sources(src, [7, 2, 5]).tolist() == [7, 2, 5] and _checked_sources(src, [7, 2]).dtype == np.int32
    for bad in (0, 7, [], [1], [8], [3, 3]):
        with pytest.raises(ValueError, match="sources"):
            _checked_sources(src, bad)
