"""The host side of the fine codes (gulon_amd/fine.py): the word-to-row maps, on words whose UTF-16 order
(String.compareTo) differs from their code-point order, and the binding table.  No GPU."""
import numpy as np
import pytest

from gulon_amd import fine, native
from gulon_amd.word_vectors import KeyIndexSorted, _jkey

# U+FF5E is one UTF-16 unit above the surrogates; U+1F600 is the pair D83D DE00: String.compareTo puts it FIRST,
# code-point order puts it last
HIGH_BMP, ASTRAL = "\uff5e", "\U0001f600"
WORDS = ["pear", ASTRAL + "b", "apple", HIGH_BMP + "a", ASTRAL + "a", "zebra", HIGH_BMP]
JAVA_ORDER = ["apple", "pear", "zebra", ASTRAL + "a", ASTRAL + "b", HIGH_BMP, HIGH_BMP + "a"]


class StubIndex:
    """What the maps read of a WordIndex: the words in row order, the dimension, word -> row."""

    def __init__(self, words, dimension=4):
        self.words, self.dimension, self.size = list(words), dimension, len(words)

    def row_of(self, word):
        return self.words.index(word) if word in self.words else None


class StubVectors:
    def __init__(self, words, dimension=4, keyed=True):
        self.words, self.dimension = sorted(words, key=_jkey), dimension
        self.key_index = KeyIndexSorted(self.words) if keyed else None


def test_the_words_differ_between_the_two_orders():
    assert sorted(WORDS, key=_jkey) == JAVA_ORDER
    assert sorted(WORDS) != JAVA_ORDER                      # code points: the astral words come last


def test_sorted_rows_is_the_java_order():
    rows = fine.sorted_rows(WORDS)
    assert rows.dtype == np.int32 and [WORDS[r] for r in rows] == JAVA_ORDER
    assert fine.sorted_rows([]).shape == (0,)
    assert fine.sorted_rows(JAVA_ORDER).tolist() == list(range(len(WORDS)))


def test_residual_rows_pairs_index_rows_with_vector_rows():
    index = StubIndex(WORDS)                                # any row order: a grouped index keeps its groups' order
    vectors = StubVectors(WORDS + ["extra", ASTRAL])        # the vectors may hold more words
    words, rows, vector_rows = fine.residual_rows(index, vectors)
    assert words == JAVA_ORDER
    assert [WORDS[r] for r in rows] == JAVA_ORDER
    assert [vectors.words[v] for v in vector_rows] == JAVA_ORDER
    assert rows.dtype == vector_rows.dtype == np.int32
    with pytest.raises(LookupError, match="the index holds the word 'zebra', the word vectors do not"):
        fine.residual_rows(index, StubVectors([w for w in WORDS if w != "zebra"]))
    with pytest.raises(ValueError, match="dimension 5 for an index of dimension 4"):
        fine.residual_rows(index, StubVectors(WORDS, dimension=5))
    with pytest.raises(ValueError, match="key index"):
        fine.residual_rows(index, StubVectors(WORDS, keyed=False))
    assert [a if isinstance(a, list) else a.tolist() for a in fine.residual_rows(StubIndex([]), StubVectors(["x"]))] \
        == [[], [], []]


def test_fine_row_map_follows_the_words():
    index = StubIndex(WORDS)
    fine_index = StubIndex(JAVA_ORDER + ["more"])           # sorted, as build_fine_index writes it
    fmap = fine.fine_row_map(index, fine_index)
    assert fmap.dtype == np.int32 and [fine_index.words[f] for f in fmap] == WORDS
    assert fine.fine_row_map(StubIndex([]), fine_index).tolist() == [0]          # one spare entry
    with pytest.raises(LookupError, match="the index holds the word 'pear', the fine index does not"):
        fine.fine_row_map(index, StubIndex(JAVA_ORDER[:1] + JAVA_ORDER[2:]))


def test_fine_refined_index_checks_its_arguments_before_the_device():
    class Fine(StubIndex):
        metric, _grouped = "l2", False
    index = StubIndex(WORDS)
    with pytest.raises(ValueError, match="candidates must be at least 1"):
        fine.FineRefinedIndex(index, Fine(JAVA_ORDER), 0)
    cosine = Fine(JAVA_ORDER)
    cosine.metric = "cosine"
    grouped = Fine(JAVA_ORDER)
    grouped._grouped = True
    for bad in (cosine, grouped):
        with pytest.raises(ValueError, match="sorted l2"):
            fine.FineRefinedIndex(index, bad, 10)
    with pytest.raises(ValueError, match="fine index of dimension 8 for an index of dimension 4"):
        fine.FineRefinedIndex(index, Fine(JAVA_ORDER, dimension=8), 10)
    with pytest.raises(LookupError, match="the fine index does not"):
        fine.FineRefinedIndex(index, Fine(JAVA_ORDER[:-1]), 10)


def test_restricted_index_refuses_fine_refined():
    from gulon_amd.word_index import RestrictedWordIndex
    with pytest.raises(NotImplementedError, match="fine_refined is not supported by a restricted index"):
        RestrictedWordIndex.fine_refined(object(), None, 10)


def test_binding_table_has_the_six_entry_points():
    names = ["gulon_index_row_residuals", "gulon_grouped_index_row_residuals", "gulon_index_refine_codes_topk",
             "gulon_index_refine_codes_topk_dev", "gulon_grouped_index_refine_codes_topk",
             "gulon_grouped_index_refine_codes_topk_dev"]
    assert [len(native.SIGNATURES[n][1]) for n in names] == [6, 6, 12, 13, 12, 13]
    L = native.lib()                                        # raises if the library lacks one of them
    assert all(hasattr(L, n) for n in names) and L.gulon_abi_version() == 3
