"""Fine codes: a second quantizer over the residuals an index leaves, and its candidates re-ranked against the two-level
reconstruction instead of the original vectors (csrc/fine.hip; DESIGN.md "Fine codes").

For an index I built from the word vectors V, y_r is the vector I's distances are about for row r: ProductQuantizer.decode
of the row for a flat index, centroid(group of r) + decode(r) for a grouped one (what gulon_*_row_errors compares with).
The fine index F of I is an ordinary sorted l2 index file: its words are I's words in String.compareTo order, its vectors
the residuals E[t] = V[word t] - y_{row_I(word t)} (MathUtils.subtract), quantized by ProductQuantizer.apply and encoded
by Index.sorted -- the reference's own build path over another matrix.

fine(k, c, q) over I and F:
  1. cand = I.query(max(c, k), q), nearest approximate first;
  2. q' = the query as the index prepares it (normalised for a cosine index);
  3. heap = TopKHeap(k); for every candidate row r, in result order: z_r = y_r + decode_F(fmap[r]) (y_r formed first, the
     fine coordinate added last, one binary32 add each); heap.update(r, distanceSq(q', z_r));
  4. Result.fromHeap(heap): keys are rows of I, distances those to z_r.
fmap takes a row of I to the row of F that holds the same word; it is built once on the host and kept on the device.
Only the two sets of codes are in HBM: the original vectors are needed to BUILD F, not to query with it."""
import ctypes as C

import numpy as np

from . import native as N
from .refine import RefinedIndex, _DeviceArray
from .word_vectors import _jkey


def sorted_rows(words):
    """The positions of `words` in String.compareTo order (UTF-16 code units; stable): int32 [len(words)]."""
    words = list(words)
    return np.asarray(sorted(range(len(words)), key=lambda i: _jkey(words[i])), np.int32).reshape(-1)


def residual_rows(word_index, vectors):
    """(words, rows, vector_rows) of the residual matrix: the index's words in String.compareTo order, each one's row
    in the index and its row in `vectors` (DeviceWordVectors with a key index).  LookupError for a word the vectors
    lack, as refine.word_row_map."""
    if vectors.dimension != word_index.dimension:
        raise ValueError(f"vectors of dimension {vectors.dimension} for an index of dimension {word_index.dimension}")
    if vectors.key_index is None:
        raise ValueError("the word vectors need a key index (DeviceWordVectors.sorted())")
    rows = sorted_rows(word_index.words)
    words = [word_index.words[r] for r in rows.tolist()]
    lookup = vectors.key_index.lookup
    vector_rows = np.zeros(len(words), np.int32)
    for t, word in enumerate(words):
        v = lookup(word)
        if v is None:
            raise LookupError(f"the index holds the word {word!r}, the word vectors do not")
        vector_rows[t] = v
    return words, rows, vector_rows


def fine_row_map(word_index, fine_word_index):
    """index row -> the row of the fine index that holds the same word: int32, one entry per index row (one spare entry
    for an index without rows).  LookupError for a word the fine index lacks."""
    row_map = np.zeros(max(word_index.size, 1), np.int32)
    for r, word in enumerate(word_index.words):
        f = fine_word_index.row_of(word)
        if f is None:
            raise LookupError(f"the index holds the word {word!r}, the fine index does not")
        row_map[r] = f
    return row_map


def _handle(index):
    """(the device handle, grouped?) of a SortedIndex / GroupedIndex / PQIndex."""
    from .grouped import GroupedIndex
    if isinstance(index, GroupedIndex):
        return index._h, True
    return (index.vector_index._h if hasattr(index, "vector_index") else index._h), False


def index_row_residuals(index, matrix, rows, vector_rows):
    """gulon_*_row_residuals, the raw form: out[t] = matrix[vector_rows[t]] - y_{rows[t]} as a new DeviceMatrix, for a
    PQIndex (a view: its own positions), a SortedIndex or a GroupedIndex."""
    from .matrix import DeviceMatrix
    h, grouped = _handle(index)
    r, v = N.i32(rows).reshape(-1), N.i32(vector_rows).reshape(-1)
    if r.size != v.size:
        raise ValueError(f"{r.size} rows for {v.size} vector rows")
    one = np.zeros(1, np.int32)
    out = C.c_void_p()
    fn = N.lib().gulon_grouped_index_row_residuals if grouped else N.lib().gulon_index_row_residuals
    N.check(fn(h, matrix._h, r if r.size else one, v if v.size else one, r.size, C.byref(out)))
    return DeviceMatrix(out, r.size, matrix.cols)


def row_residuals(word_index, vectors):
    """The residuals an index leaves, as word vectors: the index's words in String.compareTo order, row t =
    vectors[word t] - y_{row of word t}, on the device.  -> DeviceWordVectors with a key index."""
    from .word_vectors import DeviceWordVectors, KeyIndexSorted
    words, rows, vector_rows = residual_rows(word_index, vectors)
    matrix = index_row_residuals(word_index.index, vectors.matrix, rows, vector_rows)
    return DeviceWordVectors(words, matrix, KeyIndexSorted(words))


def build_fine_index(word_index, vectors, pq_config, write=None):
    """The fine index of `word_index` over `vectors` (DeviceWordVectors with a key index; the normalised reading for a
    cosine index): a sorted l2 WordIndex over the residuals, quantized by ProductQuantizer.apply with pq_config and
    encoded by Index.sorted.  write: the task log of build-index (None: silent)."""
    from .build import _quantize, log_task
    from .index import Index
    from .word_index import WordIndex
    residuals = log_task(write, "Computing residuals", lambda: row_residuals(word_index, vectors),
                         lambda e: f"Computed residuals of {e.size} word vectors")
    quantizer = _quantize(residuals.matrix, pq_config, write)
    index = log_task(write, f"Building index for {residuals.size} word vectors",
                     lambda: Index.sorted(residuals.matrix, quantizer, "l2"),
                     f"Built index for {residuals.size} word vectors")
    residuals.matrix.close()
    return WordIndex(residuals.words, index)


def refine_codes_topk(index, fine, queries, cand_rows, k, fine_map=None):
    """gulon_*_refine_codes_topk, the raw form: index a PQIndex / SortedIndex / GroupedIndex, fine a PQIndex /
    SortedIndex over its residuals, cand_rows [B][c] (negative = none), fine_map: candidate id -> row of `fine` (None:
    the identity).  -> (rows [B][k] with -1 after a query's last entry, distances [B][k], counts [B])."""
    h, grouped = _handle(index)
    fh, fine_grouped = _handle(fine)
    if fine_grouped:
        raise ValueError("the fine index is a sorted index")
    q = N.f32(queries)
    cand = N.i32(cand_rows)
    b, c = cand.shape
    rows, dist = np.full((b, k), -1, np.int32), np.zeros((b, k), np.float32)
    counts = np.zeros(b, np.int32)
    one_f, one_i = np.zeros(1, np.float32), np.zeros(1, np.int32)
    fmap = None if fine_map is None else N.i32(fine_map).reshape(-1)
    fn = N.lib().gulon_grouped_index_refine_codes_topk if grouped else N.lib().gulon_index_refine_codes_topk
    N.check(fn(h, fh, q.reshape(-1) if q.size else one_f, b, cand.reshape(-1) if cand.size else one_i, c,
               None if fmap is None else (fmap if fmap.size else one_i).ctypes.data, 0 if fmap is None else fmap.size, k,
               rows.reshape(-1) if b else one_i, dist.reshape(-1) if b else one_f, counts if b else one_i))
    return rows, dist, counts


class FineRefinedIndex(RefinedIndex):
    """A WordIndex whose results are re-ranked against its fine index: RefinedIndex's query surface, each call taking
    `candidates` index results per query and keeping the k nearest by their distance to the two-level reconstruction
    y_r + decode_F(row).  `fine_word_index`: a sorted l2 WordIndex of the same dimension that holds every word of
    `word_index` (build_fine_index, or such a file through WordIndex.load)."""

    def __init__(self, word_index, fine_word_index, candidates):
        self.word_index, self.fine, self.candidates = word_index, fine_word_index, int(candidates)
        if self.candidates < 1:
            raise ValueError("candidates must be at least 1")
        if getattr(fine_word_index, "_grouped", False) or fine_word_index.metric != "l2":
            raise ValueError("the fine index must be a sorted l2 index")
        if fine_word_index.dimension != word_index.dimension:
            raise ValueError(f"a fine index of dimension {fine_word_index.dimension} for an index of dimension "
                             f"{word_index.dimension}")
        row_map = fine_row_map(word_index, fine_word_index)
        self._map, self._work = _DeviceArray(), [_DeviceArray() for _ in range(5)]
        self._map.upload(row_map)

    def _refine(self, k, prepared, cand):
        """One batch: prepared [B][d] = q', cand [B][c_eff] index rows (-1 = none) -> (rows, distances, counts)."""
        b, c = cand.shape
        rows, dist = np.full((b, k), -1, np.int32), np.zeros((b, k), np.float32)
        counts = np.zeros(b, np.int32)
        if b == 0:
            return rows, dist, counts
        h, grouped = _handle(self.word_index.index)
        fn = N.lib().gulon_grouped_index_refine_codes_topk_dev if grouped else N.lib().gulon_index_refine_codes_topk_dev
        dq, dc, doi, dod, doc = self._work
        dq.upload(N.f32(prepared))
        dc.upload(N.i32(cand))
        doi.ensure(rows.nbytes), dod.ensure(dist.nbytes), doc.ensure(counts.nbytes)
        N.check(fn(h, _handle(self.fine.index)[0], dq.ptr, b, dc.ptr, c, self._map.ptr, self.word_index.size, k, doi.ptr,
                   dod.ptr, doc.ptr, None))
        doi.download(rows), dod.download(dist), doc.download(counts)
        if (counts < 0).any():                       # the map is built from the fine index's own key index
            raise ValueError("requirement failed: a candidate row has no row in the fine index")
        return rows, dist, counts
