"""Refined queries: an index's candidates re-ranked by their exact distance to the original vectors (csrc/refine.hip).

refined(k, c, q) over an index I and a vector matrix V:
  1. cand = I.query(max(c, k), q) -- today's result, nearest approximate first;
  2. q' = the query as the index prepares it (MathUtils.normalize(q) for a cosine index, Index.scala:324-331);
  3. heap = TopKHeap(k); for every candidate row, in result order: heap.update(row, distanceSq(q', V[map[row]])),
     map taking an index row to the row of V that holds the same word;
  4. Result.fromHeap(heap): keys are INDEX rows, distances the exact ones, ascending.
The vectors and the map stay on the device; a batch uploads its queries and candidate rows."""
import ctypes as C
from typing import List, Optional

import numpy as np

from . import native as N
from .word_index import WordResult


def refine_topk(matrix, queries, cand_rows, k, row_map=None):
    """gulon_refine_topk, the raw form: cand_rows [B][c] (negative = none), row_map: candidate id -> row of `matrix`
    (None: the identity).  -> (rows [B][k] with -1 after a query's last entry, distances [B][k], counts [B])."""
    q = N.f32(queries)
    cand = N.i32(cand_rows)
    b, c = cand.shape
    rows, dist = np.full((b, k), -1, np.int32), np.zeros((b, k), np.float32)
    counts = np.zeros(b, np.int32)
    one_f, one_i = np.zeros(1, np.float32), np.zeros(1, np.int32)
    rmap = None if row_map is None else N.i32(row_map).reshape(-1)
    N.check(N.lib().gulon_refine_topk(matrix._h, q.reshape(-1) if q.size else one_f, b,
                                      cand.reshape(-1) if cand.size else one_i, c,
                                      None if rmap is None else (rmap if rmap.size else one_i).ctypes.data,
                                      0 if rmap is None else rmap.size, k, rows.reshape(-1) if b else one_i,
                                      dist.reshape(-1) if b else one_f, counts if b else one_i))
    return rows, dist, counts


class _DeviceArray:
    """A device allocation that grows on demand (gulon_dev_malloc)."""

    def __init__(self):
        self.ptr, self.bytes = C.c_void_p(), 0

    def ensure(self, nbytes):
        if nbytes > self.bytes:
            self.free()
            N.check(N.lib().gulon_dev_malloc(C.byref(self.ptr), nbytes))
            self.bytes = nbytes
        return self.ptr

    def upload(self, a):
        self.ensure(a.nbytes)
        N.check(N.lib().gulon_memcpy_h2d(self.ptr, a.ctypes.data, a.nbytes))
        return self.ptr

    def download(self, a):
        N.check(N.lib().gulon_memcpy_d2h(a.ctypes.data, self.ptr, a.nbytes))
        return a

    def free(self):
        if self.ptr.value:
            N.lib().gulon_dev_free(self.ptr)
        self.ptr, self.bytes = C.c_void_p(), 0


def word_row_map(word_index, vectors):
    """index row -> the row of `vectors` (DeviceWordVectors with a key index) that holds the same word: int32, one
    entry per index row (one spare entry for an index without rows).  The vectors must have the index's dimension and
    hold every word of the index."""
    if vectors.dimension != word_index.dimension:
        raise ValueError(f"vectors of dimension {vectors.dimension} for an index of dimension {word_index.dimension}")
    if vectors.key_index is None:
        raise ValueError("the word vectors need a key index (DeviceWordVectors.sorted())")
    lookup = vectors.key_index.lookup
    row_map = np.zeros(max(word_index.size, 1), np.int32)
    for r, word in enumerate(word_index.words):
        v = lookup(word)
        if v is None:
            raise LookupError(f"the index holds the word {word!r}, the word vectors do not")
        row_map[r] = v
    return row_map


class RefinedIndex:
    """A WordIndex whose results are re-ranked against `vectors` (DeviceWordVectors with a key index, e.g.
    read_word2vec_device(...).sorted()): the query surface of WordIndex, each call taking `candidates` index results
    per query (the constructor's value unless overridden) and keeping the k nearest by exact distance.  For a cosine
    index the vectors must be the normalised ones (read_word2vec_device(..., normalize=True))."""

    def __init__(self, word_index, vectors, candidates):
        self.word_index, self.vectors, self.candidates = word_index, vectors, int(candidates)
        if self.candidates < 1:
            raise ValueError("candidates must be at least 1")
        row_map = word_row_map(word_index, vectors)
        self._map, self._work = _DeviceArray(), [_DeviceArray() for _ in range(5)]
        self._map.upload(row_map)

    # ---- what Tests.recall_of and the commands read from an index
    @property
    def words(self):
        return self.word_index.words

    @property
    def size(self):
        return self.word_index.size

    @property
    def dimension(self):
        return self.word_index.dimension

    @property
    def metric(self):
        return self.word_index.metric

    def row_of(self, word):
        return self.word_index.row_of(word)

    def lookup(self, word):
        return self.word_index.lookup(word)

    # ---- the refine stage
    def _candidates(self, k, candidates):
        c = self.candidates if candidates is None else int(candidates)
        if c < 1:
            raise ValueError("candidates must be at least 1")
        return max(c, k)

    def _refine(self, k, prepared, cand):
        """One batch: prepared [B][d] = q', cand [B][c_eff] index rows (-1 = none) -> (rows, distances, counts)."""
        b, c = cand.shape
        rows, dist = np.full((b, k), -1, np.int32), np.zeros((b, k), np.float32)
        counts = np.zeros(b, np.int32)
        if b == 0:
            return rows, dist, counts
        dq, dc, doi, dod, doc = self._work
        dq.upload(N.f32(prepared))
        dc.upload(N.i32(cand))
        doi.ensure(rows.nbytes), dod.ensure(dist.nbytes), doc.ensure(counts.nbytes)
        N.check(N.lib().gulon_refine_topk_dev(self.vectors.matrix._h, dq.ptr, b, dc.ptr, c, self._map.ptr,
                                              self.word_index.size, k, doi.ptr, dod.ptr, doc.ptr, None))
        doi.download(rows), dod.download(dist), doc.download(counts)
        if (counts < 0).any():                       # the map is built from the vectors' own key index
            raise ValueError("requirement failed: a candidate row has no row in the word vectors")
        return rows, dist, counts

    def _prepare(self, q):
        index = self.word_index.index
        if index.metric == "cosine" and len(q):
            from .index import normalize
            return np.stack([normalize(r) for r in q])
        return q

    def batch_query_raw(self, k, vectors, candidates=None):
        """As WordIndex.batch_query_raw: (rows [B][k] with -1 after a query's last entry, distances [B][k], counts [B],
        flags [B]).  The flags are those of the candidate query: a tie flag without GULON_FLAG_EXACT_REPLAY means the
        candidates' order among equal approximate distances is (distance, row id), not the reference heap's."""
        from .word_index import BATCH
        c = self._candidates(k, candidates)
        q = np.ascontiguousarray(vectors, np.float32).reshape(-1, self.dimension)
        cand, _, _, flags = self.word_index.batch_query_raw(c, q)
        rows, dist = np.full((len(q), k), -1, np.int32), np.zeros((len(q), k), np.float32)
        counts = np.zeros(len(q), np.int32)
        for s in range(0, len(q), BATCH):
            e = s + BATCH
            rows[s:e], dist[s:e], counts[s:e] = self._refine(k, self._prepare(q[s:e]), cand[s:e])
        return rows, dist, counts, flags

    def _results(self, rows, dist, counts, flags) -> List[WordResult]:
        words = self.word_index.words
        return [WordResult([words[i] for i in rows[j, :counts[j]].tolist()], dist[j, :counts[j]].copy(),
                           rows[j, :counts[j]].copy(), int(flags[j])) for j in range(len(counts))]

    def batch_query(self, k, vectors, candidates=None) -> List[WordResult]:
        return self._results(*self.batch_query_raw(k, vectors, candidates))

    def query(self, k, vector, candidates=None) -> WordResult:
        return self.batch_query(k, np.asarray(vector, np.float32).reshape(1, -1), candidates)[0]

    def batch_query_by_words(self, k, words, candidates=None) -> List[Optional[WordResult]]:
        """Index.queryByWord for every word (None for a word the index lacks): the query is the index's DECODED vector
        of the word, the candidates are what the index answers to it, and they are re-ranked by their exact distance
        from that decoded vector (normalised for a cosine index) to the original vectors."""
        from .word_index import BATCH
        c = self._candidates(k, candidates)
        wi = self.word_index
        index, cosine = wi.index, wi.index.metric == "cosine"
        words = list(words)
        ids = [wi.row_of(w) for w in words]
        present = [i for i, r in enumerate(ids) if r is not None]
        out: List[Optional[WordResult]] = [None] * len(words)
        for s in range(0, len(present), BATCH):
            part = present[s:s + BATCH]
            r = np.asarray([ids[i] for i in part], np.int32)
            if wi._grouped:
                oi, _, oc = index.batch_query_rows_raw(c, r)
                flags = np.zeros(len(r), np.int32)
                prepared = np.zeros((len(r), self.dimension), np.float32)
                N.check(N.lib().gulon_grouped_index_lookup_rows(index._h, r, len(r), int(cosine), prepared.reshape(-1)))
            else:
                oi, _, oc, flags = index.vector_index.batch_query_rows_raw(c, r, normalize=cosine)
                prepared = index.vector_index.decode_rows(r, normalize=cosine)
            cand = np.where(np.arange(c)[None, :] < oc[:, None], oi, -1).astype(np.int32)
            for i, res in zip(part, self._results(*self._refine(k, prepared, cand), flags)):
                out[i] = res
        return out

    def query_by_word(self, k, word, candidates=None) -> Optional[WordResult]:
        return self.batch_query_by_words(k, [word], candidates)[0]

    def batch_query_expressions(self, k, expressions, candidates=None) -> List[Optional[WordResult]]:
        """Expression queries (expressions.py), refined: the index answers every expression with `candidates` entries,
        its operands already dropped; they are re-ranked by their exact distance from the composed vector -- as the
        index prepares it, normalised for a cosine index -- to the original vectors, and the k nearest kept.  None for
        an expression that names a word the index lacks."""
        from .word_index import BATCH
        c = self._candidates(k, candidates)
        wi = self.word_index
        resolved = wi.resolve_expressions(expressions)
        present = [i for i, e in enumerate(resolved) if e is not None]
        out: List[Optional[WordResult]] = [None] * len(resolved)
        for s in range(0, len(present), BATCH):
            part = present[s:s + BATCH]
            exprs = [resolved[i] for i in part]
            oi, _, oc, flags = wi.index.batch_query_expressions_raw(c, exprs)
            prepared = wi.index.compose_rows(exprs)
            cand = np.where(np.arange(c)[None, :] < oc[:, None], oi, -1).astype(np.int32)
            for i, res in zip(part, self._results(*self._refine(k, prepared, cand), flags)):
                out[i] = res
        return out

    def query_expression(self, k, expression, candidates=None) -> Optional[WordResult]:
        return self.batch_query_expressions(k, [expression], candidates)[0]

    def close(self):
        """Frees the map and the workspace; the index and the vectors stay the caller's."""
        for a in [self._map] + self._work:
            a.free()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
