"""The exact index: brute-force neighbours over the original vectors, with the query surface of the other indexes
(csrc/exact.hip).

ExactIndex answers what `exact_nearest_neighbours` answers -- Index.exactNearestNeighbours (Index.scala:209-229) with
MathUtils.distanceSq, entries ascending in (distance, row id), tie flags -- from a handle that keeps its scratch, takes
device pointers as well as arrays, and above 63 neighbours reads the rows once instead of once per 64 entries.
ExactWordIndex puts words on it; WordIndex.exact(vectors) builds one over an index's words in the index's row order, so
its answers compare entry by entry with the index's own."""
import ctypes as C
from typing import List, Optional

import numpy as np

from . import native as N
from .index import Result, normalize
from .matrix import as_device
from .word_index import BATCH, WordResult

KNOBS = ("GULON_EXACT_SAMPLE", "GULON_EXACT_QUEUE_CAP")
STATS = ("one_pass", "fallback", "nonfinite", "sample", "capacity", "max_fill")


def normalize_rows(q):
    """index.normalize of every row of q [b][d] float32, the bits of the row-by-row call: the float32 sum of squares
    advances one dimension at a time for all the rows at once, the square root is taken in float64."""
    q = N.f32(q)
    s = np.zeros(len(q), np.float32)
    with np.errstate(all="ignore"):
        for e in range(q.shape[1]):
            s = s + q[:, e] * q[:, e]
        dist = np.sqrt(s.astype(np.float64)).astype(np.float32)
        return (q / dist[:, None]).astype(np.float32)


class ExactIndex:
    """Exact neighbours of rows [frm, until) of `matrix` (a DeviceMatrix, a Matrix or an array; the index does not own a
    DeviceMatrix it is given, which must outlive it).  metric "cosine": the queries are normalised as
    SortedIndex._prepare normalises them and the matrix is expected to hold normalised vectors already -- the
    normalised reading that build-index feeds."""

    def __init__(self, matrix, metric="l2", frm=0, until=None):
        if metric not in ("l2", "cosine"):
            raise ValueError(f"unknown metric {metric!r}")
        self.matrix, self.metric = as_device(matrix), metric
        self.frm, self.until = int(frm), self.matrix.rows if until is None else int(until)
        self._h = C.c_void_p()
        N.check(N.lib().gulon_exact_index_create(self.matrix._h, self.frm, self.until, C.byref(self._h)))

    @property
    def dimension(self):
        return self.matrix.cols

    @property
    def size(self):
        return self.until - self.frm

    def _prepare(self, q):
        q = N.f32(q).reshape(-1, self.dimension)
        if self.metric == "cosine" and len(q):
            q = np.stack([normalize(r) for r in q])
        return q

    @staticmethod
    def _outputs(b, k):
        return (np.zeros((b, max(k, 1)), np.int32), np.zeros((b, max(k, 1)), np.float32), np.zeros(max(b, 1), np.int32),
                np.zeros(max(b, 1), np.int32))

    def batch_query_raw(self, k, vectors):
        """(rows [B][k] with -1 after a query's last entry, distances [B][k] with +inf there, counts [B], flags [B])."""
        q = self._prepare(vectors)
        b = len(q)
        oi, od, oc, of = self._outputs(b, k)
        N.check(N.lib().gulon_exact_index_batch_query(self._h, q.reshape(-1) if q.size else np.zeros(1, np.float32), b, k,
                                                      oi.reshape(-1), od.reshape(-1), oc, of))
        return oi[:, :k], od[:, :k], oc[:b], of[:b]

    def batch_query_rows_raw(self, k, rows):
        """batch_query_raw with rows of the matrix as the queries, gathered on the device (they are taken as stored: a
        cosine index holds normalised rows)."""
        rows = N.i32(rows).reshape(-1)
        b = len(rows)
        oi, od, oc, of = self._outputs(b, k)
        N.check(N.lib().gulon_exact_index_query_rows(self._h, rows if b else np.zeros(1, np.int32), b, k, oi.reshape(-1),
                                                     od.reshape(-1), oc, of))
        return oi[:, :k], od[:, :k], oc[:b], of[:b]

    @staticmethod
    def _results(oi, od, oc, of):
        return [Result(oi[i, :oc[i]].copy(), od[i, :oc[i]].copy(), int(of[i])) for i in range(len(oc))]

    def batch_query(self, k, vectors) -> List[Result]:
        return self._results(*self.batch_query_raw(k, vectors))

    def query(self, k, vector) -> Result:
        return self.batch_query(k, N.f32(vector).reshape(1, -1))[0]

    def batch_query_rows(self, k, rows) -> List[Result]:
        return self._results(*self.batch_query_rows_raw(k, rows))

    def batch_query_dev(self, k, d_queries, b, d_rows, d_dist, d_counts=None, d_flags=None, stream=None):
        """The device form: every argument but k and b a device address (int), the queries taken as they are."""
        N.check(N.lib().gulon_exact_index_batch_query_dev(self._h, d_queries, b, k, d_rows, d_dist, d_counts, d_flags,
                                                          stream))

    def batch_query_rows_dev(self, k, d_query_rows, b, d_rows, d_dist, d_counts=None, d_flags=None, stream=None):
        N.check(N.lib().gulon_exact_index_query_rows_dev(self._h, d_query_rows, b, k, d_rows, d_dist, d_counts, d_flags,
                                                         stream))

    def lookup_rows(self, rows):
        """The rows themselves: [len(rows)][dimension]."""
        return self.matrix.get_rows(rows)

    def pair_distances(self, rows_a, rows_b):
        """MathUtils.distanceSq between rows rows_a[i] and rows_b[i] of the MATRIX -- the ids the queries return -- for
        every i, on the device (gulon_dataset_pair_distances).  -> [n] float32."""
        from .similarity import pair_distances_raw
        return pair_distances_raw(N.lib().gulon_dataset_pair_distances, self.matrix._h, rows_a, rows_b)

    def pair_distances_dev(self, d_rows_a, d_rows_b, n, d_dist, stream=None):
        """The device form: the rows and the distances device addresses; `stream` is waited for."""
        N.check(N.lib().gulon_dataset_pair_distances_dev(self.matrix._h, d_rows_a, d_rows_b, n, d_dist, stream))

    # ---- expression queries (expressions.py): the terms are rows of the MATRIX
    def compose_rows(self, expressions):
        """The query vector of every expression over row ids as this index prepares it -- terms and sum normalised for a
        cosine index -- composed on the device from the original rows (gulon_dataset_compose_rows).  -> [b][d] float32."""
        from .expressions import to_csr
        off, rows, w = to_csr(expressions)
        b = len(off) - 1
        cosine = int(self.metric == "cosine")
        out = np.zeros((b, self.dimension), np.float32)
        one_i, one_f = np.zeros(1, np.int32), np.zeros(1, np.float32)
        N.check(N.lib().gulon_dataset_compose_rows(self.matrix._h, off, rows if b else one_i, w if b else one_f, b,
                                                   cosine, cosine, out.reshape(-1) if out.size else one_f))
        return out

    def batch_query_terms_raw(self, k, expressions, extra):
        """gulon_exact_index_query_terms as it is: the answer at k + extra with every expression's term rows removed,
        the first k kept.  -> (rows [b][k], distances [b][k], counts [b], flags [b])."""
        from .expressions import to_csr
        off, rows, w = to_csr(expressions)
        b = len(off) - 1
        cosine = int(self.metric == "cosine")
        oi, od, oc, of = self._outputs(b, k)
        one_i, one_f = np.zeros(1, np.int32), np.zeros(1, np.float32)
        N.check(N.lib().gulon_exact_index_query_terms(self._h, off, rows if b else one_i, w if b else one_f, b, k, extra,
                                                      cosine, cosine, oi.reshape(-1), od.reshape(-1), oc, of))
        return oi[:, :k], od[:, :k], oc[:b], of[:b]

    def batch_query_expressions_raw(self, k, expressions):
        """batch_query_terms_raw per partition of the batch by its number E of distinct term rows, extra = E, in input
        order: (rows [b][k] with -1 after a query's last entry, distances [b][k] with +inf there, counts [b], flags [b])."""
        from .expressions import query_partitioned
        return query_partitioned(expressions, lambda part, extra: self.batch_query_terms_raw(k, part, extra),
                                 (((k,), np.int32, -1), ((k,), np.float32, np.inf), ((), np.int32, 0), ((), np.int32, 0)))

    def batch_query_expressions(self, k, expressions) -> List[Result]:
        """Per expression over row ids the k nearest rows of its composed vector that are none of its operands."""
        return self._results(*self.batch_query_expressions_raw(k, expressions))

    def batch_query_cosmul_raw(self, k, expressions):
        """gulon_exact_index_query_cosmul: per expression over rows of the matrix the k rows of [frm, until) with the
        largest 3CosMul score that are none of its term rows (expressions.cosmul_reference); the term
        vectors are normalised for a cosine index.  -> (rows [b][k] with -1 after an expression's last entry, SCORES
        [b][k] in descending order with -inf there, counts [b])."""
        from .expressions import to_csr
        off, rows, w = to_csr(expressions)
        b = len(off) - 1
        oi, od, oc, _ = self._outputs(b, k)
        one_i, one_f = np.zeros(1, np.int32), np.zeros(1, np.float32)
        N.check(N.lib().gulon_exact_index_query_cosmul(self._h, off, rows if b else one_i, w if b else one_f, b, k,
                                                       int(self.metric == "cosine"), oi.reshape(-1), od.reshape(-1), oc))
        return oi[:, :k], od[:, :k], oc[:b]

    def batch_query_cosmul(self, k, expressions) -> List[Result]:
        """batch_query_cosmul_raw as Results: `distances` holds the SCORES, in descending order; flags is 0."""
        oi, od, oc = self.batch_query_cosmul_raw(k, expressions)
        return [Result(oi[i, :oc[i]].copy(), od[i, :oc[i]].copy(), 0) for i in range(len(oc))]

    # ---- offset queries (csls.py): the offsets are indexed by rows of the MATRIX
    def batch_query_offset_raw(self, k, vectors, offsets, exclude=None):
        """gulon_exact_index_query_offset: per query the k rows of [frm, until) with the smallest t = distance +
        offsets[row] among those whose t is finite and that are not exclude[q] (a row of the matrix, or -1), ties by
        row id (csls.offset_query_reference).  The queries are normalised for a cosine index.  offsets: one float32 per
        row of the matrix, an array or the device array csls.csls_offsets returned.  1 <= k <= 63.
        -> (rows [b][k] with -1 after a query's last entry, keys t [b][k] with +inf there, counts [b])."""
        from .csls import offset_query_raw
        L = N.lib()
        return offset_query_raw(L.gulon_exact_index_query_offset, L.gulon_exact_index_query_offset_dev, self._h, (),
                                self.dimension, self.matrix.rows, k, self._prepare(vectors), offsets, exclude)

    def batch_query_offset(self, k, vectors, offsets, exclude=None) -> List[Result]:
        """batch_query_offset_raw as Results: `distances` holds the keys t, ascending; flags is 0."""
        from .csls import as_results
        return as_results(*self.batch_query_offset_raw(k, vectors, offsets, exclude))

    # ---- rank queries (ranks.py): offsets, excluded rows and gold rows are rows of the MATRIX
    def batch_query_rank_raw(self, vectors, gold, offsets=None, exclude=None):
        """gulon_exact_index_query_rank: per query the best row of its gold list (an iterable of rows of the matrix) in
        the order of batch_query_offset_raw -- t = distance + offsets[row] finite, not exclude[q], by (t, row) -- and how
        many candidates come before it (ranks.rank_query_reference).  No k: nothing is listed.  The queries are
        normalised for a cosine index.  offsets: None (+0), an array or a csls.DeviceOffsets (downloaded: the entry
        point takes host pointers).
        -> (rank [b], -1 without a gold candidate; row [b], -1; key t [b], +inf; total [b] candidates)."""
        from .ranks import rank_query_raw
        return rank_query_raw(N.lib().gulon_exact_index_query_rank, self._h, (), self.dimension, self.matrix.rows,
                              self._prepare(vectors), gold, offsets, exclude)

    # ---- log-sum-exp queries (softmax.py): the excluded rows are rows of the MATRIX
    def batch_query_logsumexp(self, vectors, beta, exclude=None):
        """gulon_exact_index_query_logsumexp: per query L = log of the sum of exp(-(beta / 2) * distance) over the rows
        of [frm, until) whose distance is finite and that are not exclude[q] (a row of the matrix, or -1), summed in
        float64 in a fixed order (softmax.logsumexp_reference), and the number of those rows.  The queries are
        normalised for a cosine index.  beta: finite and > 0, taken as a float32.  The last bits of L may differ
        between batches of different sizes.
        -> (L [b] float64, -inf without a term or where every term underflows; terms [b] int32)."""
        from .softmax import _beta
        beta = _beta(beta)
        q = N.f32(vectors).reshape(-1, self.dimension)
        if self.metric == "cosine" and len(q):
            q = normalize_rows(q)
        b = len(q)
        ex = None if exclude is None else N.i32(exclude).reshape(-1)
        if ex is not None and len(ex) != b:
            raise ValueError(f"requirement failed: {len(ex)} excluded rows for {b} queries")
        out, terms = np.full(max(b, 1), -np.inf, np.float64), np.zeros(max(b, 1), np.int32)
        N.check(N.lib().gulon_exact_index_query_logsumexp(
            self._h, q.reshape(-1) if q.size else np.zeros(1, np.float32), b, beta,
            None if ex is None or not b else ex.ctypes.data, out, terms.ctypes.data))
        return out[:b], terms[:b]

    def stats(self):
        """Of the last batch: queries answered in one pass, by the peeled fallback and one at a time as non-finite; the
        sample rows S (0: no sample pass), the queue capacity, the largest number of rows at or below a bound."""
        out = np.zeros(6, np.int64)
        N.check(N.lib().gulon_exact_index_stats(self._h, out))
        return dict(zip(STATS, out.tolist()))

    def tune(self, **knobs):
        """GULON_EXACT_SAMPLE=..., GULON_EXACT_QUEUE_CAP=... on this handle; results never depend on them."""
        for key, value in knobs.items():
            N.check(N.lib().gulon_exact_index_tuning(self._h, key.encode(), int(value)))

    def close(self):
        if self._h is not None and self._h.value:
            N.lib().gulon_exact_index_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ExactWordIndex:
    """Words over an ExactIndex whose row i holds the vector of words[i]: the query surface of WordIndex.  `key_index`
    maps a word to its row (default: a dictionary over `words`)."""

    def __init__(self, words, index, key_index=None):
        self.words, self.index = list(words), index
        if len(self.words) != index.size or index.frm != 0:
            raise ValueError(f"{len(self.words)} words for an exact index of rows [{index.frm}, {index.until})")
        self._rows = None if key_index is not None else {w: i for i, w in enumerate(self.words)}
        self.key_index = key_index

    @property
    def size(self):
        return len(self.words)

    @property
    def dimension(self):
        return self.index.dimension

    @property
    def metric(self):
        return self.index.metric

    def row_of(self, word) -> Optional[int]:
        return self.key_index.lookup(word) if self.key_index is not None else self._rows.get(word)

    def lookup(self, word) -> Optional[np.ndarray]:
        """The word's original vector, None if it is absent."""
        row = self.row_of(word)
        return None if row is None else self.index.lookup_rows([row])[0]

    def distances(self, pairs):
        """Per (word1, word2) the distance between the two words' original vectors, on the device; None where a word is
        absent."""
        from .similarity import word_distances
        return word_distances(self, pairs)

    def _result(self, r) -> WordResult:
        return WordResult([self.words[i] for i in r.rows.tolist()], r.distances, r.rows, r.flags)

    def batch_query(self, k, vectors) -> List[WordResult]:
        q = np.ascontiguousarray(vectors, np.float32).reshape(-1, self.dimension)
        out = []
        for s in range(0, len(q), BATCH):
            out.extend(self._result(r) for r in self.index.batch_query(k, q[s:s + BATCH]))
        return out

    def query(self, k, vector) -> WordResult:
        return self.batch_query(k, np.asarray(vector, np.float32).reshape(1, -1))[0]

    def batch_query_by_words(self, k, words) -> List[Optional[WordResult]]:
        """Index.queryByWord (Index.scala:43-45) with the word's ORIGINAL vector as the query, so the word itself comes
        first at distance 0; None for a word the index lacks."""
        words = list(words)
        rows = [self.row_of(w) for w in words]
        present = [i for i, r in enumerate(rows) if r is not None]
        out: List[Optional[WordResult]] = [None] * len(words)
        for s in range(0, len(present), BATCH):
            part = present[s:s + BATCH]
            results = self.index.batch_query_rows(k, np.asarray([rows[i] for i in part], np.int32))
            for i, r in zip(part, results):
                out[i] = self._result(r)
        return out

    def query_by_word(self, k, word) -> Optional[WordResult]:
        return self.batch_query_by_words(k, [word])[0]

    def resolve_expressions(self, expressions):
        """As WordIndex.resolve_expressions: expressions over words -> the same over row ids, None where a word is
        absent."""
        from .expressions import resolve_expressions
        return resolve_expressions(self.row_of, expressions)

    def batch_query_expressions(self, k, expressions) -> List[Optional[WordResult]]:
        """As WordIndex.batch_query_expressions, over the ORIGINAL vectors of the words: per expression the k nearest
        words of its composed vector that are none of its operands; None where a word is absent."""
        resolved = self.resolve_expressions(expressions)
        present = [i for i, e in enumerate(resolved) if e is not None]
        out: List[Optional[WordResult]] = [None] * len(resolved)
        for s in range(0, len(present), BATCH):
            part = present[s:s + BATCH]
            for i, r in zip(part, self.index.batch_query_expressions(k, [resolved[i] for i in part])):
                out[i] = self._result(r)
        return out

    def query_expression(self, k, expression) -> Optional[WordResult]:
        return self.batch_query_expressions(k, [expression])[0]

    def batch_query_cosmul(self, k, expressions) -> List[Optional[WordResult]]:
        """As WordIndex.batch_query_cosmul, over the ORIGINAL vectors of the words: per expression the k words with the
        largest 3CosMul score that are none of its operands, `distances` holding the SCORES in descending order; None
        where a word is absent.  ValueError on an l2 index."""
        if self.metric != "cosine":
            raise ValueError("requirement failed: cosmul queries need a cosine index")
        resolved = self.resolve_expressions(expressions)
        present = [i for i, e in enumerate(resolved) if e is not None]
        out: List[Optional[WordResult]] = [None] * len(resolved)
        for s in range(0, len(present), BATCH):
            part = present[s:s + BATCH]
            for i, r in zip(part, self.index.batch_query_cosmul(k, [resolved[i] for i in part])):
                out[i] = self._result(r)
        return out

    def query_cosmul(self, k, expression) -> Optional[WordResult]:
        return self.batch_query_cosmul(k, [expression])[0]

    def batch_query_offset_raw(self, k, vectors, offsets, exclude=None):
        """ExactIndex.batch_query_offset_raw, up to BATCH queries per device batch."""
        from .csls import batched_offset_query
        return batched_offset_query(self.index, self.dimension, k, vectors, offsets, exclude)

    def batch_query_offset(self, k, vectors, offsets, exclude=None) -> List[WordResult]:
        """Per query vector the k words with the smallest distance + offsets[row] (csls.py); `distances` of a result
        holds those keys."""
        from .csls import as_results
        return [self._result(r) for r in as_results(*self.batch_query_offset_raw(k, vectors, offsets, exclude))]

    def batch_query_rank_raw(self, vectors, gold, offsets=None, exclude=None):
        """ExactIndex.batch_query_rank_raw, up to BATCH queries per device batch."""
        from .ranks import batched_rank_query
        return batched_rank_query(self.index, self.dimension, vectors, gold, offsets, exclude)

    def batch_query_logsumexp(self, vectors, beta, exclude=None):
        """ExactIndex.batch_query_logsumexp, as it is: one device batch, so that a vector's answer does not depend on
        how a caller's batch would have been cut."""
        return self.index.batch_query_logsumexp(vectors, beta, exclude)

    def close(self):
        """Frees the handle and the gathered matrix this index was built over, when it owns one."""
        self.index.close()
        owned = getattr(self, "_owned_matrix", None)
        if owned is not None:
            owned.close()
            self._owned_matrix = None


def exact_word_index(word_index, vectors):
    """WordIndex.exact: the ExactWordIndex over `word_index`'s words in its row order, the vectors matched by
    refine.word_row_map (LookupError for a word they lack) and gathered once on the device."""
    from .matrix import DeviceMatrix
    from .refine import word_row_map
    row_map = word_row_map(word_index, vectors)[:word_index.size]
    h = C.c_void_p()
    N.check(N.lib().gulon_dataset_gather(vectors.matrix._h, row_map if row_map.size else np.zeros(1, np.int32),
                                         row_map.size, C.byref(h)))
    matrix = DeviceMatrix(h, row_map.size, vectors.matrix.cols)
    out = ExactWordIndex(word_index.words, ExactIndex(matrix, word_index.metric), word_index.key_index)
    out._owned_matrix = matrix
    return out
