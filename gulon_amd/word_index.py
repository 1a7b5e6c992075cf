"""An index with its words: Index.lookup / queryByWord / query (Index.scala:25-45) over a saved index file.

`WordIndex.load` reads a protobuf.Index (index_file.load_index) -- the words stay on the host, the vector side is a
device SortedIndex or GroupedIndex.  Word -> row goes through KeyIndex.Sorted / KeyIndex.Grouped (word_vectors.py,
KeyIndex.scala:15-61); the row is looked up and queried on the device (decode.hip), so `query_by_word` queries with
the index's DECODED vector, as the reference does."""
import os
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from .word_vectors import KeyIndexGrouped, KeyIndexSorted

BATCH = 1024          # rows per device batch of batch_query_by_words / batch_query


@dataclass
class WordResult:
    """Index.Result (Index.scala:56-74): neighbour words and distances, nearest first; rows = their row ids."""
    words: List[str]
    distances: np.ndarray
    rows: np.ndarray
    flags: int = 0

    def __len__(self):
        return len(self.words)

    def __iter__(self):
        return iter(zip(self.words, self.distances.tolist()))


class WordIndex:
    def __init__(self, words, index):
        from .grouped import GroupedIndex
        self.words, self.index = list(words), index
        if len(self.words) != index.size:
            raise ValueError(f"{len(self.words)} words for an index of {index.size} rows")
        self._grouped = isinstance(index, GroupedIndex)
        self.key_index = KeyIndexGrouped(self.words, index.offsets) if self._grouped else KeyIndexSorted(self.words)

    @classmethod
    def load(cls, source):
        """source: the bytes of a protobuf.Index, or a path to a file holding them (Index.read, Index.scala:147-149)."""
        from .index_file import load_index
        if isinstance(source, (bytes, bytearray, memoryview)):
            buf = bytes(source)
        else:
            with open(os.fspath(source), "rb") as fh:
                buf = fh.read()
        words, index = load_index(buf)
        return cls(words, index)

    @property
    def dimension(self):
        return self.index.dimension

    @property
    def size(self):
        return len(self.words)

    @property
    def metric(self):
        return self.index.metric

    def refined(self, vectors, candidates):
        """This index with its results re-ranked against the original `vectors` (refine.RefinedIndex): `candidates`
        index results per query, the k nearest of them by exact distance."""
        from .refine import RefinedIndex
        return RefinedIndex(self, vectors, candidates)

    def fine_refined(self, fine, candidates):
        """This index with its results re-ranked against its fine index `fine` (fine.FineRefinedIndex; a WordIndex from
        fine.build_fine_index or the build-fine command): `candidates` index results per query, the k nearest of them by
        their distance to the two-level reconstruction.  No original vectors are needed."""
        from .fine import FineRefinedIndex
        return FineRefinedIndex(self, fine, candidates)

    def exact(self, vectors):
        """The exact index over this index's words (exact.ExactWordIndex): brute-force neighbours among the original
        `vectors` (DeviceWordVectors with a key index; the normalised reading for a cosine index), matched to the
        index's words as `refined` matches them and gathered once on the device in this index's row order -- its row ids
        are this index's row ids, sorted or grouped.  A word the vectors lack: LookupError."""
        from .exact import exact_word_index
        return exact_word_index(self, vectors)

    def inspect(self, vectors=None, worst=10):
        """The diagnostics of this index (inspect.IndexReport): its shape and how its code books are used; with
        `vectors` (DeviceWordVectors with a key index; the normalised reading for a cosine index), matched to the
        index's words as `refined` matches them, also how far its rows lie from their originals and the `worst` words
        with the largest error."""
        from .inspect import inspect_word_index
        return inspect_word_index(self, vectors, worst)

    def restrict(self, words):
        """This index with its neighbours drawn from `words` only (PQIndex.select: a view gathered on the device, built
        once for any number of queries).  Words the index lacks are ignored -- their number is `.ignored` -- and
        duplicates count once.  Results carry this index's words and row ids; query_by_word looks its word up in this
        index, so the query word need not be among `words`."""
        if self._grouped:
            raise NotImplementedError("restrict is not supported by the grouped index")
        return RestrictedWordIndex(self, words)

    def update(self, add=None, remove=None):
        """A new WordIndex with words removed, replaced and added, built on the device without retraining (update.py,
        csrc/update.hip); this index is untouched.  remove: an iterable of words, applied first -- words the index lacks
        are ignored.  add: DeviceWordVectors as read (for a cosine index the normalised reading, which is what
        build-index feeds); a word the index still has is replaced, any other added, each encoded by this index's own
        quantizer in the order `add` gives them.  A kept word keeps its code.  The result's words are in String.compareTo
        order; it carries the counters .added, .replaced, .removed, .ignored.  A word twice in `add`: ValueError."""
        from .update import plan_update
        if self._grouped:
            raise NotImplementedError("update is not supported by the grouped index")
        add_words = list(add.words) if add is not None else []
        if add_words and add.dimension != self.dimension:
            raise ValueError(f"requirement failed: the added vectors have {add.dimension} dimensions, the index "
                             f"{self.dimension}")
        plan = plan_update(self.words, add_words, remove if remove is not None else ())
        out = WordIndex(plan.words, self.index.updated(plan.take, add.matrix if add_words else None))
        out.added, out.replaced, out.removed, out.ignored = plan.added, plan.replaced, plan.removed, plan.ignored
        return out

    def row_of(self, word) -> Optional[int]:
        return self.key_index.lookup(word)

    def lookup(self, word) -> Optional[np.ndarray]:
        """Index.lookup (Index.scala:38): the index's approximation of the word's vector, None if it is absent."""
        row = self.row_of(word)
        return None if row is None else self.index.lookup_rows([row])[0]

    def distances(self, pairs):
        """Per (word1, word2) the distance between lookup(word1) and lookup(word2) -- MathUtils.distanceSq, on the
        device (csrc/pairs.hip) -- None where a word is absent."""
        from .similarity import word_distances
        return word_distances(self, pairs)

    def _result(self, r) -> WordResult:
        return WordResult([self.words[i] for i in r.rows.tolist()], r.distances, r.rows, r.flags)

    def batch_query_by_words(self, k, words) -> List[Optional[WordResult]]:
        """Index.queryByWord (Index.scala:43-45) for every word, in order: None for a word the index lacks.  The words
        present are queried on the device, up to BATCH per batch."""
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
        """Expressions over words (Expression objects, sequences of Term / (word, weight), or text for
        parse_expression) -> the same over row ids, None where a word is absent."""
        from .expressions import resolve_expressions
        return resolve_expressions(self.row_of, expressions)

    def batch_query_expressions(self, k, expressions) -> List[Optional[WordResult]]:
        """Per expression over words (`king - man + woman`) the k nearest words of its composed vector that are none of
        its operands, in input order; None for an expression that names a word the index lacks.  Composed, queried and
        filtered on the device, up to BATCH expressions per batch."""
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
        """Per expression over words the k words with the largest 3CosMul score (Levy & Goldberg's multiplicative
        objective; expressions.cosmul_reference) that are none of its operands, in input order; None for
        an expression that names a word the index lacks.  `distances` of a result holds the SCORES, in descending
        order.  Scored on the device, up to BATCH expressions per batch.  ValueError on an l2 index;
        NotImplementedError for a grouped index (and, from the library, for codes wider than a byte)."""
        if self.metric != "cosine":
            raise ValueError("requirement failed: cosmul queries need a cosine index")
        if self._grouped:
            raise NotImplementedError("cosmul queries are not supported by the grouped index")
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
        """SortedIndex.batch_query_offset_raw (csls.py), up to BATCH queries per device batch: (rows
        [b][k] with -1 after a query's last entry, keys [b][k] with +inf there, counts [b]).  A grouped index answers
        from the groups its strategy searches (GroupedIndex.batch_query_offset_raw).  NotImplementedError,
        from the library, for codes wider than a byte."""
        from .csls import batched_offset_query
        return batched_offset_query(self.index, self.dimension, k, vectors, offsets, exclude)

    def batch_query_offset(self, k, vectors, offsets, exclude=None) -> List[WordResult]:
        """Per query vector the k words with the smallest distance + offsets[row] among the rows whose sum is finite
        and that are not exclude[q]; `distances` of a result holds those keys.  offsets: one float32 per row, an array
        or what csls.csls_offsets returned."""
        from .csls import as_results
        return [self._result(r) for r in as_results(*self.batch_query_offset_raw(k, vectors, offsets, exclude))]

    def batch_query_rank_raw(self, vectors, gold, offsets=None, exclude=None):
        """SortedIndex.batch_query_rank_raw (ranks.py), up to BATCH queries per device batch: (rank [b],
        row [b], key [b], total [b]) of every query's best gold row.  NotImplementedError for a grouped index, and from
        the library for codes wider than a byte."""
        if self._grouped:
            raise NotImplementedError("rank queries are not supported by a grouped index")
        from .ranks import batched_rank_query
        return batched_rank_query(self.index, self.dimension, vectors, gold, offsets, exclude)

    def batch_query(self, k, vectors) -> List[WordResult]:
        """Index.batchQuery (Index.scala:25-32) with the results' words."""
        q = np.ascontiguousarray(vectors, np.float32).reshape(-1, self.dimension)
        out = []
        for s in range(0, len(q), BATCH):
            out.extend(self._result(r) for r in self.index.batch_query(k, q[s:s + BATCH]))
        return out

    def batch_query_raw(self, k, vectors):
        """batch_query as arrays, for callers that take thousands of neighbours per query and no words (Tests.recallOf):
        (rows [B][k] int32 with -1 after a query's last entry, distances [B][k], counts [B], flags [B]; a grouped
        index sets no flags)."""
        q = np.ascontiguousarray(vectors, np.float32).reshape(-1, self.dimension)
        rows, dist = np.full((len(q), k), -1, np.int32), np.zeros((len(q), k), np.float32)
        counts, flags = np.zeros(len(q), np.int32), np.zeros(len(q), np.int32)
        for s in range(0, len(q), BATCH):
            part = q[s:s + BATCH]
            if self._grouped:
                oi, od, oc = self.index.batch_query_raw(k, part)
            else:
                oi, od, oc, flags[s:s + BATCH] = self.index.vector_index.batch_query_raw(k, self.index._prepare(part))
            have = np.arange(k)[None, :] < oc[:, None]
            rows[s:s + BATCH], dist[s:s + BATCH], counts[s:s + BATCH] = np.where(have, oi, -1), np.where(have, od, 0), oc
        return rows, dist, counts, flags

    def query(self, k, vector) -> WordResult:
        return self.batch_query(k, np.asarray(vector, np.float32).reshape(1, -1))[0]

    def close(self):
        (self.index if self._grouped else self.index.vector_index).close()


class RestrictedWordIndex(WordIndex):
    """WordIndex.restrict: `parent`'s words and key index over a SortedIndex on the view of the listed words' rows."""

    def __init__(self, parent, words):
        rows = [parent.row_of(w) for w in words]
        self.ignored = sum(r is None for r in rows)
        self.parent = parent
        self.words, self.key_index, self._grouped = parent.words, parent.key_index, False
        self.index = parent.index.select(rows=np.unique(np.asarray([r for r in rows if r is not None], np.int64)))

    @property
    def restricted_size(self):
        return self.index.size

    def lookup(self, word):
        return self.parent.lookup(word)

    def distances(self, pairs):
        return self.parent.distances(pairs)

    def batch_query_by_words(self, k, words) -> List[Optional[WordResult]]:
        """queryByWord with the word's vector decoded from the PARENT and the neighbours taken from the restriction."""
        words = list(words)
        rows = [self.row_of(w) for w in words]
        present = [i for i, r in enumerate(rows) if r is not None]
        out: List[Optional[WordResult]] = [None] * len(words)
        cosine = self.metric == "cosine"
        for s in range(0, len(present), BATCH):
            part = present[s:s + BATCH]
            vectors = self.parent.index.vector_index.decode_rows(np.asarray([rows[i] for i in part], np.int32), cosine)
            for i, r in zip(part, self.index.vector_index.batch_query(k, vectors)):
                out[i] = self._result(r)
        return out

    def restrict(self, words):
        """A restriction of a restriction: the listed words that are also in this one."""
        inside = set(self.index.vector_index.rows.tolist())
        rows = [self.row_of(w) for w in words]
        out = self.parent.restrict([w for w, r in zip(words, rows) if r is not None and r in inside])
        out.ignored = sum(r is None or r not in inside for r in rows)
        return out

    def update(self, add=None, remove=None):
        raise NotImplementedError("update is not supported by a restricted index")

    def refined(self, vectors, candidates):
        raise NotImplementedError("refined is not supported by a restricted index")

    def fine_refined(self, fine, candidates):
        raise NotImplementedError("fine_refined is not supported by a restricted index")

    def exact(self, vectors):
        raise NotImplementedError("exact is not supported by a restricted index")

    def inspect(self, vectors=None, worst=10):
        raise NotImplementedError("inspect is not supported by a restricted index")

    def resolve_expressions(self, expressions):
        raise NotImplementedError("expressions are not supported by a restricted index")

    def batch_query_expressions(self, k, expressions):
        raise NotImplementedError("expressions are not supported by a restricted index")

    def batch_query_cosmul(self, k, expressions):
        raise NotImplementedError("cosmul queries are not supported by a restricted index")

    def batch_query_offset_raw(self, k, vectors, offsets, exclude=None):
        raise NotImplementedError("offset queries are not supported by a restricted index")

    def batch_query_rank_raw(self, vectors, gold, offsets=None, exclude=None):
        raise NotImplementedError("rank queries are not supported by a restricted index")

    def close(self):
        self.index.vector_index.close()
