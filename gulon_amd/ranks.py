"""Rank queries and rank-based dictionary evaluation (csrc/rank.hip).

A rank query is the counting twin of the offset query (csls.py).  Candidates, keys and order are the
offset query's: t = d + offsets[row] in one binary32 addition, a row is a candidate if and only if t is finite and it is
not the query's excluded row, the order is (t ascending, row id ascending).  Every query brings a gold list of row ids;
the answer is the best gold row -- the gold row that is a candidate and comes first -- its t, the number of candidates
strictly ahead of it (the 0-based position it has in the offset query's answer at any depth beyond it) and the number of
candidates.  No list is kept, so there is no depth limit: a dictionary can be scored by mean reciprocal rank and by
precision at any depth, and a gold translation far down the order still counts.

  rank_query_reference        the numpy restatement over a distance matrix, as csls.offset_query_reference is
  rank_query_raw              the ctypes call behind every batch_query_rank_raw
  RankReport                  mrr, median and mean rank, hits at any depths
  evaluate_dictionary_ranks   csls.evaluate_dictionary by ranks: "nn", "csls" or "isf"
"""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import native as N
from .word_index import BATCH


def gold_lists(gold, b) -> Tuple[np.ndarray, np.ndarray]:
    """b gold lists (each an iterable of row ids, possibly empty) in CSR form -> (offsets [b + 1] int32, rows int32)."""
    lists = [np.asarray(list(g), np.int64).reshape(-1) for g in gold]
    if len(lists) != b:
        raise ValueError(f"requirement failed: {len(lists)} gold lists for {b} queries")
    offsets = np.zeros(b + 1, np.int64)
    np.cumsum([len(g) for g in lists], out=offsets[1:])
    rows = np.concatenate(lists) if lists else np.zeros(0, np.int64)
    if offsets[-1] >= 2 ** 31 or (rows.size and (rows.min() < -2 ** 31 or rows.max() >= 2 ** 31)):
        raise ValueError("requirement failed: gold lists beyond int32")
    return offsets.astype(np.int32), rows.astype(np.int32)


# ---- reference (numpy) -------------------------------------------------------------------------------------------------------

def rank_query_reference(dist_rows, offsets, gold, exclude=None, rows=None):
    """What the rank queries compute, in numpy, with csls.offset_query_reference's conventions.  dist_rows [b][n]
    float32: the distance of every query to n rows; offsets [n] float32, one per COLUMN (None: +0 for every column);
    gold: per query an iterable of row ids; rows [n] the row id of every column (None: the column number); exclude [b]
    one row id per query or -1 (None: none).  t = dist + offset in float32; the candidates are the columns with a finite
    t whose row is not the query's excluded one, ordered by (t ascending, row id ascending); a gold row that is no
    column is no candidate.
    -> (rank [b] int32: the candidates strictly ahead of the best gold row, -1 without one; row [b] int32: that row,
    -1; key [b] float32: its t, +inf; total [b] int32: the candidates)."""
    dist = np.ascontiguousarray(dist_rows, np.float32)
    if dist.ndim != 2:
        raise ValueError("requirement failed: dist_rows is [b][n]")
    b, n = dist.shape
    off = np.zeros(n, np.float32) if offsets is None else np.ascontiguousarray(offsets, np.float32).reshape(-1)
    ids = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, np.int64).reshape(-1)
    if len(off) != n or len(ids) != n:
        raise ValueError("requirement failed: one offset and one row id per column of dist_rows")
    ex = np.full(b, -1, np.int64) if exclude is None else np.asarray(exclude, np.int64).reshape(-1)
    if len(ex) != b:
        raise ValueError("requirement failed: one excluded row per query")
    goff, grows = gold_lists(gold, b)
    rank, row = np.full(b, -1, np.int32), np.full(b, -1, np.int32)
    key, total = np.full(b, np.inf, np.float32), np.zeros(b, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (dist + off[None, :]).astype(np.float32)
    for q in range(b):
        cand = np.isfinite(t[q]) & (ids != ex[q])
        total[q] = cand.sum()
        mine = np.flatnonzero(cand & np.isin(ids, grows[goff[q]:goff[q + 1]]))
        if len(mine):
            best = mine[np.lexsort((ids[mine], t[q, mine]))[0]]
            row[q], key[q] = ids[best], t[q, best]
            rank[q] = (cand & ((t[q] < t[q, best]) | ((t[q] == t[q, best]) & (ids < ids[best])))).sum()
    return rank, row, key, total


# ---- the call ------------------------------------------------------------------------------------------------------------------

def host_offsets(offsets, rows=None):
    """`offsets` as the rank entry points read them -- they take host pointers: a csls.DeviceOffsets is downloaded (once,
    by whoever asks in batches), the length is checked against `rows` where given, None stays None (+0 for every
    row)."""
    from .csls import DeviceOffsets
    if offsets is None:
        return None
    if isinstance(offsets, DeviceOffsets):
        if rows is not None and offsets.rows != rows:
            raise ValueError(f"requirement failed: {offsets.rows} offsets for {rows} rows")
        return offsets.numpy()
    off = N.f32(offsets).reshape(-1)
    if rows is not None and len(off) != rows:
        raise ValueError(f"requirement failed: {len(off)} offsets for {rows} rows")
    return off


def rank_query_raw(fn, handle, span, dimension, rows, q, gold, offsets=None, exclude=None):
    """gulon_*_query_rank behind the index classes.  fn: the entry point; span: the arguments between b and row_offsets
    (the index: from, until); rows: the length `offsets` must have; q [b][dimension] float32 as the handle takes them;
    gold: per query an iterable of row ids as the handle returns them; offsets: None, an array or a DeviceOffsets.
    -> (rank [b] int32, row [b] int32, key [b] float32, total [b] int32)."""
    q = N.f32(q).reshape(-1, dimension)
    b = len(q)
    ex = None if exclude is None else N.i32(exclude).reshape(-1)
    if ex is not None and len(ex) != b:
        raise ValueError(f"requirement failed: {len(ex)} excluded rows for {b} queries")
    goff, grows = gold_lists(gold, b)
    off = host_offsets(offsets, rows)
    rank, row = np.full(max(b, 1), -1, np.int32), np.full(max(b, 1), -1, np.int32)
    key, total = np.full(max(b, 1), np.inf, np.float32), np.zeros(max(b, 1), np.int32)
    one_f, one_i = np.zeros(1, np.float32), np.zeros(1, np.int32)
    N.check(fn(handle, q.reshape(-1) if q.size else one_f, b, *span,
               None if off is None or not len(off) else off.ctypes.data,
               None if ex is None or not b else ex.ctypes.data, goff, grows if len(grows) else one_i,
               rank, row, key, total.ctypes.data))
    return rank[:b], row[:b], key[:b], total[:b]


def batched_rank_query(index, dimension, vectors, gold, offsets, exclude):
    """index.batch_query_rank_raw in batches of up to BATCH queries, as the word indexes ask it; a DeviceOffsets is
    downloaded once."""
    q = np.ascontiguousarray(vectors, np.float32).reshape(-1, dimension)
    gold = [list(g) for g in gold]
    if len(gold) != len(q):
        raise ValueError(f"requirement failed: {len(gold)} gold lists for {len(q)} queries")
    ex = None if exclude is None else N.i32(exclude).reshape(-1)
    if ex is not None and len(ex) != len(q):
        raise ValueError(f"requirement failed: {len(ex)} excluded rows for {len(q)} queries")
    off = host_offsets(offsets)
    rank, row = np.full(len(q), -1, np.int32), np.full(len(q), -1, np.int32)
    key, total = np.full(len(q), np.inf, np.float32), np.zeros(len(q), np.int32)
    for s in range(0, len(q), BATCH):
        e = s + BATCH
        rank[s:e], row[s:e], key[s:e], total[s:e] = index.batch_query_rank_raw(
            q[s:e], gold[s:e], off, None if ex is None else ex[s:e])
    return rank, row, key, total


# ---- dictionaries ------------------------------------------------------------------------------------------------------------

@dataclass
class RankReport:
    """Dictionary induction scored by ranks: `asked` source words (each with at least one gold translation both sides
    have), `skipped` dictionary PAIRS with a word absent on either side, `ranks` [asked] the 0-based rank of every
    word's best gold translation, -1 for the `unranked` ones (no gold translation is a candidate)."""
    ks: Tuple[int, ...]
    method: str = "nn"
    asked: int = 0
    skipped: int = 0
    ranks: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    precision_report: Optional[object] = None      # translate --ranks: the precision line printed before this one

    @property
    def ranked(self) -> np.ndarray:
        r = np.asarray(self.ranks, np.int64)
        return r[r >= 0]

    @property
    def unranked(self) -> int:
        return int(self.asked - len(self.ranked))

    @property
    def mrr(self) -> float:
        """The mean of 1 / (rank + 1) over the asked words; an unranked word adds 0."""
        return float((1.0 / (self.ranked + 1.0)).sum() / self.asked) if self.asked else 0.0

    @property
    def median_rank(self) -> float:
        """The median 1-based rank over the ranked words (0 without one)."""
        return float(np.median(self.ranked + 1)) if len(self.ranked) else 0.0

    @property
    def mean_rank(self) -> float:
        """The mean 1-based rank over the ranked words (0 without one)."""
        return float((self.ranked + 1).mean()) if len(self.ranked) else 0.0

    def hits(self, k) -> int:
        """The words whose best gold translation is among the first k candidates; any k >= 1."""
        return int((self.ranked < int(k)).sum())

    def precision(self, k) -> float:
        return self.hits(k) / self.asked if self.asked else 0.0

    def line(self) -> str:
        scores = " ".join(f"@{k} {self.precision(k):.4f}" for k in self.ks)
        return (f"{self.method} ranks: mrr {self.mrr:.4f} median {self.median_rank:g} mean {self.mean_rank:.2f} {scores} "
                f"(n = {self.asked}, unranked {self.unranked}, skipped {self.skipped})")

    def lines(self) -> List[str]:
        first = [] if self.precision_report is None else self.precision_report.lines()
        return first + [self.line()]


def evaluate_dictionary_ranks(target, source, pairs: Sequence[Tuple[str, str]], ks=(1, 5, 10), method="nn",
                              neighbours=10, beta=30.0, sources=None) -> RankReport:
    """csls.evaluate_dictionary by rank queries: per source word the rank of its best gold translation among ALL the
    target's words, so the depths `ks` are not bound by the 63 entries of an offset query's list, a translation far down
    still counts (mrr, median and mean rank), and no list is selected.  target: a WordIndex over byte codes or an
    ExactWordIndex; source: an ExactWordIndex over the source vectors; pairs: csls.read_dictionary.

    method "csls": the order is the offset query's with csls_offsets(target, source, neighbours), so hits(k) equals
    evaluate_dictionary's at every k <= 63; method "isf": the same with isf_offsets(target, source, beta, sources).
    method "nn": the order is (distance ascending, row ascending) with no
    offsets -- total, but NOT the tie order of the ordinary query's heap, so among equal distances a position can differ
    from batch_query's.  The offsets are downloaded once for the whole evaluation.  NotImplementedError: a grouped, a
    rotated or a restricted target; ValueError as evaluate_dictionary."""
    from .analogies import _check_ks
    from .csls import _check_pair, _vector_side, method_offsets, resolve_dictionary
    ks = _check_ks(ks)
    _check_pair(target, source, method)
    if _vector_side(target)[0] == "grouped":
        raise NotImplementedError("rank queries are not supported by a grouped index")
    rows, gold, skipped = resolve_dictionary(target, source, list(pairs))
    report = RankReport(ks, method, len(rows), skipped, np.full(len(rows), -1, np.int64))
    if not rows:
        return report
    offsets = None
    device = method_offsets(target, source, method, neighbours, beta, sources)
    if device is not None:
        try:
            offsets = device.numpy()
        finally:
            device.free()
    rows = N.i32(rows).reshape(-1)
    for s in range(0, len(rows), BATCH):
        vectors = source.index.lookup_rows(rows[s:s + BATCH])
        report.ranks[s:s + BATCH] = target.batch_query_rank_raw(vectors, [sorted(g) for g in gold[s:s + BATCH]], offsets)[0]
    return report
