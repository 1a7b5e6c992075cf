"""Offset queries and CSLS word translation (csrc/offset.hip).

An offset query ranks the rows of an index by t = d + offsets[row] -- d the distance the index's ordinary query returns,
one binary32 addition -- keeps the rows whose t is finite and that are not the query's excluded row, and returns the first
k by (t ascending, row id ascending).  An offset of +inf masks a row; a finite one is a per-row prior.

CSLS (cross-domain similarity local scaling; Conneau et al., "Word translation without parallel data", 2018) is the use
it was built for.  Nearest-neighbour translation between two aligned embedding files suffers from hubs: a few target
words that are near everything.  CSLS subtracts from the similarity of a candidate y its mean similarity r_S(y) to its
own K nearest SOURCE words.  On unit vectors cos = 1 - d / 2, so

    CSLS(x, y) = 2 cos(x, y) - r_T(x) - r_S(y) = 2 - d(x, y) - r_T(x) - r_S(y)

and for a fixed query x ranking by CSLS descending is ranking by d(x, y) + r_S(y) ascending: an offset query with
offsets = r_S (csls_offsets).  r_T(x) shifts every score of one query alike; translation_scores adds it back for display.

  csls_offsets         r_S for every target row, on the device: the target's rows composed where they live, the source
                       ExactIndex asked for their K nearest, gulon_mean_similarity_dev straight into the offsets array
  isf_offsets          the offsets of the inverted softmax (softmax.py) over the same passes: the composed
                       rows asked of the source's batch_query_logsumexp
  evaluate_dictionary  precision@k of a bilingual dictionary (MUSE's format, read_dictionary), plain ("nn"), "csls" or
                       "isf"
  translate_words      the k translations of a list of source words

The two *_reference functions restate the arithmetic in numpy, as cosmul_reference does for its kernel."""
import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import native as N
from .index import Result
from .word_index import BATCH, WordResult

ROWS_PER_PASS = 4096          # target rows per batch of csls_offsets
METHODS = ("nn", "csls", "isf")
OFFSET_METHODS = ("csls", "isf")  # the methods that rank by an offset query


# ---- references (numpy) ----------------------------------------------------------------------------------------------------

def offset_query_reference(dist_rows, offsets, k, exclude=None, rows=None):
    """What the offset queries compute, in numpy.  dist_rows [b][n] float32: the distance of every query to n rows;
    offsets [n] float32, one per COLUMN; rows [n] the row id of every column (None: the column number); exclude [b] one
    row id per query or -1 (None: none).  t = dist + offset in float32; the candidates are the columns with a finite t
    whose row is not the query's excluded one, ordered by (t ascending, row id ascending).
    -> (rows [b][k] int32 padded with -1, keys [b][k] float32 padded with +inf, counts [b] int32)."""
    dist = np.ascontiguousarray(dist_rows, np.float32)
    if dist.ndim != 2:
        raise ValueError("requirement failed: dist_rows is [b][n]")
    b, n = dist.shape
    off = np.ascontiguousarray(offsets, np.float32).reshape(-1)
    ids = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, np.int64).reshape(-1)
    if len(off) != n or len(ids) != n:
        raise ValueError("requirement failed: one offset and one row id per column of dist_rows")
    ex = np.full(b, -1, np.int64) if exclude is None else np.asarray(exclude, np.int64).reshape(-1)
    if len(ex) != b:
        raise ValueError("requirement failed: one excluded row per query")
    out_i, out_t = np.full((b, k), -1, np.int32), np.full((b, k), np.inf, np.float32)
    counts = np.zeros(b, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (dist + off[None, :]).astype(np.float32)
    for q in range(b):
        cand = np.flatnonzero(np.isfinite(t[q]) & (ids != ex[q]))
        order = cand[np.lexsort((ids[cand], t[q, cand]))][:k]
        counts[q] = len(order)
        out_i[q, :len(order)], out_t[q, :len(order)] = ids[order], t[q, order]
    return out_i, out_t, counts


def mean_similarity_reference(dist_lists, counts, K):
    """gulon_mean_similarity in numpy: dist_lists [b][kin] float32, counts [b] or None.  c = min(counts[q], K) (None:
    min(kin, K)); out[q] = 0 when c == 0, else the float32 running sum of s_j = 1 - 0.5 * d_j, j = 0 .. c - 1, from s_0,
    divided by float32(c).  -> [b] float32."""
    d = np.ascontiguousarray(dist_lists, np.float32)
    if d.ndim != 2 or K < 1:
        raise ValueError("requirement failed: dist_lists is [b][kin] and K >= 1")
    b, kin = d.shape
    out = np.zeros(b, np.float32)
    half, one = np.float32(0.5), np.float32(1)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(b):
            c = min(kin, K) if counts is None else min(max(int(counts[q]), 0), kin, K)
            if c == 0:
                continue
            s = np.float32(one - np.float32(half * d[q, 0]))
            for j in range(1, c):
                s = np.float32(s + np.float32(one - np.float32(half * d[q, j])))
            out[q] = np.float32(s / np.float32(c))
    return out


def mean_similarity(dist_lists, counts, K) -> np.ndarray:
    """gulon_mean_similarity, the host form: dist_lists [b][kin] float32, counts [b] int32 or None -> [b] float32."""
    d = N.f32(dist_lists)
    if d.ndim != 2:
        raise ValueError("requirement failed: dist_lists is [b][kin]")
    b, kin = d.shape
    cnt = None if counts is None else N.i32(counts).reshape(-1)
    if cnt is not None and len(cnt) != b:
        raise ValueError("requirement failed: one count per list")
    out = np.zeros(max(b, 1), np.float32)
    N.check(N.lib().gulon_mean_similarity(d.reshape(-1) if d.size else np.zeros(1, np.float32),
                                          None if cnt is None or not b else cnt.ctypes.data, b, kin, K, out))
    return out[:b]


def translation_scores(keys, r_query) -> np.ndarray:
    """The CSLS scores behind the keys of a CSLS offset query, for display: (2 - t) - r_T(x) in float32, t = keys [b][k]
    (or [k]), r_query the mean similarity r_T of each query to its own nearest targets, [b] (or a scalar).  The padding
    (+inf) becomes -inf."""
    t = np.asarray(keys, np.float32)
    r = np.asarray(r_query, np.float32)
    if t.ndim == 2:
        r = r.reshape(-1, 1)
    return ((np.float32(2) - t).astype(np.float32) - r).astype(np.float32)


# ---- offsets on the device, and the query behind every batch_query_offset_raw -----------------------------------------------

class DeviceOffsets:
    """One float32 per row of an index, resident on the device: what csls_offsets returns and the batch_query_offset*
    methods take in the place of an array."""

    def __init__(self, rows):
        from .refine import _DeviceArray
        self.rows = int(rows)
        self._a = _DeviceArray()
        self._a.ensure(4 * max(self.rows, 1))

    @classmethod
    def from_host(cls, values):
        v = N.f32(values).reshape(-1)
        out = cls(len(v))
        if len(v):
            out._a.upload(v)
        return out

    @property
    def ptr(self):
        return self._a.ptr

    def numpy(self) -> np.ndarray:
        out = np.zeros(max(self.rows, 1), np.float32)
        self._a.download(out)
        return out[:self.rows]

    def free(self):
        self._a.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def offset_query_raw(host_fn, dev_fn, handle, span, dimension, rows, k, q, offsets, exclude):
    """gulon_*_query_offset behind the index classes.  host_fn / dev_fn: the two entry points; span: the arguments
    between k_nn and row_offsets (the index: from, until); rows: the length `offsets` must have; q [b][dimension]
    float32 as the handle takes them.  offsets: an array (the host form, which checks it) or DeviceOffsets (the _dev
    form: queries and answer cross once each, the offsets stay).
    -> (rows [b][k] with -1 after a query's last entry, keys [b][k] with +inf there, counts [b])."""
    q = N.f32(q).reshape(-1, dimension)
    b = len(q)
    ex = None if exclude is None else N.i32(exclude).reshape(-1)
    if ex is not None and len(ex) != b:
        raise ValueError(f"requirement failed: {len(ex)} excluded rows for {b} queries")
    oi, od = np.zeros((b, max(k, 1)), np.int32), np.zeros((b, max(k, 1)), np.float32)
    oc = np.zeros(max(b, 1), np.int32)
    one = np.zeros(1, np.float32)
    if isinstance(offsets, DeviceOffsets):
        if offsets.rows != rows:
            raise ValueError(f"requirement failed: {offsets.rows} offsets for {rows} rows")
        from .refine import _DeviceArray
        dev = {name: _DeviceArray() for name in ("q", "ex", "oi", "od", "oc")}
        try:
            dev["q"].upload(q if b else one)
            if ex is not None and b:
                dev["ex"].upload(ex)
            dev["oi"].ensure(oi.nbytes), dev["od"].ensure(od.nbytes), dev["oc"].ensure(oc.nbytes)
            N.check(dev_fn(handle, dev["q"].ptr, b, k, *span, offsets.ptr, dev["ex"].ptr if ex is not None and b else None,
                           dev["oi"].ptr, dev["od"].ptr, dev["oc"].ptr, None))
            if b and k >= 1:
                dev["oi"].download(oi), dev["od"].download(od), dev["oc"].download(oc)
        finally:
            for a in dev.values():
                a.free()
    else:
        off = N.f32(offsets).reshape(-1)
        if len(off) != rows:
            raise ValueError(f"requirement failed: {len(off)} offsets for {rows} rows")
        N.check(host_fn(handle, q.reshape(-1) if q.size else one, b, k, *span, off if len(off) else one,
                        None if ex is None or not b else ex.ctypes.data, oi.reshape(-1), od.reshape(-1), oc))
    return oi[:, :k], od[:, :k], oc[:b]


def host_offsets_for(index, offsets):
    """`offsets` as `index` will read them in every batch: the grouped index's entry point takes host pointers, so for a
    GroupedIndex (or a WordIndex over one) a DeviceOffsets is downloaded here, once; anything else is passed on."""
    from .grouped import GroupedIndex
    index = getattr(index, "index", index) if getattr(index, "_grouped", False) else index
    if isinstance(index, GroupedIndex) and isinstance(offsets, DeviceOffsets):
        if offsets.rows != index.size:
            raise ValueError(f"requirement failed: {offsets.rows} offsets for {index.size} rows")
        return offsets.numpy()
    return offsets


def batched_offset_query(index, dimension, k, vectors, offsets, exclude):
    """index.batch_query_offset_raw in batches of up to BATCH queries, as the word indexes ask it."""
    q = np.ascontiguousarray(vectors, np.float32).reshape(-1, dimension)
    ex = None if exclude is None else N.i32(exclude).reshape(-1)
    if ex is not None and len(ex) != len(q):
        raise ValueError(f"requirement failed: {len(ex)} excluded rows for {len(q)} queries")
    oi, od = np.full((len(q), k), -1, np.int32), np.full((len(q), k), np.inf, np.float32)
    oc = np.zeros(len(q), np.int32)
    offsets = host_offsets_for(index, offsets)
    for s in range(0, len(q), BATCH):
        oi[s:s + BATCH], od[s:s + BATCH], oc[s:s + BATCH] = index.batch_query_offset_raw(
            k, q[s:s + BATCH], offsets, None if ex is None else ex[s:s + BATCH])
    return oi, od, oc


def as_results(oi, od, oc) -> List[Result]:
    """The arrays of a batch_query_offset_raw as Results: `distances` holds the keys t, ascending; flags is 0 (the order
    (t, row) is total)."""
    return [Result(oi[i, :oc[i]].copy(), od[i, :oc[i]].copy(), 0) for i in range(len(oc))]


def _vector_side(index):
    """A target or source in any of its wrappings -> ("exact", ExactIndex), ("flat", SortedIndex | PQIndex) or
    ("grouped", GroupedIndex)."""
    from .exact import ExactIndex, ExactWordIndex
    from .grouped import GroupedIndex
    from .index import PQIndex, PQIndexView, SortedIndex
    from .word_index import WordIndex
    if isinstance(index, (ExactWordIndex, WordIndex)):
        index = index.index
    if isinstance(index, ExactIndex):
        return "exact", index
    if isinstance(index, GroupedIndex):
        return "grouped", index
    if isinstance(index, SortedIndex) or (isinstance(index, PQIndex) and not isinstance(index, PQIndexView)):
        return "flat", index
    raise NotImplementedError(f"{type(index).__name__} has no offset queries")


def _offset_sides(target, source, name):
    """(kind, target side, source ExactIndex) of `name` = csls_offsets / isf_offsets; ValueError for a source that is
    no exact index."""
    kind, tgt = _vector_side(target)
    skind, src = _vector_side(source)
    if skind != "exact":
        raise ValueError(f"requirement failed: the source of {name} is an exact index")
    return kind, tgt, src


def _target_span(kind, tgt, src, rule):
    """What csls_offsets and isf_offsets need of their target before the first pass.  ValueError for a target whose
    metric is known and not cosine (`rule` names who asks) and for a source of another dimension.
    -> (the number of offsets the target takes, the first and the row after the last to compute, compose): compose(off,
    rows, w, b, out) composes b one-term expressions where the target's rows live -- the dataset's rows of an exact
    target, the decoded rows of a flat one, GroupedIndex.lookup of a grouped one by grouped row position; normalised for a
    cosine index -- into the device array `out` [b][d], on the null stream."""
    from .index import SortedIndex
    metric = getattr(tgt, "metric", None)
    if metric is not None and metric != "cosine":
        raise ValueError(f"requirement failed: {rule} needs a cosine index")
    if src.dimension != tgt.dimension:
        raise ValueError(f"requirement failed: the source has {src.dimension} dimensions, the target {tgt.dimension}")
    L = N.lib()
    cosine = int(metric == "cosine")
    if kind == "exact":
        rows, first, last = tgt.matrix.rows, tgt.frm, tgt.until

        def compose(off, r, w, b, out):
            N.check(L.gulon_dataset_compose_rows_dev(tgt.matrix._h, off, r, w, b, cosine, cosine, out, None, None))
    elif kind == "grouped":                              # one offset per grouped row position
        rows, first, last = tgt.size, 0, tgt.size

        def compose(off, r, w, b, out):
            N.check(L.gulon_grouped_index_compose_rows_dev(tgt._h, off, r, w, b, cosine, cosine, out, None))
    else:
        pq = tgt.vector_index if isinstance(tgt, SortedIndex) else tgt
        rows, first, last = pq.length, 0, pq.length

        def compose(off, r, w, b, out):
            N.check(L.gulon_index_compose_rows_dev(pq._h, off, r, w, b, cosine, cosine, out, None))
    return rows, first, last, compose


def _composed_passes(span, d):
    """The batch loop of csls_offsets and isf_offsets over a _target_span: rows [first, last) in passes of
    ROWS_PER_PASS, each composed into one device array [b][d] that is yielded as (r0, b, array) -- both callers start
    from the same composed bits.  The device is synchronised after the last pass, before the arrays are freed."""
    from .refine import _DeviceArray
    _, first, last, compose = span
    dev = {name: _DeviceArray() for name in ("off", "rows", "w", "q")}
    try:
        for r0 in range(first, last, ROWS_PER_PASS):
            b = min(ROWS_PER_PASS, last - r0)
            dev["off"].upload(np.arange(b + 1, dtype=np.int32))
            dev["rows"].upload(np.arange(r0, r0 + b, dtype=np.int32))
            dev["w"].upload(np.ones(b, np.float32))
            dev["q"].ensure(4 * b * d)
            compose(dev["off"].ptr, dev["rows"].ptr, dev["w"].ptr, b, dev["q"].ptr)
            yield r0, b, dev["q"]
        N.check(N.lib().gulon_device_synchronize())
    finally:
        for a in dev.values():
            a.free()


def csls_offsets(target, source, neighbours=10) -> DeviceOffsets:
    """r_S of CSLS for every row of `target`: the mean cosine similarity of the row to its `neighbours` nearest rows of
    `source`, an ExactIndex (or ExactWordIndex) over the source vectors.  target: an ExactIndex, a SortedIndex / PQIndex
    over byte codes, a GroupedIndex, or a WordIndex / ExactWordIndex over one.  In batches of target rows, all on the
    null stream (_composed_passes): the rows composed where they live, the source's batch_query_dev at `neighbours` --
    the composed vectors taken as they are -- and gulon_mean_similarity_dev straight into the result.  -> DeviceOffsets
    with one value per target row (an exact target: per row of its matrix, +inf outside its range).  ValueError: a
    target whose metric is known and not cosine, a source of another dimension."""
    from .refine import _DeviceArray
    kind, tgt, src = _offset_sides(target, source, "csls_offsets")
    if neighbours < 1:
        raise ValueError(f"requirement failed: neighbours = {neighbours} < 1")
    span = _target_span(kind, tgt, src, "CSLS")
    out = DeviceOffsets.from_host(np.full(span[0], np.inf, np.float32))
    K, L = int(neighbours), N.lib()
    oi, od, oc = _DeviceArray(), _DeviceArray(), _DeviceArray()
    try:
        for r0, b, q in _composed_passes(span, tgt.dimension):
            oi.ensure(4 * b * K), od.ensure(4 * b * K), oc.ensure(4 * b)
            src.batch_query_dev(K, q.ptr, b, oi.ptr, od.ptr, oc.ptr)
            N.check(L.gulon_mean_similarity_dev(od.ptr, oc.ptr, b, K, K, C.c_void_p(out.ptr.value + 4 * r0), None))
    finally:
        for a in (oi, od, oc):
            a.free()
    return out


def _checked_sources(src, sources):
    """isf_offsets' `sources` before anything is made: None, an int N in [1, the source's rows], or distinct rows of the
    source's matrix inside its range as an int32 array; else ValueError."""
    if sources is None:
        return None
    if np.ndim(sources) == 0:
        if not 1 <= int(sources) <= src.size:
            raise ValueError(f"requirement failed: sources = {sources} outside [1, {src.size}]")
        return int(sources)
    rows = np.asarray(sources, np.int64).reshape(-1)
    if not len(rows) or rows.min() < src.frm or rows.max() >= src.until or len(np.unique(rows)) != len(rows):
        raise ValueError(f"requirement failed: sources: expected distinct rows in [{src.frm}, {src.until})")
    return N.i32(rows)


def _normaliser_scan(src, sources):
    """The handle isf_offsets sums over and what to close after it, for checked `sources`.  None: the source itself.
    An int N: a temporary ExactIndex over the first N rows of the source's range.  An array: a temporary ExactIndex over
    a device gather of those rows of the source's matrix, in the order given."""
    from .exact import ExactIndex
    from .matrix import DeviceMatrix
    if sources is None:
        return src, ()
    if isinstance(sources, int):
        scan = ExactIndex(src.matrix, src.metric, src.frm, src.frm + sources)
        return scan, (scan,)
    h = C.c_void_p()
    N.check(N.lib().gulon_dataset_gather(src.matrix._h, sources, len(sources), C.byref(h)))
    matrix = DeviceMatrix(h, len(sources), src.matrix.cols)
    scan = ExactIndex(matrix, src.metric)
    return scan, (scan, matrix)


def isf_offsets(target, source, beta=30.0, sources=None) -> DeviceOffsets:
    """The offsets of the inverted softmax (softmax.py) for every row of `target`: (2 / beta) * L(y),
    L(y) the log of the sum of exp(-(beta / 2) * d(x', y)) over the rows x' of `source`, an ExactIndex (or
    ExactWordIndex) over the source vectors.  target: as csls_offsets takes it.  Per pass of ROWS_PER_PASS target rows
    (_composed_passes, the loop csls_offsets runs) the composed batch is downloaded, asked of the source's
    batch_query_logsumexp, and softmax.isf_offsets_from fills the pass's slice.  A cosine source normalises what it is
    asked, as its batch_query_raw does: the composed rows, unit vectors already, are normalised once more on the way
    in, where csls_offsets hands them on as they are -- the two routes start from the same composed bits and may differ
    in the last bit of a component after that.
    sources restricts the normaliser, as Smith et al. sample it: an int N sums over the first N rows of the source,
    which are its N most frequent words ONLY where the rows are in the order of a word2vec file; an array sums over
    those rows of the source's matrix, in the order given (_normaliser_scan), which is how `translate --isf-sources` names the most frequent
    words of a source it holds in word order.
    -> DeviceOffsets with one value per target row (an exact target: per row of its matrix, +inf outside its range).
    ValueError: as csls_offsets; beta not finite or <= 0; sources outside [1, the source's rows] or not distinct rows of
    its range; a row all of whose terms underflow (beta too large for these distances)."""
    from .softmax import _beta, isf_offsets_from
    kind, tgt, src = _offset_sides(target, source, "isf_offsets")
    beta = _beta(beta)
    sources = _checked_sources(src, sources)
    span = _target_span(kind, tgt, src, "the inverted softmax")
    d = tgt.dimension
    host = np.full(span[0], np.inf, np.float32)
    scan, owned = _normaliser_scan(src, sources)
    try:
        for r0, b, q in _composed_passes(span, d):
            vectors = q.download(np.zeros((b, d), np.float32))
            host[r0:r0 + b] = isf_offsets_from(*scan.batch_query_logsumexp(vectors, beta), beta)
    finally:
        for x in owned:
            x.close()
    return DeviceOffsets.from_host(host)


# ---- dictionaries ------------------------------------------------------------------------------------------------------------

def read_dictionary(lines, lowercase=False) -> List[Tuple[str, str]]:
    """MUSE's bilingual dictionaries: every line is `source target`, split on whitespace; a source word may come back on
    several lines, each with another translation.  Blank lines are skipped; any other line must hold exactly two tokens,
    else ValueError naming its (1-based) line number.  -> [(source, target), ...] in file order."""
    pairs = []
    for number, line in enumerate(lines, 1):
        tokens = line.split()
        if not tokens:
            continue
        if len(tokens) != 2:
            raise ValueError(f"line {number}: expected a source and a target word, found {len(tokens)} tokens")
        if lowercase:
            tokens = [t.lower() for t in tokens]
        pairs.append((tokens[0], tokens[1]))
    return pairs


@dataclass
class TranslationReport:
    """Precision of dictionary induction: `asked` source words (each with at least one gold translation both sides
    have), `skipped` dictionary PAIRS with a word absent on either side, and per k the source words one of whose gold
    translations was among their first k answers."""
    ks: Tuple[int, ...]
    method: str = "nn"
    asked: int = 0
    skipped: int = 0
    hits: Dict[int, int] = field(default_factory=dict)

    def precision(self, k) -> float:
        return self.hits[k] / self.asked if self.asked else 0.0

    def line(self) -> str:
        scores = " ".join(f"@{k} {self.precision(k):.4f}" for k in sorted(self.hits))
        return f"{self.method}: {scores} (n = {self.asked}, skipped {self.skipped})"

    def lines(self) -> List[str]:
        return [self.line()]


def resolve_dictionary(target, source, pairs):
    """-> (source rows of the askable words in first-seen order, their sets of gold target rows, skipped pairs)."""
    gold: Dict[int, set] = {}
    skipped = 0
    for s, t in pairs:
        rs, rt = source.row_of(s), target.row_of(t)
        if rs is None or rt is None:
            skipped += 1
        else:
            gold.setdefault(int(rs), set()).add(int(rt))
    rows = list(gold)
    return rows, [gold[r] for r in rows], skipped


def score_lists(lists, counts, gold, ks) -> Dict[int, int]:
    """hits per k: lists [b][kmax] row ids, counts [b] live entries, gold [b] sets of rows."""
    hits = {int(k): 0 for k in ks}
    for row, c, g in zip(np.asarray(lists), np.asarray(counts), gold):
        first = next((j for j, r in enumerate(row[:int(c)].tolist()) if r in g), None)
        if first is not None:
            for k in hits:
                hits[k] += first < k
    return hits


def translation_lists(target, source, source_rows, k, method="nn", offsets=None):
    """The k translations of the source words at `source_rows` (rows of the source ExactWordIndex): per batch of up to
    BATCH words their vectors are looked up and asked of `target` -- "nn": its ordinary batch_query; "csls" and "isf":
    its batch_query_offset_raw with `offsets` (csls_offsets, isf_offsets).
    -> (rows [b][k] padded with -1, keys [b][k], counts [b])."""
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r}")
    rows = N.i32(source_rows).reshape(-1)
    oi, od = np.full((len(rows), k), -1, np.int32), np.full((len(rows), k), np.inf, np.float32)
    oc = np.zeros(len(rows), np.int32)
    if method in OFFSET_METHODS:
        offsets = host_offsets_for(target, offsets)              # a grouped target: one download for every batch
    for s in range(0, len(rows), BATCH):
        vectors = source.index.lookup_rows(rows[s:s + BATCH])
        if method in OFFSET_METHODS:
            oi[s:s + BATCH], od[s:s + BATCH], oc[s:s + BATCH] = target.batch_query_offset_raw(k, vectors, offsets)
        else:
            for i, r in enumerate(target.batch_query(k, vectors)):
                oc[s + i] = len(r.rows)
                oi[s + i, :oc[s + i]], od[s + i, :oc[s + i]] = r.rows, r.distances
    return oi, od, oc


def _check_pair(target, source, method):
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r}")
    if source.dimension != target.dimension:
        raise ValueError(f"requirement failed: the source has {source.dimension} dimensions, the target "
                         f"{target.dimension}")
    if method == "csls" and target.metric != "cosine":
        raise ValueError("requirement failed: CSLS needs a cosine index")
    if method == "isf" and target.metric != "cosine":
        raise ValueError("requirement failed: the inverted softmax needs a cosine index")


def method_offsets(target, source, method, neighbours=10, beta=30.0, sources=None) -> Optional[DeviceOffsets]:
    """The offsets `method` ranks by: csls_offsets at `neighbours`, isf_offsets at `beta` over `sources`, None for "nn"."""
    if method == "csls":
        return csls_offsets(target, source, neighbours)
    if method == "isf":
        return isf_offsets(target, source, beta, sources)
    return None


def translate_words(target, source, words, k, method="nn", neighbours=10, offsets=None, beta=30.0,
                    sources=None) -> List[Optional[WordResult]]:
    """Per source word its k translations among the target's words, None for a word the source lacks.  method "csls":
    `distances` of a result holds the keys d + r_S; "isf": the keys d + (2 / beta) * L, the normaliser over `sources`
    as isf_offsets takes it (None: every source row).  offsets: from an earlier csls_offsets / isf_offsets (None: computed
    here)."""
    _check_pair(target, source, method)
    words = list(words)
    rows = [source.row_of(w) for w in words]
    present = [i for i, r in enumerate(rows) if r is not None]
    out: List[Optional[WordResult]] = [None] * len(words)
    own = method in OFFSET_METHODS and offsets is None
    if own:
        offsets = method_offsets(target, source, method, neighbours, beta, sources)
    try:
        oi, od, oc = translation_lists(target, source, [rows[i] for i in present], k, method, offsets)
    finally:
        if own:
            offsets.free()
    for j, i in enumerate(present):
        ids = oi[j, :oc[j]]
        out[i] = WordResult([target.words[r] for r in ids.tolist()], od[j, :oc[j]].copy(), ids.copy(), 0)
    return out


def evaluate_dictionary(target, source, pairs: Sequence[Tuple[str, str]], ks=(1, 5, 10), method="nn",
                        neighbours=10, beta=30.0, sources=None) -> TranslationReport:
    """Precision@k of translating the dictionary's source words into the target's words.  target: a WordIndex over byte
    codes or an ExactWordIndex; source: an ExactWordIndex over the source vectors; pairs: read_dictionary.  A source word
    counts at k if any of its gold translations is among its first k answers; a pair with a word missing on either side
    is skipped and counted.  method "nn": the target's ordinary neighbours; "csls": its offset query with
    csls_offsets(target, source, neighbours), at most 63 answers per word; "isf": the same with
    isf_offsets(target, source, beta, sources).  ValueError: an unknown method, a source and target of different
    dimension, "csls" or "isf" on a target that is not cosine."""
    from .analogies import _check_ks
    ks = _check_ks(ks)
    _check_pair(target, source, method)
    rows, gold, skipped = resolve_dictionary(target, source, list(pairs))
    report = TranslationReport(ks, method, len(rows), skipped, {k: 0 for k in ks})
    if not rows:
        return report
    offsets = method_offsets(target, source, method, neighbours, beta, sources)
    try:
        oi, _, oc = translation_lists(target, source, rows, ks[-1], method, offsets)
    finally:
        if offsets is not None:
            offsets.free()
    report.hits = score_lists(oi, oc, gold, ks)
    return report
