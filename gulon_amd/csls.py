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
  evaluate_dictionary  precision@k of a bilingual dictionary (MUSE's format, read_dictionary), plain ("nn") or "csls"
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
METHODS = ("nn", "csls")


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


def csls_offsets(target, source, neighbours=10) -> DeviceOffsets:
    """r_S of CSLS for every row of `target`: the mean cosine similarity of the row to its `neighbours` nearest rows of
    `source`, an ExactIndex (or ExactWordIndex) over the source vectors.  target: an ExactIndex, a SortedIndex / PQIndex
    over byte codes, a GroupedIndex, or a WordIndex / ExactWordIndex over one.  In batches of target rows, all on the
    null stream: the rows composed where they live as one-term expressions (the dataset's rows of an exact target, the
    decoded rows of a flat one, GroupedIndex.lookup of a grouped one by grouped row position; normalised for a cosine
    index), the source's batch_query_dev at `neighbours`, gulon_mean_similarity_dev
    straight into the result.  -> DeviceOffsets with one value per target row (an exact target: per row of its matrix,
    +inf outside its range).  ValueError: a target whose metric is known and not cosine, a source of another
    dimension."""
    from .exact import ExactIndex
    from .index import SortedIndex
    from .refine import _DeviceArray
    kind, tgt = _vector_side(target)
    skind, src = _vector_side(source)
    if skind != "exact":
        raise ValueError("requirement failed: the source of csls_offsets is an exact index")
    if neighbours < 1:
        raise ValueError(f"requirement failed: neighbours = {neighbours} < 1")
    metric = getattr(tgt, "metric", None)
    if metric is not None and metric != "cosine":
        raise ValueError("requirement failed: CSLS needs a cosine index")
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
    out = DeviceOffsets.from_host(np.full(rows, np.inf, np.float32))
    K, d = int(neighbours), tgt.dimension
    dev = {name: _DeviceArray() for name in ("off", "rows", "w", "q", "oi", "od", "oc")}
    try:
        for r0 in range(first, last, ROWS_PER_PASS):
            b = min(ROWS_PER_PASS, last - r0)
            dev["off"].upload(np.arange(b + 1, dtype=np.int32))
            dev["rows"].upload(np.arange(r0, r0 + b, dtype=np.int32))
            dev["w"].upload(np.ones(b, np.float32))
            dev["q"].ensure(4 * b * d), dev["oi"].ensure(4 * b * K), dev["od"].ensure(4 * b * K), dev["oc"].ensure(4 * b)
            compose(dev["off"].ptr, dev["rows"].ptr, dev["w"].ptr, b, dev["q"].ptr)
            src.batch_query_dev(K, dev["q"].ptr, b, dev["oi"].ptr, dev["od"].ptr, dev["oc"].ptr)
            N.check(L.gulon_mean_similarity_dev(dev["od"].ptr, dev["oc"].ptr, b, K, K,
                                                C.c_void_p(out.ptr.value + 4 * r0), None))
        N.check(L.gulon_device_synchronize())
    finally:
        for a in dev.values():
            a.free()
    return out


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
    BATCH words their vectors are looked up and asked of `target` -- "nn": its ordinary batch_query; "csls": its
    batch_query_offset_raw with `offsets` (csls_offsets).  -> (rows [b][k] padded with -1, keys [b][k], counts [b])."""
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r}")
    rows = N.i32(source_rows).reshape(-1)
    oi, od = np.full((len(rows), k), -1, np.int32), np.full((len(rows), k), np.inf, np.float32)
    oc = np.zeros(len(rows), np.int32)
    if method == "csls":
        offsets = host_offsets_for(target, offsets)              # a grouped target: one download for every batch
    for s in range(0, len(rows), BATCH):
        vectors = source.index.lookup_rows(rows[s:s + BATCH])
        if method == "csls":
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


def translate_words(target, source, words, k, method="nn", neighbours=10, offsets=None) -> List[Optional[WordResult]]:
    """Per source word its k translations among the target's words, None for a word the source lacks.  method "csls":
    `distances` of a result holds the keys d + r_S; offsets: r_S from an earlier csls_offsets (None: computed here)."""
    _check_pair(target, source, method)
    words = list(words)
    rows = [source.row_of(w) for w in words]
    present = [i for i, r in enumerate(rows) if r is not None]
    out: List[Optional[WordResult]] = [None] * len(words)
    own = method == "csls" and offsets is None
    if own:
        offsets = csls_offsets(target, source, neighbours)
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
                        neighbours=10) -> TranslationReport:
    """Precision@k of translating the dictionary's source words into the target's words.  target: a WordIndex over byte
    codes or an ExactWordIndex; source: an ExactWordIndex over the source vectors; pairs: read_dictionary.  A source word
    counts at k if any of its gold translations is among its first k answers; a pair with a word missing on either side
    is skipped and counted.  method "nn": the target's ordinary neighbours; "csls": its offset query with
    csls_offsets(target, source, neighbours), at most 63 answers per word.  ValueError: an unknown method, a source and
    target of different dimension, "csls" on a target that is not cosine."""
    from .analogies import _check_ks
    ks = _check_ks(ks)
    _check_pair(target, source, method)
    rows, gold, skipped = resolve_dictionary(target, source, list(pairs))
    report = TranslationReport(ks, method, len(rows), skipped, {k: 0 for k in ks})
    if not rows:
        return report
    offsets = csls_offsets(target, source, neighbours) if method == "csls" else None
    try:
        oi, _, oc = translation_lists(target, source, rows, ks[-1], method, offsets)
    finally:
        if offsets is not None:
            offsets.free()
    report.hits = score_lists(oi, oc, gold, ks)
    return report
