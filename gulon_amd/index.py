"""Index (Index.scala): prepareQuery, PQIndex, SortedIndex, exactNearestNeighbours."""
import ctypes as C
import os
import weakref
from dataclasses import dataclass

import numpy as np

from . import native as N
from .matrix import Matrix, as_device
from .product_quantizer import EncodedMatrix, ProductQuantizer


@dataclass
class Result:
    """Index.Result (Index.scala:56-74) with int row ids instead of String keys
    (KeyIndex stays on the JVM side): ascending squared-L2 distances."""
    rows: np.ndarray
    distances: np.ndarray
    flags: int = 0

    def __len__(self):
        return len(self.rows)

    def __iter__(self):
        return iter(zip(self.rows.tolist(), self.distances.tolist()))


def prepare_query(pq: ProductQuantizer, queries):
    """Index.prepareQuery (Index.scala:352-383) -> [B][m][k] float32."""
    q = N.f32(queries)
    b, d = q.shape
    m, k = len(pq.quantizers), pq.num_clusters
    t = np.zeros((b, m, k), np.float32)
    N.check(N.lib().gulon_prepare_query(pq.flat_centroids(), d, m, k, q.reshape(-1) if b else np.zeros(1, np.float32),
                                        b, t.reshape(-1) if t.size else np.zeros(1, np.float32)))
    return t


def exact_nearest_neighbours(vectors, query, k, frm=0, until=None):
    """Index.exactNearestNeighbours (Index.scala:209-229) for one or many queries."""
    dm = as_device(vectors)
    q = N.f32(query)
    single = q.ndim == 1
    q = q.reshape(1, -1) if single else q
    until = dm.rows if until is None else until
    b = q.shape[0]
    oi = np.zeros((b, max(k, 1)), np.int32)
    od = np.zeros((b, max(k, 1)), np.float32)
    oc = np.zeros(max(b, 1), np.int32)
    of = np.zeros(max(b, 1), np.int32)
    N.check(N.lib().gulon_exact_knn(dm._h, frm, until, q.reshape(-1), b, k, oi.reshape(-1), od.reshape(-1), oc, of))
    res = [Result(oi[i, :oc[i]].copy(), od[i, :oc[i]].copy(), int(of[i])) for i in range(b)]
    return res[0] if single else res


_LIVE = weakref.WeakSet()     # open PQIndex handles and contexts (tune_live)


def tune_live(**knobs):
    """Tuning experiments and tests: sets the launch-shape knobs (GULON_SCAN_FILTER=0, GULON_FILTER_CAP=64, ...) in the
    environment -- where every handle created from now on takes them from -- and on every open handle and context
    (gulon_index_tuning).  The library has no process-wide setter; results never depend on the knobs."""
    for key, value in knobs.items():
        os.environ[key] = str(int(value))
        for ix in list(_LIVE):
            if ix._h is not None and ix._h.value:
                N.check(N.lib().gulon_index_tuning(ix._h, key.encode(), int(value)))


class PQIndex:
    """PQIndex(productQuantizer, data) (Index.scala:385-441): owns the HBM copy of the codes."""

    def __init__(self, product_quantizer: ProductQuantizer, data: EncodedMatrix, row_base=0, _handle=None):
        self.product_quantizer = product_quantizer
        self.data = data
        self.row_base = row_base
        _LIVE.add(self)
        if _handle is not None:
            self._h = _handle
            return
        h = C.c_void_p()
        packed = data.packed()
        N.check(N.lib().gulon_index_create(packed if packed.size else np.zeros(1, np.uint8), data.length,
                                           product_quantizer.dimension, len(product_quantizer.quantizers),
                                           product_quantizer.num_clusters, product_quantizer.flat_centroids(),
                                           row_base, C.byref(h)))
        self._h = h

    def context(self):
        """Another workspace over the same device-resident codes and codebooks (gulon_index_context_create):
        one per batch in flight / per querying thread; the codes live until the index and all its contexts
        are closed."""
        h = C.c_void_p()
        N.check(N.lib().gulon_index_context_create(self._h, C.byref(h)))
        return PQIndex(self.product_quantizer, self.data, self.row_base, _handle=h)

    @property
    def dimension(self):
        return self.product_quantizer.dimension

    @property
    def length(self):
        return self.data.length

    def batch_query_raw(self, k, vectors, frm=0, until=None):
        q = vectors.data if isinstance(vectors, Matrix) else N.f32(vectors)
        q = N.f32(q).reshape(-1, self.dimension)
        until = self.length if until is None else until
        b = q.shape[0]
        oi = np.zeros((b, max(k, 1)), np.int32)
        od = np.zeros((b, max(k, 1)), np.float32)
        oc = np.zeros(max(b, 1), np.int32)
        of = np.zeros(max(b, 1), np.int32)
        N.check(N.lib().gulon_index_batch_query(self._h, q.reshape(-1) if b else np.zeros(1, np.float32), b, k, frm,
                                                until, oi.reshape(-1), od.reshape(-1), oc, of))
        return oi[:, :k], od[:, :k], oc[:b], of[:b]

    def batch_query(self, k, vectors, frm=0, until=None):
        """PQIndex.batchQuery (Index.scala:417-440) + Result.fromHeap (Index.scala:83-94)."""
        oi, od, oc, of = self.batch_query_raw(k, vectors, frm, until)
        return [Result(oi[i, :oc[i]].copy(), od[i, :oc[i]].copy(), int(of[i])) for i in range(len(oc))]

    def query(self, k, query, frm=0, until=None):                     # Index.scala:411-412
        return self.batch_query(k, N.f32(query).reshape(1, -1), frm, until)[0]

    def decode(self, row):                                            # Index.scala:390-391
        idx = self.data.indices()[:, row]
        out = np.zeros(self.dimension, np.float32)
        for j, q in enumerate(self.product_quantizer.quantizers):
            out[q.frm:q.frm + q.dimension] = q.clusters.centroids[idx[j]]
        return out

    def decode_rows(self, rows, normalize=False):
        """ProductQuantizer.decode (ProductQuantizer.scala:37-50) of every row id in `rows`, on the device
        (gulon_index_decode_rows); normalize: MathUtils.normalize of each.  -> [len(rows)][d] float32."""
        r = N.i32(rows).reshape(-1)
        out = np.zeros((r.size, self.dimension), np.float32)
        if r.size:
            N.check(N.lib().gulon_index_decode_rows(self._h, r, r.size, int(bool(normalize)), out.reshape(-1)))
        else:
            N.check(N.lib().gulon_index_decode_rows(self._h, np.zeros(1, np.int32), 0, 0, np.zeros(1, np.float32)))
        return out

    def decode_matrix(self, frm=0, until=None):
        """ProductQuantizer.decode(EncodedMatrix) (ProductQuantizer.scala:58-78) of rows [frm, until) into HBM."""
        from .matrix import DeviceMatrix
        until = self.length if until is None else until
        h = C.c_void_p()
        N.check(N.lib().gulon_index_decode_dataset(self._h, frm, until, C.byref(h)))
        return DeviceMatrix(h, until - frm, self.dimension)

    def code_histogram(self, from_=0, until=None):
        """H[j][c] = the number of rows in [from_, until) whose code at quantizer j is c, counted on the device
        (gulon_index_code_histogram).  -> int64 [m][k]."""
        from .inspect import code_histogram_raw
        pq = self.product_quantizer
        return code_histogram_raw(N.lib().gulon_index_code_histogram, self._h, len(pq.quantizers), pq.num_clusters,
                                  self.length, from_, until)

    def row_errors(self, matrix, row_map=None, from_=0, until=None, norms=False):
        """MathUtils.distanceSq(matrix[row_map[r]], decode(r)) for every row r in [from_, until), on the device
        (gulon_index_row_errors); row_map None: the identity.  -> (row_error [until - from_] float32,
        quantizer_error [m] float64: the same sum restricted to each quantizer's coordinates, added over the rows)
        and, norms=True, row_norm_sq [until - from_]: the squared norms of the originals."""
        from .inspect import row_errors_raw
        return row_errors_raw(N.lib().gulon_index_row_errors, self._h, len(self.product_quantizer.quantizers),
                              self.length, matrix, row_map, from_, until, norms)

    def pair_distances(self, rows_a, rows_b):
        """MathUtils.distanceSq(decode(rows_a[i]), decode(rows_b[i])) for every i, on the device
        (gulon_index_pair_distances; similarity.pair_distance_reference).  -> [n] float32."""
        from .similarity import pair_distances_raw
        return pair_distances_raw(N.lib().gulon_index_pair_distances, self._h, rows_a, rows_b)

    def pair_distances_dev(self, d_rows_a, d_rows_b, n, d_dist, stream=None):
        """The device form: the rows and the distances device addresses; `stream` is waited for."""
        N.check(N.lib().gulon_index_pair_distances_dev(self._h, d_rows_a, d_rows_b, n, d_dist, stream))

    def batch_query_rows_raw(self, k, rows, frm=0, until=None, normalize=False):
        r = N.i32(rows).reshape(-1)
        until = self.length if until is None else until
        b = r.size
        oi = np.zeros((b, max(k, 1)), np.int32)
        od = np.zeros((b, max(k, 1)), np.float32)
        oc = np.zeros(max(b, 1), np.int32)
        of = np.zeros(max(b, 1), np.int32)
        N.check(N.lib().gulon_index_query_rows(self._h, r if b else np.zeros(1, np.int32), b, k, int(bool(normalize)),
                                               frm, until, oi.reshape(-1), od.reshape(-1), oc, of))
        return oi[:, :k], od[:, :k], oc[:b], of[:b]

    def batch_query_rows(self, k, rows, frm=0, until=None, normalize=False):
        """batchQuery(k, rows decoded) without leaving the device (gulon_index_query_rows): the same results as
        batch_query(k, decode_rows(rows, normalize), frm, until)."""
        oi, od, oc, of = self.batch_query_rows_raw(k, rows, frm, until, normalize)
        return [Result(oi[i, :oc[i]].copy(), od[i, :oc[i]].copy(), int(of[i])) for i in range(len(oc))]

    def compose_rows(self, expressions, normalize_terms=False, normalize_query=False):
        """The composed vector of every expression over row ids (expressions.py), on the device
        (gulon_index_compose_rows).  -> [len(expressions)][d] float32."""
        from .expressions import to_csr
        off, rows, w = to_csr(expressions)
        b = len(off) - 1
        out = np.zeros((b, self.dimension), np.float32)
        one_i, one_f = np.zeros(1, np.int32), np.zeros(1, np.float32)
        N.check(N.lib().gulon_index_compose_rows(self._h, off, rows if b else one_i, w if b else one_f, b,
                                                 int(bool(normalize_terms)), int(bool(normalize_query)),
                                                 out.reshape(-1) if out.size else one_f))
        return out

    def batch_query_terms_raw(self, k, expressions, extra, frm=0, until=None, normalize_terms=False,
                              normalize_query=False):
        """gulon_index_query_terms as it is: the answer at k + extra with every expression's term rows removed, the
        first k kept.  -> (rows [b][k], distances [b][k], counts [b], flags [b])."""
        from .expressions import to_csr
        off, rows, w = to_csr(expressions)
        b = len(off) - 1
        until = self.length if until is None else until
        oi = np.zeros((b, max(k, 1)), np.int32)
        od = np.zeros((b, max(k, 1)), np.float32)
        oc = np.zeros(max(b, 1), np.int32)
        of = np.zeros(max(b, 1), np.int32)
        one_i, one_f = np.zeros(1, np.int32), np.zeros(1, np.float32)
        N.check(N.lib().gulon_index_query_terms(self._h, off, rows if b else one_i, w if b else one_f, b, k, extra,
                                                int(bool(normalize_terms)), int(bool(normalize_query)), frm, until,
                                                oi.reshape(-1), od.reshape(-1), oc, of))
        return oi[:, :k], od[:, :k], oc[:b], of[:b]

    def batch_query_terms_partitioned(self, k, expressions, frm=0, until=None, normalize_terms=False,
                                      normalize_query=False):
        """batch_query_terms_raw per partition of the batch by its number E of distinct term rows, extra = E, in input
        order: (rows [b][k] with -1 after a query's last entry, distances [b][k], counts [b], flags [b])."""
        from .expressions import query_partitioned
        return query_partitioned(
            expressions,
            lambda part, extra: self.batch_query_terms_raw(k, part, extra, frm, until, normalize_terms, normalize_query),
            (((k,), np.int32, -1), ((k,), np.float32, np.inf), ((), np.int32, 0), ((), np.int32, 0)))

    def batch_query_terms(self, k, expressions, frm=0, until=None, normalize_terms=False, normalize_query=False):
        """Per expression: batchQuery(k + E, composed vector) with the E distinct term rows removed and the first k
        kept, without leaving the device between composing and the final list."""
        oi, od, oc, of = self.batch_query_terms_partitioned(k, expressions, frm, until, normalize_terms, normalize_query)
        return [Result(oi[i, :oc[i]].copy(), od[i, :oc[i]].copy(), int(of[i])) for i in range(len(oc))]

    def batch_query_cosmul_raw(self, k, expressions, frm=0, until=None, normalize=False):
        """gulon_index_query_cosmul: per expression over row ids the k rows of [frm, until) with the largest 3CosMul
        score that are none of its term rows (expressions.cosmul_reference).  -> (rows [b][k] with -1
        after an expression's last entry, SCORES [b][k] in descending order with -inf there, counts [b])."""
        from .expressions import to_csr
        off, rows, w = to_csr(expressions)
        b = len(off) - 1
        until = self.length if until is None else until
        oi = np.zeros((b, max(k, 1)), np.int32)
        od = np.zeros((b, max(k, 1)), np.float32)
        oc = np.zeros(max(b, 1), np.int32)
        one_i, one_f = np.zeros(1, np.int32), np.zeros(1, np.float32)
        N.check(N.lib().gulon_index_query_cosmul(self._h, off, rows if b else one_i, w if b else one_f, b, k,
                                                 int(bool(normalize)), frm, until, oi.reshape(-1), od.reshape(-1), oc))
        return oi[:, :k], od[:, :k], oc[:b]

    def batch_query_cosmul(self, k, expressions, frm=0, until=None, normalize=False):
        """batch_query_cosmul_raw as Results: `distances` holds the SCORES, in descending order; flags is 0 (the order
        (score descending, row ascending) is total)."""
        oi, od, oc = self.batch_query_cosmul_raw(k, expressions, frm, until, normalize)
        return [Result(oi[i, :oc[i]].copy(), od[i, :oc[i]].copy(), 0) for i in range(len(oc))]

    def batch_query_offset_raw(self, k, vectors, offsets, exclude=None, frm=0, until=None):
        """gulon_index_query_offset: per query (taken as given) the k rows of [frm, until) with the smallest
        t = distance + offsets[row] among those whose t is finite and that are not exclude[q] (a row id as returned, or
        -1), ties by row id (csls.offset_query_reference).  offsets: one float32 per row of the index, an
        array or the device array csls.csls_offsets returned.  1 <= k <= 63, byte codes, no view.  Offsets may be
        negative; NaN and -inf are refused (ValueError).  A query none of whose t is finite -- a NaN or infinite
        component, distances that overflow -- is answered with no row.  With a row_base, offsets stay indexed by the
        index's own rows, exclude and the answer carry the base.  Every byte-code index there is has a table of at most
        144 KiB (PQIndex refuses a larger m with NotImplementedError), which is what one query slot of the scan needs.
        -> (rows [b][k] with -1 after a query's last entry, keys t [b][k] with +inf there, counts [b])."""
        from .csls import offset_query_raw
        L = N.lib()
        until = self.length if until is None else until
        return offset_query_raw(L.gulon_index_query_offset, L.gulon_index_query_offset_dev, self._h, (frm, until),
                                self.dimension, self.length, k, vectors, offsets, exclude)

    def batch_query_offset(self, k, vectors, offsets, exclude=None, frm=0, until=None):
        """batch_query_offset_raw as Results: `distances` holds the keys t, ascending; flags is 0 (the order (t, row) is
        total)."""
        from .csls import as_results
        return as_results(*self.batch_query_offset_raw(k, vectors, offsets, exclude, frm, until))

    def batch_query_rank_raw(self, vectors, gold, offsets=None, exclude=None, frm=0, until=None):
        """gulon_index_query_rank: per query (taken as given) the best row of its gold list (an iterable of row ids as
        returned) in the order of batch_query_offset_raw over [frm, until) -- t = distance + offsets[row] finite, not
        exclude[q], by (t, row) -- and how many candidates come before it (ranks.rank_query_reference).
        No k: nothing is listed.  offsets: None (+0), an array or a csls.DeviceOffsets (downloaded: the entry point
        takes host pointers).  Byte codes, no view.
        -> (rank [b], -1 without a gold candidate; row [b], -1; key t [b], +inf; total [b] candidates)."""
        from .ranks import rank_query_raw
        until = self.length if until is None else until
        return rank_query_raw(N.lib().gulon_index_query_rank, self._h, (frm, until), self.dimension, self.length,
                              vectors, gold, offsets, exclude)

    def select(self, rows=None, mask=None):
        """The view of this index over a subset of its rows (gulon_index_select_*): an index of its own, gathered on
        the device, that answers in THIS index's row ids.  Exactly one of `rows` (strictly ascending row numbers) and
        `mask` (a bool array of length n, a packed uint64 array of ceil(n / 64) words -- bit r & 63 of word r >> 6 --
        or a torch device tensor of uint64 / int64 words, used where it lies)."""
        if (rows is None) == (mask is None):
            raise ValueError("select takes exactly one of rows and mask")
        h = C.c_void_p()
        if rows is not None:
            r = np.asarray(rows).reshape(-1)
            if r.size and not np.issubdtype(r.dtype, np.integer):
                raise ValueError("rows must be integers")
            if r.size and (r.min() < -2 ** 31 or r.max() >= 2 ** 31):
                bad = int(np.flatnonzero((r < -2 ** 31) | (r >= 2 ** 31))[0])
                raise ValueError(f"requirement failed: rows[{bad}] = {int(r[bad])} outside [0, {self.length})")
            r = N.i32(r)
            N.check(N.lib().gulon_index_select_rows(self._h, r if r.size else np.zeros(1, np.int32), r.size,
                                                    C.byref(h)))
        elif hasattr(mask, "data_ptr"):
            import torch
            words = (self.length + 63) // 64
            if not mask.is_cuda or mask.dtype not in (torch.uint64, torch.int64) or mask.numel() != words \
                    or not mask.is_contiguous():
                raise ValueError(f"a device mask is a contiguous uint64 / int64 tensor of {words} words")
            torch.cuda.current_stream(mask.device).synchronize()      # the mask is read on the library's stream
            N.check(N.lib().gulon_index_select_mask_dev(self._h, mask.data_ptr(), C.byref(h)))
        else:
            N.check(N.lib().gulon_index_select_mask(self._h, pack_mask(mask, self.length), C.byref(h)))
        return PQIndexView(self, h)

    def indices(self, frm=0, until=None):
        """EncodedMatrix.indices of rows [frm, until) read back from the device (gulon_index_get_codes): the centroid
        ids of the index's plain code buffer, un-blocked in HBM and copied down once.  -> int32 [m][until - frm].  A
        view answers in its own positions."""
        until = self.length if until is None else until
        m = len(self.product_quantizer.quantizers)
        out = np.zeros(max(m * max(until - frm, 0), 1), np.uint16)
        N.check(N.lib().gulon_index_get_codes(self._h, frm, until, out))
        return out[:m * (until - frm)].reshape(m, until - frm).astype(np.int32)

    def encode(self, matrix):
        """PQIndex(pq, pq.encode(matrix)) with pq the quantizer this index holds in HBM (gulon_index_encode_dataset):
        the rows of `matrix` (a DeviceMatrix is used where it lies) encoded in their order -- that order fixes the
        tie-break stream -- and written straight into a new index on the device.  -> a root index of matrix.rows rows."""
        dm = as_device(matrix)
        if dm.cols != self.dimension:
            raise ValueError(f"requirement failed: the vectors have {dm.cols} dimensions, the index {self.dimension}")
        h = C.c_void_p()
        N.check(N.lib().gulon_index_encode_dataset(self._h, dm._h, C.byref(h)))
        return DevicePQIndex(self.product_quantizer, h, dm.rows)

    def merged(self, other, take):
        """A new root index of len(take) rows gathered on the device (gulon_index_merge): row p carries the code of this
        index's row take[p] when take[p] >= 0, of `other`'s row -1 - take[p] otherwise; any order, repeats allowed.
        `other` (None: every entry is >= 0) must have this index's shape and bitwise equal code books."""
        t = np.asarray(take).reshape(-1)
        if t.size and not np.issubdtype(t.dtype, np.integer):
            raise ValueError("take must be integers")
        if t.size and (t.min() < -2 ** 31 or t.max() >= 2 ** 31):
            bad = int(np.flatnonzero((t < -2 ** 31) | (t >= 2 ** 31))[0])
            raise ValueError(f"requirement failed: take[{bad}] = {int(t[bad])} outside the int32 range")
        t = N.i32(t)
        h = C.c_void_p()
        N.check(N.lib().gulon_index_merge(self._h, other._h if other is not None else None,
                                          t if t.size else np.zeros(1, np.int32), t.size, C.byref(h)))
        return DevicePQIndex(self.product_quantizer, h, t.size)

    def close(self):
        if self._h is not None and self._h.value:
            N.lib().gulon_index_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DevicePQIndex(PQIndex):
    """An index made on the device (PQIndex.encode / PQIndex.merged): an ordinary root index whose codes exist in HBM
    only.  `data`, its EncodedMatrix, is read back through `indices` the first time it is asked for (dump_index)."""

    def __init__(self, product_quantizer, handle, length, _state=None):
        self.product_quantizer = product_quantizer
        self.row_base = 0
        self._h = handle
        self._length = length
        self._state = _state if _state is not None else {"data": None}      # shared with the contexts
        _LIVE.add(self)

    @property
    def length(self):
        return self._length

    @property
    def data(self):
        if self._state["data"] is None:
            coder = self.product_quantizer.coder_factory(self._length)
            self._state["data"] = EncodedMatrix(coder, [coder.build_code(ix) for ix in self.indices()])
        return self._state["data"]

    def context(self):
        h = C.c_void_p()
        N.check(N.lib().gulon_index_context_create(self._h, C.byref(h)))
        return DevicePQIndex(self.product_quantizer, h, self._length, _state=self._state)


def pack_mask(mask, n):
    """A row mask as ceil(n / 64) uint64 words, bit r & 63 of word r >> 6 for row r: from a bool array of length n, or
    from an array of that many words as it is."""
    m = np.asarray(mask)
    words = (n + 63) // 64
    if m.dtype == np.bool_:
        if m.shape != (n,):
            raise ValueError(f"a bool mask has one entry per row: {m.shape} for {n} rows")
        bits = np.zeros(words * 64, np.uint8)
        bits[:n] = m
        out = np.packbits(bits.reshape(words, 8, 8), axis=2, bitorder="little").reshape(words, 8)
        return np.ascontiguousarray(out).view("<u8").reshape(-1).astype(np.uint64) if words else np.zeros(1, np.uint64)
    if m.dtype not in (np.uint64, np.int64) or m.shape != (words,):
        raise ValueError(f"a packed mask is {words} uint64 words for {n} rows")
    return np.ascontiguousarray(m).view(np.uint64) if words else np.zeros(1, np.uint64)


def mask_rows(mask, n):
    """The rows a packed mask selects, ascending (bits at or above n ignored): the host statement of mask_to_rows."""
    w = np.ascontiguousarray(mask, np.uint64)[:(n + 63) // 64]
    bits = np.unpackbits(w.astype("<u8").view(np.uint8), bitorder="little")[:n]
    return np.flatnonzero(bits).astype(np.int32)


class PQIndexView(PQIndex):
    """A view (PQIndex.select): the PQIndex over the selected rows of `source`, in ascending order, on the device.  Its
    queries return row ids of the root index -- the index the first view was taken of; `positions_raw` the view's own
    positions.  frm / until, and the rows of decode_rows / batch_query_rows, are positions of the view."""

    def __init__(self, source, handle, _state=None):
        self.product_quantizer = source.product_quantizer
        self.row_base = 0
        self._h = handle
        # shared between a view and its contexts: the root's codes and the lazily downloaded rows
        self._state = _state if _state is not None else {
            "root": source._state["root"] if isinstance(source, PQIndexView) else source.data,
            "root_base": source._state["root_base"] if isinstance(source, PQIndexView) else source.row_base,
            "rows": None, "data": None}
        _LIVE.add(self)

    @property
    def length(self):
        s = C.c_int32(0)
        N.check(N.lib().gulon_index_view_size(self._h, C.byref(s)))
        return s.value

    @property
    def rows(self):
        """The selected rows (local rows of the root index), ascending."""
        if self._state["rows"] is None:
            out = np.zeros(max(self.length, 1), np.int32)
            N.check(N.lib().gulon_index_view_rows(self._h, out))
            self._state["rows"] = out[:self.length]
        return self._state["rows"]

    @property
    def data(self):
        """The EncodedMatrix of the view: the root's columns at `rows`."""
        if self._state["data"] is None:
            from .coder import Coder
            root = self._state["root"]
            coder = Coder(root.coder.width, self.length)
            self._state["data"] = EncodedMatrix(coder, [coder.build_code(ix[self.rows]) for ix in root.indices()])
        return self._state["data"]

    def context(self):
        h = C.c_void_p()
        N.check(N.lib().gulon_index_context_create(self._h, C.byref(h)))
        return PQIndexView(self, h, _state=self._state)

    def positions_raw(self, k, vectors, frm=0, until=None):
        """batch_query_raw in the view's own positions."""
        return PQIndex.batch_query_raw(self, k, vectors, frm, until)

    def batch_query_raw(self, k, vectors, frm=0, until=None):
        q = vectors.data if isinstance(vectors, Matrix) else N.f32(vectors)
        q = N.f32(q).reshape(-1, self.dimension)
        until = self.length if until is None else until
        b = q.shape[0]
        oi = np.zeros((b, max(k, 1)), np.int32)
        od = np.zeros((b, max(k, 1)), np.float32)
        oc = np.zeros(max(b, 1), np.int32)
        of = np.zeros(max(b, 1), np.int32)
        N.check(N.lib().gulon_index_view_batch_query(self._h, q.reshape(-1) if b else np.zeros(1, np.float32), b, k,
                                                     frm, until, oi.reshape(-1), od.reshape(-1), oc, of))
        return oi[:, :k], od[:, :k], oc[:b], of[:b]

    def map_positions(self, positions):
        """Positions of the view -> row ids of the root index; negative entries (padding) stay."""
        p = N.i32(positions)
        if not self.length:
            return p
        live = (p >= 0) & (p < self.length)
        return np.where(live, self._state["root_base"] + self.rows[np.where(live, p, 0)], p).astype(np.int32)

    def batch_query_rows_raw(self, k, rows, frm=0, until=None, normalize=False):
        oi, od, oc, of = PQIndex.batch_query_rows_raw(self, k, rows, frm, until, normalize)
        return self.map_positions(oi), od, oc, of


def normalize(xs):
    """MathUtils.normalize (MathUtils.scala:100-120): sequential fp32 sum, math.sqrt in double."""
    xs = N.f32(xs)
    s = np.float32(0)
    for x in xs:
        s = np.float32(s + np.float32(x * x))
    dist = np.float32(np.sqrt(np.float64(s)))
    return (xs / dist).astype(np.float32)


class SortedIndex:
    """Index.SortedIndex (Index.scala:310-337) without the String key index."""

    def __init__(self, vector_index: PQIndex, metric="l2"):
        self.vector_index = vector_index
        self.metric = metric

    @property
    def dimension(self):
        return self.vector_index.dimension

    @property
    def size(self):
        return self.vector_index.length

    def _prepare(self, q):                                            # Index.scala:324-331
        q = N.f32(q.data if isinstance(q, Matrix) else q).reshape(-1, self.dimension)
        if self.metric == "cosine":
            q = np.stack([normalize(r) for r in q]) if len(q) else q
        return q

    def batch_query(self, k, vectors):                                # Index.scala:333-336
        return self.vector_index.batch_query(k, self._prepare(vectors))

    def query(self, k, vector):                                       # Index.scala:321-322
        return self.batch_query(k, N.f32(vector).reshape(1, -1))[0]

    def lookup_row(self, row):                                        # Index.scala:318-319
        return self.vector_index.decode(row)

    def lookup_rows(self, rows):                                      # Index.scala:318-319, on the device
        return self.vector_index.decode_rows(rows)

    def batch_query_rows(self, k, rows):
        """Index.queryByWord (Index.scala:38-45) on row ids: query(k, lookup(row)) for every row, decoded (and for a
        cosine index normalised, Index.scala:324-331) on the device."""
        return self.vector_index.batch_query_rows(k, rows, normalize=self.metric == "cosine")

    def pair_distances(self, rows_a, rows_b):
        """The distance between lookup_rows(rows_a)[i] and lookup_rows(rows_b)[i] for every i, on the device."""
        return self.vector_index.pair_distances(rows_a, rows_b)

    def pair_distances_dev(self, d_rows_a, d_rows_b, n, d_dist, stream=None):
        self.vector_index.pair_distances_dev(d_rows_a, d_rows_b, n, d_dist, stream)

    def code_histogram(self, from_=0, until=None):
        return self.vector_index.code_histogram(from_, until)

    def row_errors(self, matrix, row_map=None, from_=0, until=None, norms=False):
        return self.vector_index.row_errors(matrix, row_map, from_, until, norms)

    def select(self, rows=None, mask=None):
        """A SortedIndex over the view of the selected rows (PQIndex.select), same metric: its results name rows of
        this index."""
        return SortedIndex(self.vector_index.select(rows, mask), self.metric)

    def updated(self, take, added=None):
        """A SortedIndex over take's rows (PQIndex.merged), same metric: take[p] >= 0 keeps this index's row take[p] with
        its code, take[p] < 0 is row -1 - take[p] of `added` -- a matrix encoded in its row order by this index's own
        quantizer (PQIndex.encode; for a cosine index the rows are normalised already).  This index is untouched."""
        new = self.vector_index.encode(added) if added is not None else None
        try:
            return SortedIndex(self.vector_index.merged(new, take), self.metric)
        finally:
            if new is not None:
                new.close()

    def compose_rows(self, expressions):
        """The query vector of every expression over row ids as this index prepares it: terms and sum normalised for a
        cosine index (expressions.py)."""
        cosine = self.metric == "cosine"
        return self.vector_index.compose_rows(expressions, cosine, cosine)

    def batch_query_expressions_raw(self, k, expressions):
        cosine = self.metric == "cosine"
        return self.vector_index.batch_query_terms_partitioned(k, expressions, normalize_terms=cosine,
                                                               normalize_query=cosine)

    def batch_query_expressions(self, k, expressions):
        """Per expression over row ids the k nearest rows of its composed vector that are none of its operands."""
        cosine = self.metric == "cosine"
        return self.vector_index.batch_query_terms(k, expressions, normalize_terms=cosine, normalize_query=cosine)


    def batch_query_cosmul_raw(self, k, expressions):
        """PQIndex.batch_query_cosmul_raw over all rows, the term vectors normalised for a cosine index: (rows,
        SCORES in descending order, counts)."""
        return self.vector_index.batch_query_cosmul_raw(k, expressions, normalize=self.metric == "cosine")

    def batch_query_cosmul(self, k, expressions):
        """Per expression over row ids the k rows with the largest 3CosMul score that are none of its operands;
        `distances` of a Result holds the SCORES, in descending order."""
        return self.vector_index.batch_query_cosmul(k, expressions, normalize=self.metric == "cosine")

    def batch_query_offset_raw(self, k, vectors, offsets, exclude=None):
        """PQIndex.batch_query_offset_raw over all rows, the queries normalised for a cosine index: (rows, keys
        distance + offsets[row] in ascending order, counts)."""
        return self.vector_index.batch_query_offset_raw(k, self._prepare(vectors), offsets, exclude)

    def batch_query_offset(self, k, vectors, offsets, exclude=None):
        """Per query the k rows with the smallest distance + offsets[row] among the rows whose sum is finite and that
        are not exclude[q]; `distances` of a Result holds those keys."""
        return self.vector_index.batch_query_offset(k, self._prepare(vectors), offsets, exclude)

    def batch_query_rank_raw(self, vectors, gold, offsets=None, exclude=None):
        """PQIndex.batch_query_rank_raw over all rows, the queries normalised for a cosine index (prepared as
        batch_query_offset_raw prepares them): (rank, row, key, total)."""
        return self.vector_index.batch_query_rank_raw(self._prepare(vectors), gold, offsets, exclude)



class Index:
    @staticmethod
    def sorted(vectors, quantizer: ProductQuantizer, metric="l2") -> SortedIndex:
        """Index.sorted (Index.scala:107-114): encode, then wrap."""
        encoded = quantizer.encode(as_device(vectors))
        return SortedIndex(PQIndex(quantizer, encoded), metric)

    @staticmethod
    def grouped(grouped_vectors, residuals_quantizer: ProductQuantizer, strategy, metric="l2"):
        """Index.grouped (Index.scala:133-147): the quantizer is one on the RESIDUALS."""
        from .grouped import grouped
        return grouped(grouped_vectors, residuals_quantizer, strategy, metric)
