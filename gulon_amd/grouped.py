"""GroupedIndex (Index.scala:231-308) and the grouping of the vectors behind it
(WordVectors.grouped / Grouped.residuals, WordVectors.scala:24-58,118-138).

Build (CommandUtils.scala:127-147, command/BuildIndex): coarse KMeans on the full vectors ->
`group` (par_assign on the original order + stable ordering by word and cluster, group centroids, group
offsets, residual matrix on the device) -> ProductQuantizer on the residuals -> `Index.grouped`.
Row ids of a GroupedIndex are positions in the GROUPED order; `GroupedVectors.perm` maps them back.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import native as N
from .kmeans import KMeans
from .matrix import DeviceMatrix, as_device
from .product_quantizer import EncodedMatrix, ProductQuantizer
from .vectors import Vectors


@dataclass(frozen=True)
class LimitGroups:                     # GroupedIndex.Strategy.LimitGroups (Index.scala:304)
    count: int


@dataclass(frozen=True)
class LimitVectors:                    # GroupedIndex.Strategy.LimitVectors (Index.scala:305)
    count: int


@dataclass
class GroupedVectors:
    """WordVectors.Grouped without the keys (those stay with the caller)."""
    perm: np.ndarray                   # grouped position -> original row
    centroids: np.ndarray              # [g][d] centroids of the groups (a leading empty group is possible, see group)
    offsets: np.ndarray                # [g-1] first grouped row of groups 1..g-1
    residuals: DeviceMatrix            # grouped row - its group's centroid, resident in HBM

    @property
    def size(self):
        return len(self.perm)

    def cluster_of(self, i):           # WordVectors.Grouped.clusterOf (WordVectors.scala:110-113)
        return int(np.searchsorted(self.offsets, i, side="right"))


def group(vectors, clustering: KMeans, word_order=None) -> GroupedVectors:
    """WordVectors.grouped (WordVectors.scala:24-58).

    parAssign runs over the rows in the order given (the reference assigns BEFORE it sorts, so the
    25 000-row tie-break streams see the original order, :27); `word_order` = row indices stably sorted by
    word (:28-29; None: the rows are already in word order); rows are then stably ordered by cluster (:30).
    The builder loop is seeded with the cluster of ORIGINAL row 0 (`prev = assignments(0)`, :38-39): when that
    is not the lowest-numbered non-empty cluster the reference emits a leading empty group [0, 0) with a
    copy of row 0's centroid -- reproduced here (offsets[0] == 0), since it changes what LimitGroups(m)
    searches and what the index file holds."""
    if clustering.k <= 0:
        raise ValueError("requirement failed: must have at least 1 cluster")
    dm = as_device(vectors)
    assignments = clustering.par_assign(Vectors(dm))
    n = len(assignments)
    order = np.arange(n, dtype=np.int64) if word_order is None else np.asarray(word_order, np.int64)
    perm = order[np.argsort(assignments[order], kind="stable")].astype(np.int32)
    sa = assignments[perm]
    if n == 0:
        return GroupedVectors(perm, np.zeros((0, dm.cols), np.float32), np.zeros(0, np.int32), dm)
    change = np.r_[sa[0] != assignments[0], sa[1:] != sa[:-1]]          # `prev != a` at grouped position i
    offsets = np.flatnonzero(change).astype(np.int32)
    cent_ids = np.r_[assignments[0], sa[offsets]]
    centroids = np.ascontiguousarray(N.f32(clustering.centroids)[cent_ids])
    g = len(cent_ids)
    group_of = np.searchsorted(offsets, np.arange(n), side="right").astype(np.int32)
    h = C.c_void_p()
    N.check(N.lib().gulon_dataset_group_residuals(dm._h, perm, group_of, centroids.reshape(-1), g, C.byref(h)))
    return GroupedVectors(perm, centroids, offsets, DeviceMatrix(h, dm.rows, dm.cols))


class GroupedIndex:
    """Index.GroupedIndex over row ids."""

    def __init__(self, quantizer: ProductQuantizer, encoded_residuals: EncodedMatrix, centroids, offsets,
                 strategy, metric="l2"):
        self.quantizer, self.data = quantizer, encoded_residuals
        self.centroids = N.f32(centroids).reshape(-1, quantizer.dimension)
        self.offsets = np.ascontiguousarray(offsets, np.int32)
        if len(self.centroids) != len(self.offsets) + 1:        # the reference's assert, Index.scala:240-241
            raise AssertionError(f"{len(self.centroids)} != {len(self.offsets)} + 1")
        self.strategy, self.metric = strategy, metric
        h = C.c_void_p()
        packed = encoded_residuals.packed()
        N.check(N.lib().gulon_grouped_index_create(
            packed if packed.size else np.zeros(1, np.uint8), encoded_residuals.length, quantizer.dimension,
            len(quantizer.quantizers), quantizer.num_clusters, quantizer.flat_centroids(),
            self.centroids.reshape(-1), self.offsets if len(self.offsets) else np.zeros(1, np.int32),
            len(self.centroids), C.byref(h)))
        self._h = h

    @property
    def dimension(self):
        return self.quantizer.dimension

    @property
    def size(self):
        return self.data.length

    def _strategy(self):
        if isinstance(self.strategy, LimitGroups):
            return 0, int(self.strategy.count)
        if isinstance(self.strategy, LimitVectors):
            return 1, int(self.strategy.count)
        raise ValueError("strategy must be LimitGroups or LimitVectors")

    def batch_query_raw(self, k, vectors):
        from .index import normalize
        q = N.f32(vectors.data if hasattr(vectors, "data") and not isinstance(vectors, np.ndarray) else vectors)
        q = q.reshape(-1, self.dimension)
        if self.metric == "cosine" and len(q):
            q = np.stack([normalize(r) for r in q])
        b = q.shape[0]
        s, limit = self._strategy()
        oi = np.zeros((b, max(k, 1)), np.int32)
        od = np.zeros((b, max(k, 1)), np.float32)
        oc = np.zeros(max(b, 1), np.int32)
        N.check(N.lib().gulon_grouped_index_batch_query(self._h, q.reshape(-1) if b else np.zeros(1, np.float32), b, k,
                                                        s, limit, oi.reshape(-1), od.reshape(-1), oc))
        return oi[:, :k], od[:, :k], oc[:b]

    def batch_query(self, k, vectors):
        """GroupedIndex.batchQuery (Index.scala:254-257): one GroupedIndex.query per row."""
        from .index import Result
        oi, od, oc = self.batch_query_raw(k, vectors)
        return [Result(oi[i, :oc[i]].copy(), od[i, :oc[i]].copy(), 0) for i in range(len(oc))]

    def query(self, k, query):                                   # Index.scala:265-282
        return self.batch_query(k, N.f32(query).reshape(1, -1))[0]

    def lookup_rows(self, rows):
        """GroupedIndex.lookup (Index.scala:247-253) of every row id in `rows`, on the device:
        centroids(partition) + decode(row), the partition by the reference's Arrays.binarySearch(offsets, row) --
        which, where offsets repeat, can differ from the row's own group (cluster_of)."""
        r = N.i32(rows).reshape(-1)
        out = np.zeros((r.size, self.dimension), np.float32)
        if r.size:
            N.check(N.lib().gulon_grouped_index_lookup_rows(self._h, r, r.size, 0, out.reshape(-1)))
        else:
            N.check(N.lib().gulon_grouped_index_lookup_rows(self._h, np.zeros(1, np.int32), 0, 0,
                                                            np.zeros(1, np.float32)))
        return out

    def lookup_row(self, row):
        return self.lookup_rows([row])[0]

    def pair_distances(self, rows_a, rows_b):
        """MathUtils.distanceSq(lookup_rows(rows_a)[i], lookup_rows(rows_b)[i]) for every i, on the device
        (gulon_grouped_index_pair_distances): between the vectors lookup_rows hands out, so with ITS partition rule, not
        with the row's own group as row_errors.  -> [n] float32."""
        from .similarity import pair_distances_raw
        return pair_distances_raw(N.lib().gulon_grouped_index_pair_distances, self._h, rows_a, rows_b)

    def pair_distances_dev(self, d_rows_a, d_rows_b, n, d_dist, stream=None):
        """The device form: the rows and the distances device addresses; `stream` is waited for."""
        N.check(N.lib().gulon_grouped_index_pair_distances_dev(self._h, d_rows_a, d_rows_b, n, d_dist, stream))

    def code_histogram(self, from_=0, until=None):
        """H[j][c] = the number of rows in [from_, until) whose residual code at quantizer j is c, counted on the
        device (gulon_grouped_index_code_histogram).  -> int64 [m][k]."""
        from .inspect import code_histogram_raw
        return code_histogram_raw(N.lib().gulon_grouped_index_code_histogram, self._h, len(self.quantizer.quantizers),
                                  self.quantizer.num_clusters, self.size, from_, until)

    def row_errors(self, matrix, row_map=None, from_=0, until=None, norms=False):
        """As PQIndex.row_errors, against the vector a query compares with: the centroid of the row's OWN group
        (cluster_of: the group whose row range holds it, which is where a query scans it) + decode(row).  Where
        offsets repeat this is not always the group lookup_rows adds (the reference's binarySearch rule)."""
        from .inspect import row_errors_raw
        return row_errors_raw(N.lib().gulon_grouped_index_row_errors, self._h, len(self.quantizer.quantizers),
                              self.size, matrix, row_map, from_, until, norms)

    def batch_query_rows_raw(self, k, rows):
        r = N.i32(rows).reshape(-1)
        b = r.size
        s, limit = self._strategy()
        oi = np.zeros((b, max(k, 1)), np.int32)
        od = np.zeros((b, max(k, 1)), np.float32)
        oc = np.zeros(max(b, 1), np.int32)
        N.check(N.lib().gulon_grouped_index_query_rows(self._h, r if b else np.zeros(1, np.int32), b, k,
                                                       int(self.metric == "cosine"), s, limit, oi.reshape(-1),
                                                       od.reshape(-1), oc))
        return oi[:, :k], od[:, :k], oc[:b]

    def batch_query_rows(self, k, rows):
        """Index.queryByWord (Index.scala:38-45) on row ids: query(k, lookup(row)) for every row, looked up (and for a
        cosine index normalised) on the device."""
        from .index import Result
        oi, od, oc = self.batch_query_rows_raw(k, rows)
        return [Result(oi[i, :oc[i]].copy(), od[i, :oc[i]].copy(), 0) for i in range(len(oc))]

    def compose_rows(self, expressions, normalize_terms=None, normalize_query=None):
        """The composed vector of every expression over grouped row positions (expressions.py), on the device
        (gulon_grouped_index_compose_rows); the flags default to what the metric asks for.  -> [b][d] float32."""
        from .expressions import to_csr
        cosine = self.metric == "cosine"
        nt = cosine if normalize_terms is None else bool(normalize_terms)
        nq = cosine if normalize_query is None else bool(normalize_query)
        off, rows, w = to_csr(expressions)
        b = len(off) - 1
        out = np.zeros((b, self.dimension), np.float32)
        one_i, one_f = np.zeros(1, np.int32), np.zeros(1, np.float32)
        N.check(N.lib().gulon_grouped_index_compose_rows(self._h, off, rows if b else one_i, w if b else one_f, b,
                                                         int(nt), int(nq), out.reshape(-1) if out.size else one_f))
        return out

    def batch_query_terms_raw(self, k, expressions, extra):
        """gulon_grouped_index_query_terms as it is: the answer at k + extra with every expression's term rows removed,
        the first k kept.  -> (rows [b][k], distances [b][k], counts [b])."""
        from .expressions import to_csr
        off, rows, w = to_csr(expressions)
        b = len(off) - 1
        s, limit = self._strategy()
        cosine = int(self.metric == "cosine")
        oi = np.zeros((b, max(k, 1)), np.int32)
        od = np.zeros((b, max(k, 1)), np.float32)
        oc = np.zeros(max(b, 1), np.int32)
        one_i, one_f = np.zeros(1, np.int32), np.zeros(1, np.float32)
        N.check(N.lib().gulon_grouped_index_query_terms(self._h, off, rows if b else one_i, w if b else one_f, b, k,
                                                        extra, cosine, cosine, s, limit, oi.reshape(-1), od.reshape(-1),
                                                        oc))
        return oi[:, :k], od[:, :k], oc[:b]

    def batch_query_expressions_raw(self, k, expressions):
        """batch_query_terms_raw per partition of the batch by its number E of distinct term rows, extra = E, in input
        order: (rows [b][k] with -1 after a query's last entry, distances [b][k], counts [b], flags [b] = 0)."""
        from .expressions import query_partitioned
        oi, od, oc = query_partitioned(expressions, lambda part, extra: self.batch_query_terms_raw(k, part, extra),
                                       (((k,), np.int32, -1), ((k,), np.float32, np.inf), ((), np.int32, 0)))
        return oi, od, oc, np.zeros(len(oc), np.int32)

    def batch_query_expressions(self, k, expressions):
        """Per expression over grouped row positions the k nearest rows of its composed vector that are none of its
        operands: GroupedIndex.batchQuery at k + E, the E distinct operands removed, the first k kept."""
        from .index import Result
        oi, od, oc, _ = self.batch_query_expressions_raw(k, expressions)
        return [Result(oi[i, :oc[i]].copy(), od[i, :oc[i]].copy(), 0) for i in range(len(oc))]

    # ---- offset queries (csls.py): the offsets are indexed by grouped row position
    def batch_query_offset_raw(self, k, vectors, offsets, exclude=None):
        """gulon_grouped_index_query_offset: per query (normalised for a cosine index, as batch_query_raw does) the k
        rows of its searched groups with the smallest t = distance + offsets[row] among those whose t is finite and
        that are not exclude[q] (None, or one grouped row position or -1 per query), by (t, row).  offsets: one float32
        per row, an array or a csls.DeviceOffsets -- the entry point takes host pointers, so a DeviceOffsets is
        downloaded.  -> (rows [b][k] with -1 after a query's last entry, keys [b][k] with +inf there, counts [b])."""
        from .csls import DeviceOffsets, offset_query_raw
        from .index import normalize
        q = N.f32(vectors.data if hasattr(vectors, "data") and not isinstance(vectors, np.ndarray) else vectors)
        q = q.reshape(-1, self.dimension)
        if self.metric == "cosine" and len(q):
            q = np.stack([normalize(r) for r in q])
        if isinstance(offsets, DeviceOffsets):
            if offsets.rows != self.size:
                raise ValueError(f"requirement failed: {offsets.rows} offsets for {self.size} rows")
            offsets = offsets.numpy()
        return offset_query_raw(N.lib().gulon_grouped_index_query_offset, None, self._h, self._strategy(),
                                self.dimension, self.size, k, q, offsets, exclude)

    def batch_query_offset(self, k, vectors, offsets, exclude=None):
        """batch_query_offset_raw as Results: `distances` holds the keys t, ascending; flags is 0 (the order (t, row) is
        total)."""
        from .csls import as_results
        return as_results(*self.batch_query_offset_raw(k, vectors, offsets, exclude))

    def batch_query_rank_raw(self, vectors, gold, offsets=None, exclude=None):
        raise NotImplementedError("rank queries are not supported by a grouped index")

    def close(self):
        if self._h is not None and self._h.value:
            N.lib().gulon_grouped_index_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def grouped(grouped_vectors: GroupedVectors, residuals_quantizer: ProductQuantizer, strategy, metric="l2"):
    """Index.grouped (Index.scala:133-147): encode the residuals, wrap."""
    encoded = residuals_quantizer.encode(grouped_vectors.residuals)
    return GroupedIndex(residuals_quantizer, encoded, grouped_vectors.centroids, grouped_vectors.offsets, strategy,
                        metric)
