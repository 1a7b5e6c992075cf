"""Index diagnostics: how an index's code books are used and how well its rows represent the vectors it was built from
(csrc/inspect.hip; DESIGN.md "Index diagnostics").

The device gives two things -- the code histogram H[j][c] and, against the original vectors, the per-row squared error
MathUtils.distanceSq(original, decoded) with its per-quantizer sums -- and IndexReport is plain host arithmetic on those
arrays.  reference_quality is the reference's own figure, ProductQuantizerSpec.quality
(ProductQuantizerSpec.scala:70-73)."""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from . import native as N


def code_histogram_raw(fn, handle, m, k, n, from_=0, until=None):
    """gulon_*_code_histogram -> int64 [m][k]."""
    until = n if until is None else until
    out = np.zeros((m, k), np.int64)
    N.check(fn(handle, int(from_), int(until), out.reshape(-1) if out.size else np.zeros(1, np.int64)))
    return out


def row_errors_raw(fn, handle, m, n, matrix, row_map=None, from_=0, until=None, norms=False):
    """gulon_*_row_errors -> (row_error [until - from_] float32, quantizer_error [m] float64[, row_norm_sq])."""
    from .matrix import as_device
    until = n if until is None else until
    rows = max(int(until) - int(from_), 0)
    dm = as_device(matrix)
    rmap = None if row_map is None else N.i32(row_map).reshape(-1)
    err = np.zeros(rows, np.float32)
    nrm = np.zeros(rows, np.float32) if norms else None
    qerr = np.zeros(max(m, 1), np.float64)
    one = np.zeros(1, np.int32)
    N.check(fn(handle, dm._h, None if rmap is None else (rmap if rmap.size else one).ctypes.data,
               0 if rmap is None else rmap.size, int(from_), int(until), err.ctypes.data if rows else None,
               nrm.ctypes.data if norms and rows else None, qerr))
    return (err, qerr[:m], nrm) if norms else (err, qerr[:m])


def reference_quality(row_error):
    """ProductQuantizerSpec.quality (ProductQuantizerSpec.scala:70-73): the sum over the rows of
    MathUtils.distanceSq(original, decoded), a binary32 sum taken left to right."""
    e = np.ascontiguousarray(row_error, np.float32).reshape(-1)
    return np.float32(np.cumsum(e, dtype=np.float32)[-1]) if e.size else np.float32(0)


def entropy_bits(counts):
    """The entropy of one quantizer's code usage, in bits (0 for an empty histogram)."""
    c = np.asarray(counts, np.float64)
    total = c.sum()
    if total <= 0:
        return 0.0
    p = c[c > 0] / total
    return float(-(p * np.log2(p)).sum())


def worst_rows(row_error, w):
    """The w rows with the largest error, largest first; equal errors in ascending row order."""
    e = np.asarray(row_error, np.float32)
    order = np.lexsort((np.arange(len(e)), -e.astype(np.float64)))
    return order[:max(int(w), 0)]


@dataclass
class IndexReport:
    n: int
    d: int
    m: int
    k: int
    metric: str
    form: str                                   # "sorted" | "grouped"
    groups: int = 0                             # grouped: the number of groups (empty ones included)
    group_size_min: Optional[int] = None
    group_size_median: Optional[float] = None
    group_size_max: Optional[int] = None
    centroids_used: List[int] = field(default_factory=list)       # per quantizer: codes with at least one row
    largest_share: List[float] = field(default_factory=list)      # per quantizer: the most used code's share of the rows
    entropy: List[float] = field(default_factory=list)            # per quantizer: bits (log2 k at most)
    # with vectors
    mean_row_error: Optional[float] = None
    relative_error: Optional[float] = None      # sum(row_error) / sum(row_norm_sq), float64
    quantizer_mean_error: Optional[List[float]] = None
    worst: Optional[List[Tuple[int, float, Optional[str]]]] = None   # (row, error, word or None), largest error first

    @classmethod
    def from_arrays(cls, d, metric, form, histogram, group_sizes=None, row_error=None, row_norm_sq=None,
                    quantizer_error=None, worst=10, words=None):
        """histogram: int [m][k] over all rows; group_sizes: rows per group of a grouped index; row_error / row_norm_sq
        [n] and quantizer_error [m] when the index was compared with its vectors; words: row -> word."""
        h = np.asarray(histogram, np.int64)
        m, k = h.shape
        n = int(h[0].sum()) if m else 0
        rep = cls(n, int(d), m, k, metric, form)
        rep.centroids_used = [int((row > 0).sum()) for row in h]
        rep.largest_share = [float(row.max() / row.sum()) if row.sum() else 0.0 for row in h]
        rep.entropy = [entropy_bits(row) for row in h]
        if group_sizes is not None:
            s = np.asarray(group_sizes, np.int64)
            rep.groups = len(s)
            if len(s):
                rep.group_size_min, rep.group_size_max = int(s.min()), int(s.max())
                rep.group_size_median = float(np.median(s))
        if row_error is not None:
            e = np.asarray(row_error, np.float32)
            total = float(e.astype(np.float64).sum())
            rep.mean_row_error = total / len(e) if len(e) else 0.0
            if row_norm_sq is not None:
                norm = float(np.asarray(row_norm_sq, np.float32).astype(np.float64).sum())
                rep.relative_error = total / norm if norm > 0 else float("nan")
            if quantizer_error is not None:
                rep.quantizer_mean_error = [float(q) / len(e) if len(e) else 0.0 for q in quantizer_error]
            rep.worst = [(int(r), float(e[r]), None if words is None else words[int(r)])
                         for r in worst_rows(e, worst)]
        return rep

    def lines(self):
        """The report as the `inspect` command prints it."""
        out = [f"index: {self.form}, metric {self.metric}, {self.n} rows, d = {self.d}, m = {self.m}, k = {self.k}"]
        if self.form == "grouped":
            out.append(f"groups: {self.groups}, rows per group min {self.group_size_min} / median "
                       f"{self.group_size_median:g} / max {self.group_size_max}")
        full = np.log2(self.k) if self.k > 0 else 0.0
        for j in range(self.m):
            out.append(f"quantizer {j}: {self.centroids_used[j]} of {self.k} centroids used, largest share "
                       f"{self.largest_share[j]:.4f}, entropy {self.entropy[j]:.3f} of {full:.3f} bits")
        if self.mean_row_error is not None:
            out.append(f"mean row error: {self.mean_row_error:.6g}")
            if self.relative_error is not None:
                out.append(f"relative error: {self.relative_error:.6g}")
            if self.quantizer_mean_error is not None:
                for j, q in enumerate(self.quantizer_mean_error):
                    out.append(f"quantizer {j}: mean error {q:.6g}")
            for row, err, word in self.worst or []:
                out.append(f"worst: {word if word is not None else row} (row {row}): {err:.6g}")
        return out


def inspect_word_index(word_index, vectors=None, worst=10):
    """WordIndex.inspect: the report of a loaded index, against `vectors` (DeviceWordVectors with a key index, the
    normalised reading for a cosine index) when given."""
    from .refine import word_row_map
    index = word_index.index
    grouped = word_index._grouped
    sizes = None
    if grouped:
        sizes = np.diff(np.r_[0, np.asarray(index.offsets, np.int64), index.size])
    hist = index.code_histogram()
    if vectors is None:
        return IndexReport.from_arrays(index.dimension, index.metric, "grouped" if grouped else "sorted", hist, sizes)
    row_map = word_row_map(word_index, vectors)[:word_index.size]
    err, qerr, nrm = index.row_errors(vectors.matrix, row_map, norms=True)
    return IndexReport.from_arrays(index.dimension, index.metric, "grouped" if grouped else "sorted", hist, sizes, err,
                                   nrm, qerr, worst, word_index.words)
