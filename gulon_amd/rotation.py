"""Rotated indexes: an orthogonal rotation learned before quantizing (OPQ), applied once to the data and once to each
query (csrc/rotate.hip; DESIGN.md "Rotated indexes").  Not in the reference.

The quantizer cuts a vector into m runs of consecutive coordinates and spends the same log2 k bits on each.  A rotation R
(d x d, orthogonal) moves the variance to where those bits are: the index is built over X R, a query q is asked as q R,
and nothing downstream changes -- the inner index is an ordinary index over other numbers.  Distances between rotated
vectors are the distances between the originals up to binary32 rounding.

rotate: out[i][c] = sum_j x[i][j] * R[j][c], binary32, s = 0; j ascending: s = s + (x[i][j] * R[j][c]), unfused
(rotate_reference restates it in numpy).  R is kept in a side-car file beside the index file, as fine codes are: the
reference's protobuf has no field for it."""
import ctypes as C
import os
import struct

import numpy as np

from . import native as N

MAGIC, VERSION = b"GULONROT", 1


def rotate_reference(x, R, transpose=False):
    """The kernel's arithmetic in numpy float32: out[i][c] = sum_j x[i][j] * R[j][c] (transpose: R[c][j]), s = 0 and, j
    ascending, s = s + (x[i][j] * R[j][c]), product and sum each rounded to binary32.  For tests and documentation."""
    R = np.asarray(R, np.float32)
    d = R.shape[0]
    x = np.asarray(x, np.float32)
    rows = x.reshape(-1, d)
    if transpose:
        R = R.T
    s = np.zeros(rows.shape, np.float32)
    with np.errstate(all="ignore"):
        for j in range(d):
            s = s + rows[:, j:j + 1] * R[j][None, :]
    return s.reshape(x.shape)


def eigenvalue_allocation(eigenvalues, sizes):
    """Which column goes to which quantizer: the eigenvalues, largest first, are dealt one at a time to the bucket that
    is not yet full and has the smallest running sum of log eigenvalues (ties: the lowest bucket), so that the buckets'
    products of variances come out balanced.  sizes: the widths of the quantizers' coordinate runs (subvector_bounds;
    they may differ).  Non-positive eigenvalues count as the smallest positive double.  -> the column order, bucket 0's
    columns first: an int64 permutation of range(len(eigenvalues))."""
    w = np.asarray(eigenvalues, np.float64).reshape(-1)
    sizes = [int(s) for s in sizes]
    if sum(sizes) != w.size or any(s < 0 for s in sizes):
        raise ValueError(f"buckets of {sum(sizes)} columns for {w.size} eigenvalues")
    logs = np.log(np.maximum(w, np.nextafter(0.0, 1.0)))
    buckets, sums = [[] for _ in sizes], [0.0] * len(sizes)
    for i in np.argsort(-w, kind="stable").tolist():
        b = min((b for b in range(len(sizes)) if len(buckets[b]) < sizes[b]), key=lambda b: (sums[b], b))
        buckets[b].append(i)
        sums[b] += logs[i]
    return np.asarray([i for bucket in buckets for i in bucket], np.int64)


def procrustes(moment):
    """The orthogonal R that minimises |X R - Y| (Frobenius) given moment = X^T Y: U @ Vt of its SVD, in float64."""
    u, _, vt = np.linalg.svd(np.asarray(moment, np.float64))
    return u @ vt


def moment(a, b):
    """gulon_dataset_moment: out[p][q] = sum_r a[r][p] * b[r][q] in binary64, for two DeviceMatrix of equal rows.
    -> float64 [a.cols][b.cols]; the same bits on every call."""
    if a.rows != b.rows:
        raise ValueError(f"requirement failed: the moment of {a.rows} rows with {b.rows} rows")
    out = np.zeros((a.cols, b.cols), np.float64)
    N.check(N.lib().gulon_dataset_moment(a._h, b._h, out.reshape(-1)))
    return out


class Rotation:
    """A d x d float32 matrix R, applied as x R (apply) or x R^T (apply_transposed) on the device."""

    def __init__(self, matrix):
        m = np.array(matrix, np.float32, order="C")
        if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1:
            raise ValueError("a rotation is a square matrix of at least one row")
        self.matrix = m

    @classmethod
    def identity(cls, d):
        return cls(np.eye(d, dtype=np.float32))

    @property
    def dimension(self):
        return self.matrix.shape[0]

    def _rows(self, x, transpose):
        x = np.asarray(x, np.float32)
        if x.size % self.dimension or (x.ndim and x.shape[-1] != self.dimension):
            raise ValueError(f"vectors of dimension {x.shape[-1] if x.ndim else 1} for a rotation of dimension "
                             f"{self.dimension}")
        rows = np.ascontiguousarray(x).reshape(-1, self.dimension)
        out = np.zeros(rows.shape, np.float32)
        one = np.zeros(1, np.float32)
        N.check(N.lib().gulon_rotate_rows(rows.reshape(-1) if rows.size else one, rows.shape[0], self.dimension,
                                          self.matrix.reshape(-1), int(bool(transpose)),
                                          out.reshape(-1) if out.size else one))
        return out.reshape(x.shape)

    def apply(self, x):
        """x R for host vectors ([d] or [..., d]), on the device (gulon_rotate_rows)."""
        return self._rows(x, False)

    def apply_transposed(self, x):
        """x R^T: the way back, for an orthogonal R."""
        return self._rows(x, True)

    def apply_device(self, matrix, transpose=False):
        """A new DeviceMatrix = matrix R, without leaving HBM (gulon_dataset_rotate)."""
        from .matrix import DeviceMatrix
        if matrix.cols != self.dimension:
            raise ValueError(f"a matrix of dimension {matrix.cols} for a rotation of dimension {self.dimension}")
        h = C.c_void_p()
        N.check(N.lib().gulon_dataset_rotate(matrix._h, self.matrix.reshape(-1), int(bool(transpose)), C.byref(h)))
        return DeviceMatrix(h, matrix.rows, matrix.cols)

    def rotate_word_vectors(self, vectors):
        """DeviceWordVectors with the same words and key index and the rotated matrix."""
        from .word_vectors import DeviceWordVectors
        matrix = None if vectors.matrix is None else self.apply_device(vectors.matrix)
        return DeviceWordVectors(vectors.words, matrix, vectors.key_index, vectors.stats)

    def orthogonality_error(self):
        """max |R^T R - I|, in float64."""
        r = self.matrix.astype(np.float64)
        return float(np.abs(r.T @ r - np.eye(self.dimension)).max())

    def save(self, path):
        with open(os.fspath(path), "wb") as fh:
            fh.write(MAGIC + struct.pack("<II", VERSION, self.dimension))
            fh.write(self.matrix.astype("<f4").tobytes())

    @classmethod
    def load(cls, path):
        """ValueError for a wrong magic or version, a short or long file, a non-finite entry."""
        with open(os.fspath(path), "rb") as fh:
            buf = fh.read()
        if len(buf) < 16 or buf[:8] != MAGIC:
            raise ValueError(f"{path}: not a rotation file")
        version, d = struct.unpack("<II", buf[8:16])
        if version != VERSION:
            raise ValueError(f"{path}: rotation file of version {version}, expected {VERSION}")
        if d < 1 or len(buf) != 16 + 4 * d * d:
            raise ValueError(f"{path}: {len(buf) - 16} bytes of matrix for d = {d}")
        m = np.frombuffer(buf, "<f4", d * d, 16).reshape(d, d)
        if not np.isfinite(m).all():
            raise ValueError(f"{path}: the rotation has a non-finite entry")
        return cls(m)


def rotation_error(matrix, rotation, pq_config, decode=False):
    """What train_rotation minimises: rotate `matrix` (rotation None: taken as it is), train a quantizer on the result
    (ProductQuantizer.apply), encode it, and add up gulon_index_row_errors in float64.  -> the error, or with decode
    (error, the decoded rows as a DeviceMatrix the caller closes)."""
    from .index import PQIndex
    from .product_quantizer import Config, ProductQuantizer
    rotated = matrix if rotation is None else rotation.apply_device(matrix)
    index = None
    try:
        config = Config(pq_config.num_clusters, pq_config.num_quantizers, pq_config.max_iterations)
        pq = ProductQuantizer.apply(rotated, config)
        index = PQIndex(pq, pq.encode(rotated))
        error = float(index.row_errors(rotated)[0].astype(np.float64).sum())
        return (error, index.decode_matrix()) if decode else error
    finally:
        if index is not None:
            index.close()
        if rotation is not None:
            rotated.close()


def train_rotation(matrix, pq_config, rounds=4, write=None):
    """Learn a rotation for `matrix` (DeviceMatrix) and the quantizer shape of pq_config (product_quantizer.Config):
      1. C = moment(X, X); the eigenvectors of C, dealt to the quantizers by eigenvalue_allocation;
      2. for t = 0 .. rounds: E_t = rotation_error(X, float32(R)); unless t is the last, Y = the decoded rows and
         R = procrustes(moment(X, Y)) -- each round retrains the quantizer;
      3. E_id, the same for the matrix as it is;
      4. the candidate with the smallest error, the identity included: a rotation never makes the training matrix worse.
    -> (Rotation, {"identity": E_id, "rounds": [E_0 ...], "chosen": t or "identity"}).  write: the task log (None:
    silent).  ValueError for a matrix with a non-finite moment."""
    from .build import log_task
    from .vectors import subvector_bounds
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError("rounds must not be negative")
    d = matrix.cols
    fr, un = subvector_bounds(d, pq_config.num_quantizers)

    def initial():
        c = moment(matrix, matrix)
        if not np.isfinite(c).all():
            raise ValueError("the vectors have a non-finite second moment")
        w, v = np.linalg.eigh(c)
        return v[:, eigenvalue_allocation(w, (un - fr).tolist())]
    R = log_task(write, "Computing initial rotation", initial, "Computed initial rotation")
    candidates, errors = [], []
    for t in range(rounds + 1):
        rotation = Rotation(R.astype(np.float32))
        last = t == rounds

        def step():
            if last:
                return rotation_error(matrix, rotation, pq_config), None
            error, decoded = rotation_error(matrix, rotation, pq_config, decode=True)
            try:
                return error, procrustes(moment(matrix, decoded))
            finally:
                decoded.close()
        error, R_next = log_task(write, f"Rotation round {t}", step, lambda r: f"Rotation round {t}: error {r[0]:.6g}")
        candidates.append(rotation)
        errors.append(error)
        if not last:
            R = R_next
    identity = log_task(write, "Evaluating the identity", lambda: rotation_error(matrix, None, pq_config),
                        lambda e: f"Identity: error {e:.6g}")
    best = int(np.argmin(errors))
    history = {"identity": identity, "rounds": errors, "chosen": best}
    if not errors[best] < identity:
        history["chosen"] = "identity"
        return Rotation.identity(d), history
    return candidates[best], history


class RotatedWordIndex:
    """An index built over rotated vectors, asked in the original space: anything with WordIndex's query surface (a
    WordIndex, its restriction, its refined forms) behind a Rotation.  Query vectors are rotated first; lookup rotates
    back; queries by word and by expression go through unchanged -- the stored rows already live in the rotated space
    and composing is linear.  Word vectors handed in (refined, inspect, update) are rotated once on the device, and what
    comes back is wrapped again where it is an index.  Anything else (`words`, `size`, `metric`, `row_of`, `close`, the
    counters of `update` and `restrict` ...) is the inner index's."""

    def __init__(self, inner, rotation):
        if inner.dimension != rotation.dimension:
            raise ValueError(f"a rotation of dimension {rotation.dimension} for an index of dimension {inner.dimension}")
        self.inner, self.rotation = inner, rotation

    def __getattr__(self, name):                     # only what this class does not define
        if name in ("inner", "rotation"):
            raise AttributeError(name)
        return getattr(self.inner, name)

    @property
    def dimension(self):
        return self.inner.dimension

    def _rotated(self, vectors):
        q = np.ascontiguousarray(vectors, np.float32)
        if q.size % self.dimension:
            raise ValueError(f"query vectors of {q.size} numbers for an index of dimension {self.dimension}")
        return self.rotation.apply(q.reshape(-1, self.dimension))

    def _vectors(self, vectors):
        if vectors.dimension != self.dimension:
            raise ValueError(f"vectors of dimension {vectors.dimension} for an index of dimension {self.dimension}")
        return self.rotation.rotate_word_vectors(vectors)

    # ---- queries by vector: rotated first
    def batch_query(self, k, vectors, *args, **kwargs):
        return self.inner.batch_query(k, self._rotated(vectors), *args, **kwargs)

    def batch_query_raw(self, k, vectors, *args, **kwargs):
        return self.inner.batch_query_raw(k, self._rotated(vectors), *args, **kwargs)

    def query(self, k, vector, *args, **kwargs):
        return self.batch_query(k, np.asarray(vector, np.float32).reshape(1, -1), *args, **kwargs)[0]

    def lookup(self, word):
        v = self.inner.lookup(word)
        return None if v is None else self.rotation.apply_transposed(v)

    def batch_query_cosmul(self, k, expressions):
        raise NotImplementedError("cosmul queries are not supported by a rotated index")

    def query_cosmul(self, k, expression):
        raise NotImplementedError("cosmul queries are not supported by a rotated index")

    def batch_query_rank_raw(self, vectors, gold, offsets=None, exclude=None):
        raise NotImplementedError("rank queries are not supported by a rotated index")

    # ---- forms of the index that take word vectors or give an index back
    def refined(self, vectors, candidates):
        return RotatedWordIndex(self.inner.refined(self._vectors(vectors), candidates), self.rotation)

    def fine_refined(self, fine, candidates):
        fine = fine.inner if isinstance(fine, RotatedWordIndex) else fine        # the fine index lives in the rotated space
        return RotatedWordIndex(self.inner.fine_refined(fine, candidates), self.rotation)

    def restrict(self, words):
        return RotatedWordIndex(self.inner.restrict(words), self.rotation)

    def inspect(self, vectors=None, worst=10):
        if vectors is None:
            return self.inner.inspect(None, worst)
        rotated = self._vectors(vectors)
        try:
            return self.inner.inspect(rotated, worst)
        finally:
            rotated.matrix.close()

    def update(self, add=None, remove=None):
        if add is None or add.matrix is None:
            return RotatedWordIndex(self.inner.update(add=add, remove=remove), self.rotation)
        rotated = self._vectors(add)
        try:
            return RotatedWordIndex(self.inner.update(add=rotated, remove=remove), self.rotation)
        finally:
            rotated.matrix.close()
