"""Tests (Tests.scala) and SummaryStats (MathUtils.scala:5-60): the recall of an index against exact neighbours, for
several k from ONE index query per sampled vector.

The word vectors stay on the device: the exact k-th distances come from gulon_exact_knn, the per-batch evaluation
(gather the returned rows, exact distances, hits per k) is gulon_recall_counts (csrc/recall.hip).  The host keeps what
is per query or per k: the cutoffs (double arithmetic), word -> row through the vectors' KeyIndexSorted, and the
SummaryStats fold, in query order.  `recall.py` (one k, eps = 0, for bench.py --full) is not touched by this."""
from dataclasses import dataclass

import numpy as np

from . import native as N
from .recall import sample_rows
from .word_index import BATCH

DEFAULT_KS = (1, 2, 3, 5, 10, 25, 50, 100, 500, 1000)          # Tests.defaultKs (Tests.scala:53)

_F = np.float32


@dataclass(frozen=True)
class SummaryStats:
    """SummaryStats(count, mean, s) (MathUtils.scala:5-24); mean and s are binary32, every operation rounds to it."""
    count: int = 0
    mean: np.float32 = _F(0)
    s: np.float32 = _F(0)

    @classmethod
    def of(cls, x):                                              # SummaryStats.apply(x: Float) (:27)
        return cls(1, _F(x), _F(0))

    @property
    def variance(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            return _F(self.s) / _F(self.count)

    @property
    def std_dev(self):
        """(float) sqrt((double)(s / count)); NaN for count = 0 (0f / 0), as on the JVM."""
        with np.errstate(invalid="ignore"):
            return _F(np.sqrt(np.float64(self.variance)))

    def combine(self, that):
        """`++` (MathUtils.scala:9-20), the operations in the reference's order."""
        if that.count == 0:
            return self
        if self.count == 0:
            return that
        n = self.count + that.count
        d = _F(_F(self.mean) - _F(that.mean))
        with np.errstate(over="ignore", invalid="ignore"):
            mean = _F(self.mean + _F(_F(_F(that.count) / _F(n)) * _F(that.mean - self.mean)))
            s = _F(_F(self.s + that.s) + _F(_F(_F(_F(d * d) * _F(self.count)) * _F(that.count)) / _F(n)))
        return SummaryStats(n, mean, s)


def fold(values):
    """Monoid.combineAll over SummaryStats(x), left to right (Tests.scala:41): the result depends on the order."""
    out = SummaryStats()
    for x in values:
        out = out.combine(SummaryStats.of(x))
    return out


def cutoff(max_distance_sq, eps):
    """Tests.scala:33-35 for arrays of float32 k-th distances; eps a float32.  eps = 0: the distance itself; otherwise
    ((double) sqrt(distance) * (double) (1f + eps))^2 rounded to float -- `1f + eps` is a FLOAT sum, the square is the
    correctly rounded double product."""
    v = np.asarray(max_distance_sq, np.float32)
    eps = _F(eps)
    if eps == 0:
        return v.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.sqrt(v.astype(np.float64)) * np.float64(_F(_F(1) + eps))
        return (r * r).astype(np.float32)


class Recall(dict):
    """{k: SummaryStats}, plus what the tie note of DESIGN.md 9f asks for: `flagged` = the queries whose index result
    carried a tie flag without the exact replay (their order among equal distances is (distance, row id), not the
    reference heap's, so a count of theirs can differ from the JVM's by one where the tie straddles a k)."""
    flagged = 0
    flagged_queries = ()


def recall_counts(matrix, queries, rows, ks, cutoffs, distances=False):
    """gulon_recall_counts: -> tp [B][len(ks)] int32 (and the [B][max_k] exact distances with distances=True)."""
    q = N.f32(queries)
    rows = N.i32(rows)
    b, max_k = rows.shape
    ks = N.i32(ks).reshape(-1)
    cut = N.f32(cutoffs).reshape(b, len(ks))
    tp = np.zeros((b, len(ks)), np.int32)
    dist = np.zeros((b, max_k), np.float32) if distances else None
    one_f, one_i = np.zeros(1, np.float32), np.zeros(1, np.int32)
    N.check(N.lib().gulon_recall_counts(matrix._h, q.reshape(-1) if q.size else one_f, b,
                                        rows.reshape(-1) if rows.size else one_i, max_k, ks if ks.size else one_i,
                                        len(ks), cut.reshape(-1) if cut.size else one_f,
                                        tp.reshape(-1) if tp.size else one_i,
                                        dist.ctypes.data if distances and dist.size else None))
    return (tp, dist) if distances else tp


class Tests:
    """Tests(wordVectors, queries) (Tests.scala:11-12).  word_vectors: DeviceWordVectors with a key index (.sorted());
    queries [B][d]; ks ascending; kth[q][j] = exact distance of the ks[j]-th neighbour of query q, valid for
    j < kept[q] (the k <= result length, Tests.scala:93-95)."""
    __test__ = False                    # a product class: pytest must not collect it where a test module imports it

    def __init__(self, word_vectors, queries, ks, kth, kept):
        self.word_vectors, self.queries, self.ks, self.kth, self.kept = word_vectors, queries, tuple(ks), kth, kept

    @classmethod
    def sample(cls, word_vectors, sample_size=1000, ks=DEFAULT_KS, seed=0):
        """Tests.sample (Tests.scala:76-87): sample_size draws of java.util.Random(seed).nextInt(size); the drawn rows
        are the queries, duplicates included."""
        if word_vectors.size <= 0:
            raise ValueError("bound must be positive")                       # Random.nextInt(0)
        rows = sample_rows(word_vectors.size, sample_size, seed)
        return cls.for_queries(word_vectors, word_vectors.matrix.get_rows(rows), ks)

    @classmethod
    def for_queries(cls, word_vectors, queries, ks=DEFAULT_KS):
        """Tests.forQueries (Tests.scala:89-107): exact neighbours at max(ks), the k-th distance for every k kept."""
        ks = sorted(set(int(k) for k in ks))
        if not ks or ks[0] < 1:
            raise ValueError("ks must be positive")
        matrix = word_vectors.matrix
        q = N.f32(queries).reshape(-1, matrix.cols)
        b, kmax = len(q), ks[-1]
        kth = np.full((b, len(ks)), np.nan, np.float32)
        kept = np.zeros(b, np.int64)
        at = np.asarray(ks) - 1
        for s in range(0, b, BATCH):
            part = q[s:s + BATCH]
            n = len(part)
            oi, od = np.zeros((n, kmax), np.int32), np.zeros((n, kmax), np.float32)
            oc, of = np.zeros(n, np.int32), np.zeros(n, np.int32)
            N.check(N.lib().gulon_exact_knn(matrix._h, 0, matrix.rows, part.reshape(-1), n, kmax, oi.reshape(-1),
                                            od.reshape(-1), oc, of))
            have = at[None, :] < oc[:, None]
            kth[s:s + n] = np.where(have, od[:, at], np.float32(np.nan))
            kept[s:s + n] = have.sum(axis=1)
        return cls(word_vectors, q, ks, kth, kept)

    def results(self, i):
        """Tests.Query.results of query i: [(k, distance of the k-th exact neighbour)]."""
        return [(self.ks[j], self.kth[i, j]) for j in range(int(self.kept[i]))]

    def _vector_rows(self, index, rows, row_map):
        """The rows of the WORD VECTORS behind an index's result rows (wordVectors.keyIndex.lookup(word).get,
        Tests.scala:27): each index row is resolved once, through the vectors' key index; negative rows stay."""
        valid = rows >= 0
        fresh = np.unique(rows[valid])
        fresh = fresh[row_map[fresh] == -2]
        lookup = self.word_vectors.key_index.lookup
        for r in fresh.tolist():
            v = lookup(index.words[r])
            if v is None:
                raise LookupError(f"the index holds the word {index.words[r]!r}, the word vectors do not")
            row_map[r] = v
        return np.where(valid, row_map[np.where(valid, rows, 0)], -1).astype(np.int32)

    def recall_of(self, index, eps=0.0, evaluate=recall_counts):
        """Tests.recallOf (Tests.scala:18-41).  index: a WordIndex.  Per query ONE index query at the largest k it
        kept; tp(k) = the entries among the first k whose exact distance to the query is <= cutoff(k); the sample
        tp.toFloat / k goes into SummaryStats, folded in query order.  -> Recall ({k: SummaryStats}, .flagged)."""
        cut = cutoff(self.kth, eps)
        ks = np.asarray(self.ks, np.int32)
        b = len(self.queries)
        tp = np.zeros((b, len(ks)), np.int32)
        row_map = np.full(index.size, -2, np.int64)
        flagged = []
        for nk in sorted(set(self.kept.tolist()) - {0}):
            group = np.flatnonzero(self.kept == nk)
            max_k = int(ks[nk - 1])
            for s in range(0, len(group), BATCH):
                part = group[s:s + BATCH]
                rows, _, counts, flags = index.batch_query_raw(max_k, self.queries[part])
                tied = (flags & (N.FLAG_BOUNDARY_TIE | N.FLAG_INTERIOR_TIE)) != 0
                flagged.extend(part[tied & ((flags & N.FLAG_EXACT_REPLAY) == 0)].tolist())
                vrows = self._vector_rows(index, rows, row_map)
                tp[part, :nk] = evaluate(self.word_vectors.matrix, self.queries[part], vrows, ks[:nk], cut[part, :nk])
        out = Recall()
        for j, k in enumerate(self.ks):
            sel = self.kept > j
            if sel.any():
                out[k] = fold(tp[sel, j].astype(np.float32) / _F(k))
        out.flagged, out.flagged_queries = len(flagged), tuple(sorted(flagged))
        return out


def java_float_to_string(x):
    """java.lang.Float.toString of a binary32: the shortest decimal that lies inside the value's rounding interval
    (the closest of that length), at least one fraction digit, plain notation for 1e-3 <= |x| < 1e7 and
    `d.dddE-n` outside it.  The interval is half an ulp to either side; for a normal power of two, whose lower
    neighbour is half as far, the JDK takes the narrower quarter ulp on BOTH sides (Float.MIN_NORMAL prints as
    1.17549435E-38 although 1.1754944E-38 would read back).  Never fewer than two digits (1.4E-45, not 1.0E-45)."""
    from fractions import Fraction
    f = _F(x)
    if f != f:
        return "NaN"
    bits = int(f.view(np.uint32))
    sign = "-" if bits >> 31 else ""
    expo, frac = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    if expo == 0xFF:
        return sign + "Infinity"
    if expo == 0 and frac == 0:
        return sign + "0.0"
    e2 = (expo if expo else 1) - 150                            # value = mant * 2^e2
    mant = frac | (0x800000 if expo else 0)
    value = Fraction(mant) * Fraction(2) ** e2
    power_of_two = frac == 0 and expo > 0
    half = Fraction(2) ** e2 / (4 if power_of_two else 2)
    e10 = len(str(value.numerator)) - len(str(value.denominator))   # an estimate of floor(log10(value)), refined below
    while Fraction(10) ** e10 > value:
        e10 -= 1
    while Fraction(10) ** (e10 + 1) <= value:
        e10 += 1
    for n in range(2, 10):                                      # two digits at least: Float.MIN_VALUE is 1.4E-45
        scale = Fraction(10) ** (e10 - n + 1)
        digits, rest = divmod(value / scale, 1)                 # the closest n-digit decimal, a tie to the even digit
        digits = int(digits) + (rest > Fraction(1, 2) or (rest == Fraction(1, 2) and int(digits) % 2 == 1))
        off = abs(digits * scale - value)
        # a decimal exactly half an ulp away reads back as the value when the significand is even (ties to even)
        if off < half or (off == half and mant % 2 == 0 and not power_of_two) or n == 9:
            break
    text, exp = str(digits), e10
    if len(text) > n:                                           # 9.99.. rounded up to 10.0..
        text, exp = text[:-1], exp + 1
    text = text.rstrip("0") or "0"
    if -3 <= exp < 7:
        if exp >= 0:
            whole, rest = text[:exp + 1].ljust(exp + 1, "0"), text[exp + 1:]
        else:
            whole, rest = "0", "0" * (-exp - 1) + text
        return f"{sign}{whole}.{rest or '0'}"
    return f"{sign}{text[0]}.{text[1:] or '0'}E{exp}"
