"""Named input regimes for the parity tests: data at the edges of the float32 range and queries with tight bounds.

Every GPU result is claimed to equal the CPU oracle bit for bit whatever the data; the kernels that skip work (the
8-bit lower-bound filters, the MFMA k-means filter, the grouped index's pre-selection) rest on RELATIVE error bounds
plus a few hand-written guards for where a relative bound stops holding.  A regime is a seeded generator of float32
inputs that reaches one of those places, and a CPU-side predicate that states what the inputs must exhibit -- checked
without a GPU in test_oracle_cross.py, at every shape the GPU tests use.  Nothing here looks at a GPU result: the
exponents of `large` (query and build path) and of the build path's `partial_inf` are found from the oracle alone; the
query path's `partial_inf` uses fixed magnitudes (2^20, 2^62.6, 2^70) that its predicate validates against the oracle.

Query path:  query_case(oracle, regime, n, d, m, k, B, seed) -> (cents [k*d], idx [m][n], Q [B][d])
Build path:  build_case(oracle, regime, n, d, frm, s, k, seed) -> X [n][d]
"""
import numpy as np

from oracle import py_oracle as po

QUERY_REGIMES = ("subnormal", "straddle", "large", "partial_inf", "mixed", "mixed_mild", "offset", "degenerate", "tight")
BUILD_REGIMES = QUERY_REGIMES[:-1]
FINITE_REGIMES = tuple(r for r in QUERY_REGIMES if r != "partial_inf")

TINY = np.float32(2.0 ** -126)          # the smallest normal float32
F32_MAX = float(np.finfo(np.float32).max)

# ---- the shapes of the GPU tests (test_gpu_value_regimes.py); the CPU predicate test walks the same lists -------------
# name: (n, d, m, k)
BYTE_FORMS = {
    "m16": (40000, 64, 16, 256),        # the ordered copy, one 16-byte word
    "m8": (40000, 32, 8, 256),          # two 4-byte words
    "m25": (30000, 100, 25, 256),       # seven 4-byte words, ragged
    "m32": (30000, 64, 32, 256),        # two 16-byte words
    "m36": (20000, 72, 36, 256),        # the widest 16-queries-per-entry table
    "m64": (24000, 128, 64, 256),       # 8 queries per entry
    "m100": (20000, 200, 100, 256),     # 4 queries per entry
    "k5": (20000, 12, 4, 5),            # width-4 codes
}
WIDE_FORMS = {
    "w1024": (30000, 64, 16, 1024),     # 10-bit codes
    "w4096": (30000, 32, 8, 4096),      # 12-bit codes
    "w5000": (20000, 24, 12, 5000),     # 16-bit codes, the table gathered from memory
    "w16384": (20000, 16, 8, 16384),    # sliced tables
}
FORMS = {**BYTE_FORMS, **WIDE_FORMS}
QUERY_B = 40
QUERY_KS = (1, 10, 63)

# `tight` with the library's own thresholds: (n, d, m, k)
PRODUCTION_FORMS = {
    "m16": (600000, 64, 16, 256), "m8": (600000, 32, 8, 256), "m25": (600000, 50, 25, 256),
    "m32": (600000, 64, 32, 256), "m64": (600000, 128, 64, 256), "m100": (600000, 200, 100, 256),
    "w1024": (420000, 32, 8, 1024),
}
PRODUCTION_B, PRODUCTION_K = 24, 10
PRODUCTION_PER = 400                    # rows per cluster there: the sample and the first stages (2 % + 8 % of the rows) must
                                        # meet K + 1 rows of a query's cluster for the main stage to start from a tight tau

# tie replay under `tight`: (n, d, m, k, K, B)
TIE_FORMS = {"m16": (260000, 64, 16, 256, 5, 70), "m8": (300000, 32, 8, 256, 10, 100), "m40": (200000, 80, 40, 256, 10, 64)}

# build path, n = 30 000 (parAssign restarts its random stream once): name: (d, frm, s, k)
BUILD_N = 30000
BUILD_FORMS = {
    "fp32_s4": (6, 1, 4, 16),           # resident fp32 MFMA
    "bf16_s8": (10, 1, 8, 256),         # bf16 split, 3 compact words
    "bf16_s10": (12, 1, 10, 256),       # 4 compact words
    "bf16_s13": (16, 2, 13, 256),       # 5 compact words
    "bf16_s14": (16, 1, 14, 256),       # three pieces, one instruction per product
    "stream_s33": (40, 4, 33, 70),      # streaming kernel
    "stream_s128": (128, 0, 128, 300),  # coarse clustering shape
    "fallback_s130": (140, 3, 130, 5),  # no MFMA
}
PQ_BUILD = (30000, 40, 4, 64)           # n, d, m, k
KNN_SHAPE = (30000, 24)                 # exact kNN: n, d
KNN_TIGHT_MK = (6, 256)                 # ... its `tight` rows are the decoded rows of a clustered (m, k) index

# grouped index: (n, d, groups, m, k, limit, K)
GROUPED_REGIMES = ("subnormal", "large", "mixed_mild", "offset")
GROUPED_PATHS = {
    "by_group": (60000, 24, 300, 8, 64, 90, 10),
    "literal": (20000, 24, 40, 8, 64, 12, 100),
    "wide": (12000, 16, 12, 4, 300, 5, 10),
}


def same_bits(a, b, nan_by_position=False):
    """float32 arrays equal bit for bit; nan_by_position: NaNs only have to sit at the same places (their payloads are
    not part of the contract: a JVM canonicalises them)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    if nan_by_position:
        assert np.array_equal(np.isnan(a), np.isnan(b))
        ok = ~np.isnan(a)
        a, b = a[ok], b[ok]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def sub_range(n):
    """A [from, until) that cuts row blocks (64) and ordering windows (256) at both ends."""
    return n // 7 + 37, n - n // 5 - 11


def _seed(regime, *shape):
    return [QUERY_REGIMES.index(regime) + 1, *[int(v) for v in shape]]


def _pow2(e):
    return np.float32(2.0 ** e)


def _sub_scales(d, m, lo, hi):
    """per-dimension scale: the dimensions of quantizer j get 2^(lo + (hi - lo) j / (m - 1))"""
    sc = np.ones(d, np.float32)
    for j, (f, u) in enumerate(po.subvectors(d, m)):
        sc[f:u] = _pow2(lo + (hi - lo) * j / max(m - 1, 1))
    return sc


def cents_as_rows(cents, d, m, k):
    """flat code book -> [k][d]: row c holds centroid c of every quantizer"""
    out = np.empty((k, d), np.float32)
    for f, u in po.subvectors(d, m):
        out[:, f:u] = cents[k * f: k * u].reshape(k, u - f)
    return out


def rows_as_cents(rows, d, m, k):
    out = np.empty(k * d, np.float32)
    for f, u in po.subvectors(d, m):
        out[k * f: k * u] = rows[:, f:u].reshape(-1)
    return out


def decode(cents, idx, d, m, k):
    """idx [m][r] -> the r decoded vectors"""
    cr = cents_as_rows(cents, d, m, k)
    out = np.empty((idx.shape[1], d), np.float32)
    for j, (f, u) in enumerate(po.subvectors(d, m)):
        out[:, f:u] = cr[idx[j], f:u]
    return out


def tight_noise(d, m, k):
    """the queries of `tight` are a decoded row + N(0, noise^2): a twentieth of the typical spacing of the k/4 centroid
    families in a sub-vector's dimensions, so that the row's own family stays the nearest in every quantizer"""
    return 0.05 * (k / 4.0 + 1.0) ** (-1.0 / max(1, d // m))


def sibling_centroids(rng, c0, d, m, k):
    """The code book of `tight`: the centroids of every quantizer come in families of four siblings, c, c + t, c + 2 t,
    c + 3 t, where t moves ONE coordinate by d * noise * 2^-23.  For a query at distance ~ noise per dimension
    from a row, swapping a code for a sibling moves that row's distance (~ d * noise^2) by
    2 t * noise ~ 2^-22 of it: a few units in the last place."""
    cr = c0[(np.arange(k) // 4) * 4].copy()
    step = np.float32(d * tight_noise(d, m, k) * 2.0 ** -23)
    for f, u in po.subvectors(d, m):
        coord = f + rng.integers(0, u - f, k // 4 + 1)[np.arange(k) // 4]
        # (the moved coordinate is kept small enough for t to be several of ITS units in the last place)
        cr[np.arange(k), coord] *= np.float32(min(1.0, d * tight_noise(d, m, k)))
        cr[np.arange(k), coord] += (np.arange(k) % 4).astype(np.float32) * step
    return cr


def clustered_codes(rng, n, m, k, per=50):
    """Codes of the `tight` regime: each row copies the codes of one of ~n/per base rows and re-draws one or two of its
    m quantizers -- to a sibling of the code it replaces (sibling_centroids), so the rows of a cluster are a few units in
    the last place apart for a query next to them, and since a cluster has few distinct variants, some of its rows are
    equal: exact ties."""
    nbase = max(1, n // per)
    base = rng.integers(0, k, (m, nbase)).astype(np.int32)
    idx = base[:, rng.integers(0, nbase, n)]
    nredraw = rng.integers(1, 3, n)
    first = rng.integers(0, m, n)
    second = (first + rng.integers(1, max(m, 2), n)) % m
    pick = rng.integers(1, 4, (2, n))
    rows = np.arange(n)
    for j in range(m):
        a = rows[first == j]
        idx[j, a] = np.minimum(idx[j, a] // 4 * 4 + (idx[j, a] + pick[0, a]) % 4, k - 1)
        b = rows[(second == j) & (nredraw == 2) & (second != first)]
        idx[j, b] = np.minimum(idx[j, b] // 4 * 4 + (idx[j, b] + pick[1, b]) % 4, k - 1)
    return np.ascontiguousarray(idx)


def _table_top(oracle, cents, d, m, k, Q):
    """the oracle's largest possible distance over the queries: the float32 sum, in quantizer order, of each table's
    largest entry (rounding is monotone, so no row's distance exceeds it and a row with those codes reaches it)"""
    T = oracle.prepare_query(cents, d, m, k, Q)
    top = np.zeros(len(Q), np.float32)
    with np.errstate(over="ignore"):
        for j in range(m):
            top = (top + T[:, j, :].max(axis=1)).astype(np.float32)
    return float(top.max()), T


def query_case(oracle, regime, n, d, m, k, B, seed=0, per=50):
    """(cents, idx, Q) of one regime at one index shape"""
    rng = np.random.default_rng(_seed(regime, n, d, m, k, B, seed))
    c0 = rng.standard_normal((k, d)).astype(np.float32)           # centroid c of every quantizer, as a row
    q0 = rng.standard_normal((B, d)).astype(np.float32)
    idx = None
    if regime == "subnormal":
        cr, Q = c0 * _pow2(-70), q0 * _pow2(-70)
    elif regime == "straddle":
        cr, Q = c0 * _pow2(-64), q0 * _pow2(-64)
    elif regime == "large":
        e = 60
        while True:                                               # lowered until the oracle's largest distance is finite
            cr, Q = c0 * _pow2(e), q0 * _pow2(e)
            top, _ = _table_top(oracle, rows_as_cents(cr, d, m, k), d, m, k, Q)
            if np.isfinite(top):
                break
            e -= 1
    elif regime == "partial_inf":
        # Three classes of centroids -- A: small; B: +2^62.6 in every coordinate (finite against a small query, +inf
        # against a query at -2^62.6); C: 2^70 (+inf against everything) -- three kinds of rows -- 6 with A codes only,
        # 34 with A codes and a B code in quantizer 0, the rest with at least one C code -- and three kinds of queries:
        # small ones (40 rows at a finite distance), ones whose first sub-vector sits at -2^62.6 (6 rows) and huge ones
        # (none).  So for K + 1 = 2, 11, 64 a query's nearest are all finite, all +inf, or finite ones followed by +inf.
        ka, kb = max(1, k // 4), max(2, k // 2)
        big = _pow2(62.6)
        cr = c0 * _pow2(20)
        cr[ka:kb] = big * (1.0 + 0.1 * rng.random((kb - ka, d))).astype(np.float32)
        cr[kb:] = _pow2(70) * np.sign(c0[kb:]) * (1.0 + 0.1 * rng.random((k - kb, d))).astype(np.float32)
        idx = rng.integers(0, k, (m, n)).astype(np.int32)
        rows = np.arange(n)
        idx[rows % m, rows] = rng.integers(kb, k, n)               # every ordinary row holds a C code
        lo_, hi_ = sub_range(n)
        fin = np.sort(rng.permutation(np.arange(lo_, hi_))[:28])   # 28 finite rows inside the sub-range, 12 outside
        fin = np.concatenate([fin, rng.permutation(lo_)[:6], hi_ + rng.permutation(n - hi_)[:6]])
        idx[:, fin] = rng.integers(0, ka, (m, len(fin)))
        idx[0, fin[4:-2]] = rng.integers(ka, kb, len(fin) - 6)     # all but 4 + 2 of them: a B code in quantizer 0
        Q = q0 * _pow2(20)
        f, u = po.subvectors(d, m)[0]
        Q[1::3, f:u] = -big * (1.0 + 0.1 * rng.random((len(Q[1::3]), u - f))).astype(np.float32)
        Q[2::3] = q0[2::3] * _pow2(70)
    elif regime in ("mixed", "mixed_mild"):
        sc = _sub_scales(d, m, -40, 40) if regime == "mixed" else _sub_scales(d, m, -8, 8)
        cr, Q = c0 * sc, q0 * sc
    elif regime == "offset":
        cr = (1000.0 + 0.01 * c0).astype(np.float32)
        Q = (1000.0 + 0.01 * q0).astype(np.float32)
    elif regime == "degenerate":
        cr, Q = c0.copy(), q0.copy()
        sub = po.subvectors(d, m)
        f, u = sub[0]
        cr[:, f:u] = cr[0, f:u]                                   # all-equal centroids: a constant table
        f, u = sub[1 % m]
        cr[:, f:u] = 0.0                                          # an all-zero quantizer
        f, u = sub[2 % m]
        cr[:, f:u][rng.random((k, u - f)) < 0.3] = -0.0
        f, u = sub[m - 1]
        if m > 4:
            cr[:, f:u] = cr[k - 1, f:u]
        idx = rng.integers(0, k, (m, n)).astype(np.int32)
        Q[0] = 0.0                                                # a zero query
        Q[1] = decode(rows_as_cents(cr, d, m, k), idx[:, 5:6], d, m, k)[0]    # a centroid combination that is a row
        Q[2] = -0.0
        Q[3] = decode(rows_as_cents(cr, d, m, k), rng.integers(0, k, (m, 1)).astype(np.int32), d, m, k)[0]
        Q[4, : d // 2] = 0.0
    elif regime == "tight":
        cr = sibling_centroids(rng, c0, d, m, k)
        cents = rows_as_cents(cr, d, m, k)
        idx = clustered_codes(rng, n, m, k, per)
        rows = rng.integers(0, n, B)
        Q = (decode(cents, idx[:, rows], d, m, k) + rng.standard_normal((B, d)) * tight_noise(d, m, k)).astype(np.float32)
    else:
        raise KeyError(regime)
    if idx is None:
        idx = rng.integers(0, k, (m, n)).astype(np.int32)
    return rows_as_cents(np.ascontiguousarray(cr, np.float32), d, m, k), idx, np.ascontiguousarray(Q, np.float32)


def _sample_distances(T, idx, rng, rows=2000):
    """[B][rows]: the float32 ADC distances of a sample of rows (quantizer order, as Index.scala sums them)"""
    pick = rng.integers(0, idx.shape[1], rows)
    acc = np.zeros((T.shape[0], rows), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(T.shape[1]):
            acc = (acc + T[:, j, idx[j, pick]]).astype(np.float32)
    return acc


def query_predicate(oracle, regime, cents, idx, Q, d, m, k, K=10):
    """Asserts what the regime must exhibit at this shape; returns the figures it looked at."""
    top, T = _table_top(oracle, cents, d, m, k, Q)
    live = T[np.isfinite(T) & (T != 0)]
    out = {"top": top}
    if regime == "subnormal":
        out["subnormal_share"] = share = float((live < TINY).mean())
        assert share > 0.9, out
    elif regime == "straddle":
        cr = cents_as_rows(cents, d, m, k)
        with np.errstate(under="ignore"):
            sq = np.square((Q[:, None, :] - cr[None, :64, :]).astype(np.float32)).astype(np.float32)
        out["squares_below"] = below = float((sq < TINY).mean())
        assert 0.05 < below < 0.95, out
    elif regime == "large":
        assert np.isfinite(top) and top > 2.0 ** 120, out
        assert np.isfinite(T).all()
    elif regime == "partial_inf":
        out["inf_share"] = share = float(np.isinf(T).mean())
        assert 0.1 <= share <= 0.9, out
        assert not np.isnan(T).any()
        # finite and infinite distances in one query: at K = 1, 10, 63 some queries have K + 1 finite nearest, some none,
        # and (from K = 10 on) some a finite head with +inf behind it -- over the full range and the sub-range
        for frm, until in ((0, idx.shape[1]), sub_range(idx.shape[1])):
            for Kq in QUERY_KS:
                kd = oracle.pq_batch_query(idx, d, k, cents, Q, Kq + 1, frm, until)[1]
                nfin = np.isfinite(kd).sum(axis=1)
                out[f"finite/mixed/inf K={Kq} from {frm}"] = split = (int((nfin == Kq + 1).sum()),
                                                                   int(((nfin > 0) & (nfin <= Kq)).sum()), int((nfin == 0).sum()))
                assert split[2] > 0 and split[0] + split[1] > 0, out
                assert split[0] > 0 if Kq == 1 else split[1] > 0, out
    elif regime == "mixed":
        # one quantizer dominates: its typical entry is beyond 2^24 times everything the first half can add up to
        small = T[:, : m // 2, :].max(axis=2).astype(np.float64).sum(axis=1)
        big = np.median(T[:, m - 1, :], axis=1).astype(np.float64)
        out["dominance"] = float((big / small).min())
        assert (big > 2.0 ** 24 * small).all(), out
        assert np.isfinite(T).all() and (live >= TINY).all()
    elif regime == "mixed_mild":
        med = np.median(T, axis=2).astype(np.float64)
        out["spread"] = spread = float((med[:, m - 1] / med[:, 0]).min())
        assert 2.0 ** 16 < spread < 2.0 ** 48, out
        assert np.isfinite(T).all() and (live >= TINY).all()
    elif regime == "offset":
        # cancellation: a distance is below one ulp of the squared norms it would be the difference of
        q2 = np.stack([np.square(Q[:, f:u].astype(np.float64)).sum(axis=1) for f, u in po.subvectors(d, m)], axis=1)
        out["distance_over_norm"] = r = float((T.max(axis=2) / q2).max())
        assert r < 2.0 ** -24, out
    elif regime == "degenerate":
        assert (T[:, 0, :] == T[:, 0, :1]).all()                       # a constant table for every query
        mins = T.min(axis=2).astype(np.float64).sum(axis=1)
        assert mins[1] == 0.0 and mins[3] == 0.0                        # budget 0: the query is a centroid combination
        assert np.signbit(cents[cents == 0]).any() and np.signbit(Q[2]).all()
        assert not Q[0].any()
    elif regime == "tight":
        oi, od, oc = oracle.pq_batch_query(idx, d, k, cents, Q, K)
        med = np.median(_sample_distances(T, idx, np.random.default_rng(1)), axis=1)
        out["kth_over_median"] = r = float((od[:, K - 1] / med).max())
        assert r < 1.0 / 20.0, out
        # tight around tau: the distinct distances next to the K-th one are a few units in the last place apart, and the
        # budget (tau - sum of the table minima) is a few 1e-6 of tau -- what tau' = tau (1 + 2 m_pad u) has to cover
        wide_od = oracle.pq_batch_query(idx, d, k, cents, Q, K + 50)[1]
        near = np.zeros(len(Q), bool)
        for q in range(len(Q)):                      # the DISTINCT distances next to the K-th one (equal rows tie exactly)
            u = np.unique(wide_od[q])
            at = int(np.searchsorted(u, wide_od[q, K - 1]))
            gaps = np.diff(u[max(0, at - 1): at + 2]) / np.spacing(u[at])
            near[q] = ((gaps > 0) & (gaps <= 16)).any()
        out["queries_with_gaps_of_1_to_16_ulp"] = int(near.sum())
        assert near.sum() * 2 >= len(Q), out
        budget = (wide_od[:, K].astype(np.float64) - T.min(axis=2).astype(np.float64).sum(axis=1)) / wide_od[:, K]
        out["median_budget_over_tau"] = float(np.median(budget))
        # (1e-6 of tau is a whole level of the 8-bit tables once the budget is below 255e-6 of tau)
        assert np.median(budget) < 2.0 ** -12, out
    return out


# ---- build path ------------------------------------------------------------------------------------------------------
def _init_tables(oracle, X, frm, s, k, seed, rows=256):
    """squared distances (the oracle's chain) from the first `rows` rows to the oracle's initial centroids"""
    C0, _ = oracle.kmeans_init(X, frm, s, k, seed)
    with np.errstate(all="ignore"):
        return oracle.prepare_query(C0.reshape(-1), s, 1, k, np.ascontiguousarray(X[:rows, frm:frm + s]))[:, 0, :], C0


def build_case(oracle, regime, n, d, frm, s, k, seed=0, dup=False):
    """X [n][d] of one regime; k-means runs on its columns [frm, frm + s)"""
    rng = np.random.default_rng(_seed(regime, n, d, frm, s, k, seed))
    x0 = rng.standard_normal((n, d)).astype(np.float32)
    if regime == "subnormal":
        X = x0 * _pow2(-70)
    elif regime == "straddle":
        X = x0 * _pow2(-64)
    elif regime == "large":
        e = 60
        while True:                                   # every |x|^2 and every distance (<= 4 max |x|^2) stays finite
            X = x0 * _pow2(e)
            if 4.0 * np.square(X[:, frm:frm + s].astype(np.float64)).sum(axis=1).max() < 0.9 * F32_MAX:
                break
            e -= 1
    elif regime == "partial_inf":
        lo, hi = 56.0, 68.0
        for _ in range(24):
            e = 0.5 * (lo + hi)
            X = x0 * _pow2(e)
            share = float(np.isinf(_init_tables(oracle, X, frm, s, k, seed)[0]).mean())
            if 0.35 <= share <= 0.65:
                break
            lo, hi = (lo, e) if share > 0.5 else (e, hi)
    elif regime in ("mixed", "mixed_mild"):
        X = x0 * (_sub_scales(d, d, -40, 40) if regime == "mixed" else _sub_scales(d, d, -8, 8))
    elif regime == "offset":
        X = (1000.0 + 0.01 * x0).astype(np.float32)
    elif regime == "degenerate":
        X = x0.copy()
        X[rng.random((n, d)) < 0.1] = -0.0
        X[:100] = 0.0                                 # rows that are zero but for the constant column
        X[:, frm] = np.float32(0.75)                  # a constant column
        if s >= 3:
            X[:, frm + 1] = 0.0                       # a zero column
        dup = True
    else:
        raise KeyError(regime)
    X = np.ascontiguousarray(X, np.float32)
    if dup:                                           # duplicated rows => duplicate init centroids => tie draws
        X[n - n // 3:] = X[: n // 3]
    return X


def build_predicate(oracle, regime, X, frm, s, k, seed=0):
    T, C0 = _init_tables(oracle, X, frm, s, k, seed)
    live = T[np.isfinite(T) & (T != 0)]
    V = X[:, frm:frm + s].astype(np.float64)
    x2 = np.square(V).sum(axis=1)
    out = {}
    if regime == "subnormal":
        out["subnormal_share"] = share = float((live < TINY).mean())
        assert share > 0.9, out
    elif regime == "straddle":
        with np.errstate(under="ignore"):
            sq = np.square((X[:4096, None, frm:frm + s] - C0[None, :8, :]).astype(np.float32)).astype(np.float32)
        out["squares_below"] = below = float((sq[sq != 0] < TINY).mean())
        assert 0.05 < below < 0.95, out
    elif regime == "large":
        c2 = np.square(C0.astype(np.float64)).sum(axis=1).max()
        out["x2max"] = float(x2.max())
        assert np.isfinite(T).all() and 2.0 ** 120 < x2.max() and 4.0 * x2.max() < F32_MAX, out
        assert x2.max() * c2 > F32_MAX                                    # nx * cmax2 overflows
    elif regime == "partial_inf":
        out["inf_share"] = share = float(np.isinf(T).mean())
        assert 0.1 <= share <= 0.9, out
    elif regime == "mixed":
        col = np.abs(V).max(axis=0)
        out["column_spread"] = float(col.max() / col.min())
        assert col.max() > 2.0 ** 13 * col.min() and np.isfinite(T).all(), out
    elif regime == "mixed_mild":
        col = np.abs(V).max(axis=0)
        out["column_spread"] = spread = float(col.max() / col.min())
        assert 1.0 < spread < 2.0 ** 20 and np.isfinite(T).all(), out
    elif regime == "offset":
        out["distance_over_norm"] = r = float(T.max() / x2.min())
        assert r < 2.0 ** -24, out
    elif regime == "degenerate":
        assert (X[:, frm] == X[0, frm]).all() and not X[:100, frm + 1:].any()
        assert np.signbit(X[X == 0]).any()
        assert np.array_equal(X[len(X) - len(X) // 3:], X[: len(X) // 3])     # duplicated rows: ties between centroids
    return out
