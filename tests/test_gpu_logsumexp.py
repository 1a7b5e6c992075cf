"""The log-sum-exp scan of the exact index (csrc/logsumexp.hip, gulon_exact_index_query_logsumexp) against
softmax.logsumexp_reference -- numpy float64 with the exactly rounded sum -- over distances restated in numpy float32
one dimension at a time.  Where the range holds at most 8191 rows the restated distances are first checked bit for bit
against the handle's own ordinary query at K = the rows of the range.

terms must be equal.  L must lie within 2^-40 + 4 * spacing64(|L_ref|) of the reference (DESIGN.md 9af derives it: z is
the same IEEE product on both sides; what differs is exp and log, 1 ulp each, and the order of a sum of at most 2^20
positive terms), and be -inf exactly where the reference is."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import bits
from cosmul_ref import exact_distances

pytestmark = pytest.mark.gpu

EXACT_SUB_BATCH = 4096                       # table_scan.hpp
MAX_LIST = 8191                              # the deepest ordinary query of the exact index


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def rows_of(seed, n, d):
    """Rows whose squared distances are about 1: beta up to 100 keeps every term far above the underflow."""
    return (np.random.default_rng(seed).standard_normal((n, d)) * (0.7 / np.sqrt(d))).astype(np.float32)


def queries_of(seed, X, b, lo=0, hi=None):
    """b noisy copies of rows of X[lo:hi] and the rows they were made from."""
    rng = np.random.default_rng(seed)
    made_from = rng.integers(lo, len(X) if hi is None else hi, b)
    noise = rng.standard_normal((b, X.shape[1])) * (0.1 / np.sqrt(X.shape[1]))
    return (X[made_from] + noise).astype(np.float32), made_from.astype(np.int32)


def close_enough(L, ref):
    L, ref = np.asarray(L, np.float64), np.asarray(ref, np.float64)
    assert L.shape == ref.shape
    inf = np.isneginf(ref)
    assert np.array_equal(np.isneginf(L), inf), (L, ref)
    assert np.isfinite(L[~inf]).all() and np.isfinite(ref[~inf]).all()
    err = np.abs(L[~inf] - ref[~inf])
    bound = 2.0 ** -40 + 4 * np.spacing(np.abs(ref[~inf]))
    print(f"largest |L - L_ref| = {err.max() if err.size else 0:.3g}, smallest bound {bound.min() if err.size else 0:.3g}")
    assert (err <= bound).all(), (err.max(), L[~inf][np.argmax(err - bound)], ref[~inf][np.argmax(err - bound)])


def own_distances_agree(ix, Q, dist, frm, until):
    """The restated distances carry the handle's own bits: its ordinary query at K = the rows of the range returns every
    row at a finite distance, and what it returns is dist[q][row - frm]."""
    n = until - frm
    if not 1 <= n <= MAX_LIST or not len(Q):
        return
    oi, od, oc, _ = ix.batch_query_raw(n, Q)
    for q in range(len(Q)):
        assert oc[q] >= np.isfinite(dist[q]).sum()
        got, want = od[q, :oc[q]], dist[q, oi[q, :oc[q]] - frm]
        assert np.array_equal(bits(got), bits(want))


def check(g, X, Q, beta, frm=0, until=None, exclude=None, metric="l2"):
    until = len(X) if until is None else until
    dm = g.DeviceMatrix.from_host(X)
    ix = g.ExactIndex(dm, metric, frm, until)
    try:
        L, terms = ix.batch_query_logsumexp(Q, beta, exclude)
        dist = exact_distances(X[frm:until], ix._prepare(Q))
        own_distances_agree(ix, Q, dist, frm, until)
    finally:
        ix.close()
        dm.close()
    want_L, want_terms = g.logsumexp_reference(dist, beta, exclude, rows=np.arange(frm, until))
    assert L.dtype == np.float64 and terms.dtype == np.int32
    assert np.array_equal(terms, want_terms), (terms, want_terms)
    close_enough(L, want_L)
    return L, terms


# ---- shapes: the smallest at which each path can go wrong -----------------------------------------------------------------

@pytest.mark.parametrize("n", (1, 63, 255, 256, 257, 1000))
def test_row_counts(g, n):
    X = rows_of(n, n, 8)
    Q, _ = queries_of(n + 1, X, 5)
    _, terms = check(g, X, Q, 30.0)
    assert (terms == n).all()


def test_a_range_inside_the_rows(g):
    n = 1000                                                     # several row chunks; the range starts inside a 256-row group
    X = rows_of(11, n, 8)
    Q, _ = queries_of(12, X, 5, 37, n - 5)
    _, terms = check(g, X, Q, 30.0, 37, n - 5)
    assert (terms == n - 42).all()


@pytest.mark.parametrize("d", (1, 31, 32, 33, 70))
def test_dimensions_around_the_staging_step(g, d):
    X = rows_of(d, 300, d)
    Q, _ = queries_of(d + 1, X, 3)
    check(g, X, Q, 30.0)


@pytest.mark.parametrize("b", (1, 15, 16, 17, 40))
def test_batch_sizes_around_the_query_tile(g, b):
    X = rows_of(b, 300, 8)
    Q, _ = queries_of(b + 1, X, b)
    check(g, X, Q, 30.0)


def test_several_steps_per_chunk(g):
    """524 544 rows are 2049 groups of 256: one query tile asks for 2048 chunks, so every chunk but the last walks two
    groups and a lane's accumulator advances more than once."""
    n = 524544
    X = rows_of(21, n, 2)
    Q, _ = queries_of(22, X, 16)
    _, terms = check(g, X, Q, 30.0)
    assert (terms == n).all()


def test_two_passes(g):
    b = EXACT_SUB_BATCH + 5
    X = rows_of(31, 300, 8)
    Q, made_from = queries_of(32, X, b)
    exclude = np.where(np.arange(b) % 2 == 1, made_from, -1).astype(np.int32)    # the second pass reads ITS excluded rows
    _, terms = check(g, X, Q, 30.0, exclude=exclude)
    assert np.array_equal(terms, np.where(exclude >= 0, 299, 300))


# ---- content ----------------------------------------------------------------------------------------------------------------

def test_excluded_rows_inside_and_outside_the_range(g):
    X = rows_of(41, 600, 8)
    Q, made_from = queries_of(42, X, 20, 100, 500)
    exclude = np.where(np.arange(20) % 2 == 1, made_from, -1).astype(np.int32)
    exclude[4] = 7                                               # a row of the dataset outside the range: no term is lost
    _, terms = check(g, X, Q, 30.0, 100, 500, exclude)
    assert np.array_equal(terms, np.where(np.arange(20) % 2 == 1, 399, 400))


def test_a_nan_row_is_no_term(g):
    X = rows_of(51, 300, 8)
    X[5, 3] = np.nan
    Q, _ = queries_of(52, X, 6, 10)
    L, terms = check(g, X, Q, 30.0)
    assert (terms == 299).all() and np.isfinite(L).all()


def test_an_infinite_query_beside_ordinary_ones(g):
    X = rows_of(61, 300, 8)
    Q, _ = queries_of(62, X, 7)
    Q[2, 0] = np.inf
    L, terms = check(g, X, Q, 30.0)
    assert terms[2] == 0 and np.isneginf(L[2])
    assert (np.delete(terms, 2) == 300).all() and np.isfinite(np.delete(L, 2)).all()


def test_copies_of_the_query_add_one_each(g):
    X = np.tile(rows_of(71, 1, 8), (257, 1))                     # 257 rows, all the query: S = 257 exactly
    L, terms = check(g, X, X[:1], 30.0)
    assert terms[0] == 257 and abs(L[0] - math.log(257)) <= 2.0 ** -40 + 4 * np.spacing(math.log(257))
    X = rows_of(72, 300, 8)                                      # three copies among other rows: S >= 3
    Q = X[[10]]
    X[[20, 30]] = X[10]
    L, _ = check(g, X, Q, 30.0)
    assert math.log(3) < L[0] < math.log(4)


def test_every_term_underflows(g):
    X = (rows_of(81, 300, 8) * 40).astype(np.float32)            # distances of hundreds: exp(-128 * d) is 0
    Q = (X[:4] + np.float32(3)).astype(np.float32)
    L, terms = check(g, X, Q, 256.0)
    assert (terms == 300).all() and np.isneginf(L).all()
    with pytest.raises(ValueError, match="beta too large for these distances"):
        g.isf_offsets_from(L, terms, 256.0)


@pytest.mark.parametrize("beta", (0.5, 30.0, 100.0))
def test_beta(g, beta):
    X = rows_of(91, 300, 8)
    Q, _ = queries_of(92, X, 6)
    check(g, X, Q, beta)


def test_a_cosine_handle_normalises_its_queries(g):
    X = rows_of(101, 300, 16)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    Q, _ = queries_of(102, X, 6)
    Q = (Q * np.float32(3)).astype(np.float32)
    L, _ = check(g, X, Q, 30.0, metric="cosine")
    dm = g.DeviceMatrix.from_host(X)
    l2 = g.ExactIndex(dm, "l2")
    try:
        assert not np.array_equal(l2.batch_query_logsumexp(Q, 30.0)[0], L)       # taken as given there
    finally:
        l2.close()
        dm.close()


def test_a_used_handle_answers_like_a_fresh_one(g):
    X = rows_of(111, 700, 8)
    Q, made_from = queries_of(112, X, 20)
    dm = g.DeviceMatrix.from_host(X)
    used, fresh = g.ExactIndex(dm, "l2"), g.ExactIndex(dm, "l2")
    try:
        first = used.batch_query_logsumexp(Q, 30.0, made_from)
        used.batch_query_raw(100, Q)
        used.batch_query_offset_raw(10, Q, np.zeros(700, np.float32))
        used.batch_query_rank_raw(Q, [[int(r)] for r in made_from])
        used.batch_query_logsumexp(Q[:3], 100.0)
        again = used.batch_query_logsumexp(Q, 30.0, made_from)
        want = fresh.batch_query_logsumexp(Q, 30.0, made_from)
    finally:
        used.close()
        fresh.close()
        dm.close()
    for got in (first, again):
        assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and np.array_equal(got[1], want[1])


def test_the_host_checks(g):
    N = g.native
    L = N.lib()
    X = rows_of(121, 50, 4)
    dm = g.DeviceMatrix.from_host(X)
    ix = g.ExactIndex(dm, "l2")
    q, out, terms = np.zeros(8, np.float32), np.zeros(2, np.float64), np.zeros(2, np.int32)

    def call(b=2, beta=30.0, exclude=None, queries=q, lse=out, handle=None):
        return L.gulon_exact_index_query_logsumexp(ix._h if handle is None else handle, queries, b, beta, exclude, lse,
                                                   terms.ctypes.data)
    try:
        assert call() == N.OK
        assert call(b=0) == N.OK
        assert L.gulon_exact_index_query_logsumexp(ix._h, q, 2, 30.0, None, out, None) == N.OK       # out_terms is nullable
        for beta in (0.0, -1.0, float("nan"), float("inf")):
            assert call(beta=beta) == N.ERR_INVALID_ARGUMENT and "beta" in N.last_error()
        assert call(b=-1) == N.ERR_INVALID_ARGUMENT
        bad = np.array([-1, 50], np.int32)
        assert call(exclude=bad.ctypes.data) == N.ERR_INVALID_ARGUMENT and "exclude[1] = 50" in N.last_error()
        bad = np.array([-2, 3], np.int32)
        assert call(exclude=bad.ctypes.data) == N.ERR_INVALID_ARGUMENT and "exclude[0] = -2" in N.last_error()
        fn = L.gulon_exact_index_query_logsumexp
        saved = fn.argtypes
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        try:
            assert fn(ix._h, None, 2, 30.0, None, out.ctypes.data, None) == N.ERR_INVALID_ARGUMENT
            assert fn(ix._h, q.ctypes.data, 2, 30.0, None, None, None) == N.ERR_INVALID_ARGUMENT
            assert fn(ix._h, None, 0, 30.0, None, None, None) == N.OK                # b = 0 launches nothing
        finally:
            fn.argtypes = saved
        with pytest.raises(ValueError, match="beta"):
            ix.batch_query_logsumexp(X[:2], 0.0)
        with pytest.raises(ValueError, match="excluded rows"):
            ix.batch_query_logsumexp(X[:2], 30.0, [1])
    finally:
        ix.close()
        dm.close()
