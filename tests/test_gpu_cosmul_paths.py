"""The 3CosMul scans (csrc/cosmul.hip) in the launch geometries and on the data the other cosmul files do
not reach: more than one row chunk on the flat index, more than one 256-row group per workgroup on the exact index,
ranges that cut chunks and start past the first group, row_base, contexts, short and empty ranges, equal scores across
waves and chunks, scores clamped to 0, non-finite distances, and the _dev forms with a bad expression in a later pass.

Every case that names a geometry asserts it first, through gulon_selftest_cosmul_{flat,exact}_shape of the hooks library
(the launchers' own arithmetic); every case that names a property of its data asserts it from the numpy reference alone.
Then rows and score BITS against that reference (cosmul_ref.same): no tolerances.

The flat worlds are planted, not trained: ProductQuantizer.from_flat over random centroids and random codes through the
coder.  d = 32, m = 16, k = 256 unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits
from cosmul_ref import (equal_neighbours, exact_distances, flat_term_distances, mixed_batch, native_index, per_expression,
                        reference_lists, run_dev, same, unit_rows, zero_factors)

pytestmark = pytest.mark.gpu

N_FLAT = 6250                                # 98 code blocks: three chunks of 33 / 33 / 32, the last block ragged
UP_TO_FIVE = ("+", "+-", "+-+", "-+++-")     # m = 25 is m_pad = 28: five terms in 144 KiB of LDS
NAN_AT, PINF_AT, NINF_AT = (3, 7), (5, 9), (5, 200)      # (quantizer, centroid) of the planted non-finite centroids


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def flat_shape(g, vi, b, frm, until):
    """[questions per pass, chunks of the first pass, code blocks per chunk] of a flat cosmul call."""
    out = np.zeros(3, np.int32)
    H = g.native.hooks_lib()
    assert H.gulon_selftest_cosmul_flat_shape(vi._h, b, frm, until, out) == 0, H.gulon_last_error()
    return out.tolist()


def exact_shape(g, ix, b):
    """[questions per pass, chunks of the first pass, 256-row groups per chunk] of an exact cosmul call."""
    out = np.zeros(3, np.int32)
    H = g.native.hooks_lib()
    assert H.gulon_selftest_cosmul_exact_shape(ix._h, b, out) == 0, H.gulon_last_error()
    return out.tolist()


# ---------------------------------------------------------------- flat index
_FLAT = {}


def flat_world(g, name):
    """(PQIndex, quantizer, codes [n][m], flat centroids, codes as planted [m][n]): made once per name."""
    if name in _FLAT:
        return _FLAT[name]
    n, d, m, k = {"m25": (N_FLAT, 32, 25, 256), "m64": (2000, 128, 64, 256)}.get(name, (N_FLAT, 32, 16, 256))
    rng = np.random.default_rng(sum(map(ord, name)))
    cents = (rng.standard_normal(k * d) / np.sqrt(d)).astype(np.float32)       # decoded rows of norm about 1
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    if name == "twins":                      # rows r and r + 3125 hold the same codes
        idx = np.concatenate([idx[:, :n // 2], idx[:, :n // 2]], axis=1)
    if name == "far":                        # any two rows differ by far more than 4
        cents *= np.float32(3 * np.sqrt(d))
    if name == "nonfinite":
        fr, un = g.subvector_bounds(d, m)
        at = lambda jc, e: k * int(fr[jc[0]]) + jc[1] * int(un[jc[0]] - fr[jc[0]]) + e
        cents[at(NAN_AT, 0)], cents[at(PINF_AT, 1)], cents[at(NINF_AT, 0)] = np.nan, np.inf, -np.inf
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    _FLAT[name] = (native_index(g, pq, idx), pq, np.ascontiguousarray(idx.T), pq.flat_centroids(), idx)
    return _FLAT[name]


def flat_reference(oracle, w, exprs, knn, frm=0, until=None, normalize=True, row_base=0):
    """The contract on the host for rows [frm, until) of the world `w`; returned ids and the dropped term rows carry
    row_base."""
    vi, _, codes, cents, _ = w
    until = len(codes) if until is None else until
    D = flat_term_distances(oracle, vi, codes, cents, exprs, normalize)
    based = [[(r + row_base, s) for r, s in e] for e in exprs]
    return reference_lists(per_expression(D[:, frm:until], exprs), based, row_base + np.arange(frm, until), knn)


def padding(got, q=slice(None)):
    return (got[0][q] == -1).all() and np.isneginf(got[1][q]).all() and (got[2][q] == 0).all()


@pytest.mark.parametrize("name,knn", [("m16", 10), ("m16", 55), ("m25", 10), ("m25", 55)])
def test_flat_three_uneven_chunks(g, oracle, name, knn):
    """98 blocks as 33 / 33 / 32 with the last block ragged, both code-word layouts (m = 16: one 16-byte word; m = 25:
    seven 4-byte words, the last padded)."""
    w = flat_world(g, name)
    vi = w[0]
    exprs = mixed_batch(knn + len(name), N_FLAT, 17, **({"patterns": UP_TO_FIVE} if name == "m25" else {}))
    assert flat_shape(g, vi, 17, 0, N_FLAT)[1:] == [3, 33]
    same(vi.batch_query_cosmul_raw(knn, exprs, normalize=True), flat_reference(oracle, w, exprs, knn))


@pytest.mark.parametrize("name,knn", [("m16", 10), ("m16", 55), ("m25", 10), ("m25", 55)])
def test_flat_range_cuts_first_and_last_chunk(g, oracle, name, knn):
    """Rows [70, 6100): blocks 1 .. 95 as 48 / 47, the first and the last holding rows outside the range.  (At k = 55
    the 19 lists name a sixth of the rows, so no code block can go unread unnoticed.)"""
    w = flat_world(g, name)
    vi = w[0]
    exprs = mixed_batch(31, N_FLAT, 17, **({"patterns": UP_TO_FIVE} if name == "m25" else {}))
    exprs += [[(5, 1.0), (6200, -1.0), (69, 1.0)], [(6100, 1.0), (70, -1.0), (6099, 1.0)]]
    rows = [r for e in exprs for r, _ in e]
    assert any(r < 70 or r >= 6100 for r in rows) and any(70 <= r < 6100 for r in rows)
    assert flat_shape(g, vi, len(exprs), 70, 6100)[1:] == [2, 48]
    got = vi.batch_query_cosmul_raw(knn, exprs, 70, 6100, normalize=True)
    same(got, flat_reference(oracle, w, exprs, knn, 70, 6100))
    assert got[0].min() >= 70 and got[0].max() < 6100


@pytest.mark.parametrize("knn", [10, 55])
def test_flat_equal_scores_across_chunks(g, oracle, knn):
    """Rows r and r + 3125 hold the same codes and lie in different chunks (a chunk is 2112 rows): they must come out
    next to each other, the lower row first."""
    w = flat_world(g, "twins")
    vi, codes = w[0], w[2]
    assert np.array_equal(codes[:3125], codes[3125:])
    exprs = mixed_batch(41, N_FLAT, 17)
    assert flat_shape(g, vi, 17, 0, N_FLAT)[1:] == [3, 33] and 3125 > 33 * 64
    want = flat_reference(oracle, w, exprs, knn)
    for pairs in equal_neighbours(want):
        assert any(b - a == 3125 for a, b in pairs), pairs
    same(vi.batch_query_cosmul_raw(knn, exprs, normalize=True), want)


def test_flat_every_score_clamped_to_zero(g, oracle):
    """l2, rows as they are, any two rows further apart than 4: every row that is no term row scores 0, so the answer is
    the first k of them in row order -- across the waves of a workgroup and across three chunks."""
    from gulon_amd.expressions import cosmul_reference
    w = flat_world(g, "far")
    vi, codes, cents = w[0], w[2], w[3]
    frm, until, knn = 70, N_FLAT, 55
    exprs = mixed_batch(51, N_FLAT, 17, patterns=("+", "+-"), lo=frm)
    exprs[0] = [(frm, 1.0), (frm + 2, -1.0)]                 # the first rows of the range are term rows
    assert flat_shape(g, vi, 17, frm, until)[1:] == [3, 33]
    D = per_expression(flat_term_distances(oracle, vi, codes, cents, exprs, False), exprs)
    want = flat_reference(oracle, w, exprs, knn, frm, until, normalize=False)
    for q, e in enumerate(exprs):
        others = np.setdiff1d(np.arange(frm, until), [r for r, _ in e])
        assert (D[q][:, others] > 4).all()
        assert (cosmul_reference(D[q], [s for _, s in e])[others] == 0).all()
        assert want[0][q].tolist() == others[:knn].tolist() and (want[1][q] == 0).all()
    same(vi.batch_query_cosmul_raw(knn, exprs, frm, until, normalize=False), want)


def test_flat_row_base_and_context(g, oracle):
    """An index at row_base 5000: term rows and ranges are local, the returned ids carry the base.  Its context()
    answers identically, and the parent's batch_query is what it was before any of it."""
    w0 = flat_world(g, "m16")
    vi0, pq, idx = w0[0], w0[1], w0[4]
    based = native_index(g, pq, idx, row_base=5000)
    ctx = None
    try:
        w = (based,) + w0[1:]
        Q = unit_rows(3, 9, 32)
        before = based.batch_query_raw(10, Q)
        exprs = mixed_batch(61, N_FLAT, 17)
        assert flat_shape(g, based, 17, 0, N_FLAT)[1:] == [3, 33]
        got = based.batch_query_cosmul_raw(10, exprs, normalize=True)
        same(got, flat_reference(oracle, w, exprs, 10, row_base=5000))
        assert got[0].min() >= 5000
        plain = vi0.batch_query_cosmul_raw(10, exprs, normalize=True)
        same(got, (np.where(plain[0] >= 0, plain[0] + 5000, -1), plain[1], plain[2]))
        cut = based.batch_query_cosmul_raw(55, exprs, 70, 6100, normalize=True)
        same(cut, flat_reference(oracle, w, exprs, 55, 70, 6100, row_base=5000))
        ctx = based.context()
        assert flat_shape(g, ctx, 17, 0, N_FLAT)[1:] == [3, 33]
        same(ctx.batch_query_cosmul_raw(10, exprs, normalize=True), got)
        same(ctx.batch_query_cosmul_raw(55, exprs, 70, 6100, normalize=True), cut)
        same(based.batch_query_cosmul_raw(10, exprs, normalize=True), got)
        after = based.batch_query_raw(10, Q)
        fresh = native_index(g, pq, idx, row_base=5000)
        try:
            other = fresh.batch_query_raw(10, Q)
        finally:
            fresh.close()
        for x in (after, other, ctx.batch_query_raw(10, Q)):
            assert np.array_equal(x[0], before[0]) and np.array_equal(bits(x[1]), bits(before[1]))
            assert np.array_equal(x[2], before[2]) and np.array_equal(x[3], before[3])
    finally:
        if ctx is not None:
            ctx.close()
        based.close()


def test_flat_short_ranges(g, oracle):
    w = flat_world(g, "m16")
    vi = w[0]
    exprs = mixed_batch(71, N_FLAT, 5)
    for at in (128, 100, 0, N_FLAT):                         # from == until, at a multiple of 64 and not
        assert padding(vi.batch_query_cosmul_raw(10, exprs, at, at, normalize=True))
    one = [[(777, 1.0), (5, -1.0)], [(6000, 1.0), (777, -1.0), (4, 1.0)], [(777, 1.0)]]
    assert padding(vi.batch_query_cosmul_raw(10, one, 777, 778, normalize=True))          # the one row is an operand
    got, want = vi.batch_query_cosmul_raw(10, one, 778, 779, normalize=True), flat_reference(oracle, w, one, 10, 778, 779)
    assert want[2].tolist() == [1, 1, 1] and (want[0][:, 0] == 778).all()
    same(got, want)
    frm, until, knn = 1010, 1050, 55                         # 40 rows over two code blocks, fewer than k
    short = mixed_batch(72, until, 9, lo=frm) + mixed_batch(73, N_FLAT, 4)
    want = flat_reference(oracle, w, short, knn, frm, until)
    left = [40 - len({r for r, _ in e if frm <= r < until}) for e in short]
    assert want[2].tolist() == left and min(left) < 40 and max(left) == 40
    got = vi.batch_query_cosmul_raw(knn, short, frm, until, normalize=True)
    same(got, want)
    for q, c in enumerate(left):
        assert (got[0][q, c:] == -1).all() and np.isneginf(got[1][q, c:]).all()


def nonfinite_assertions(D, exprs, zero_p, zero_n):
    """From the reference alone: every score finite and >= 0; expression zero_p has a positive term and expression
    zero_n a negative term whose factor is 0 on every row (but, at most, the term's own)."""
    from gulon_amd.expressions import cosmul_reference
    for Dq, e in zip(D, exprs):
        score = cosmul_reference(Dq, [s for _, s in e])
        assert np.isfinite(score).all() and (score >= 0).all()
    for q, sign in ((zero_p, 1.0), (zero_n, -1.0)):
        zf = zero_factors(D[q])
        assert any(zf[t].sum() >= zf.shape[1] - 1 for t, (_, s) in enumerate(exprs[q]) if s == sign), (q, sign)


def test_flat_non_finite_centroids(g, oracle):
    """l2, rows as they are.  One centroid holds a NaN, one +inf and one -inf: a term row that selects the NaN centroid
    is at a NaN distance from every row, one that selects the +inf centroid at inf or NaN; candidates that select them
    are at NaN / inf from every term.  Every factor of those is 0, in P and -- where the denominator becomes 0 + 0.001 --
    in N; every score stays finite."""
    w = flat_world(g, "nonfinite")
    vi, codes, cents = w[0], w[2], w[3]
    sel = {name: np.flatnonzero(codes[:, j] == c) for name, (j, c) in
           (("nan", NAN_AT), ("pinf", PINF_AT), ("ninf", NINF_AT))}
    assert all(10 <= len(rows) <= 50 for rows in sel.values()), {n: len(r) for n, r in sel.items()}
    special = np.concatenate(list(sel.values()))
    A = int(np.setdiff1d(np.arange(100, N_FLAT), special)[0])
    B = int(np.setdiff1d(sel["nan"], np.concatenate([sel["pinf"], sel["ninf"]]))[0])
    Cc = int(np.setdiff1d(sel["pinf"], sel["nan"])[0])
    exprs = [[(A, 1.0)], [(B, 1.0)], [(Cc, 1.0)], [(A, 1.0), (B, -1.0)], [(A, 1.0), (Cc, -1.0)], [(B, 1.0), (A, -1.0)],
             [(Cc, 1.0), (A, -1.0)], [(A, 1.0), (B, -1.0), (Cc, 1.0)], [(B, -1.0), (A, 1.0), (Cc, -1.0)]]
    exprs += mixed_batch(81, N_FLAT, 8)
    assert flat_shape(g, vi, len(exprs), 0, N_FLAT)[1:] == [3, 33]
    D = per_expression(flat_term_distances(oracle, vi, codes, cents, exprs, False), exprs)
    assert np.isfinite(D[0][0][np.setdiff1d(np.arange(N_FLAT), special)]).all() and np.isnan(D[0][0][sel["nan"]]).all()
    assert np.isinf(D[0][0][np.setdiff1d(sel["pinf"], sel["nan"])]).all()
    assert np.isnan(D[1][0]).all()                                                   # term B
    assert (np.isnan(D[2][0]) | np.isposinf(D[2][0])).all()                          # term C
    assert np.isnan(D[2][0]).any() and np.isposinf(D[2][0]).any()
    nonfinite_assertions(D, exprs, 1, 3)
    nonfinite_assertions(D, exprs, 2, 4)
    for knn in (10, 55):
        same(vi.batch_query_cosmul_raw(knn, exprs, normalize=False),
             flat_reference(oracle, w, exprs, knn, normalize=False))


def test_flat_dev_form_bad_expression_in_the_second_pass(g):
    """m = 64: 512 questions per pass.  Of 600, number 550 has no positive term and number 590 a row outside the index:
    those two come back empty and set the row-error word, the others answer as the host form does for the list without
    them."""
    N = g.native
    vi = flat_world(g, "m64")[0]
    n, k = 2000, 3
    exprs = mixed_batch(12, n, 600, patterns=("+", "+-"))
    exprs[550] = [(4, -1.0), (5, -1.0)]
    exprs[590] = [(7, 1.0), (n, -1.0)]
    good = [q for q in range(600) if q not in (550, 590)]
    assert flat_shape(g, vi, 600, 0, n)[0] == 512
    err = C.c_int32(-1)
    N.check(N.lib().gulon_index_row_error(vi._h, C.byref(err)))                     # cleared
    call = lambda off, rows, w, b, oi, os_, oc, _: N.lib().gulon_index_query_cosmul_dev(vi._h, off, rows, w, b, k, 1, 0, n,
                                                                                       oi, os_, oc, None)
    (oi, os_, oc), _ = run_dev(g, call, exprs, k, False)
    N.check(N.lib().gulon_index_row_error(vi._h, C.byref(err)))
    assert err.value == 1
    assert padding((oi, os_, oc), [550, 590])
    host = vi.batch_query_cosmul_raw(k, [exprs[q] for q in good], normalize=True)
    assert (host[2] == k).all()
    same((oi[good], os_[good], oc[good]), host)
    N.check(N.lib().gulon_index_row_error(vi._h, C.byref(err)))
    assert err.value == 0


# ---------------------------------------------------------------- exact index
_EXACT = {}


def exact_world(g, name):
    """(X, its device copy): made once per name."""
    if name not in _EXACT:
        X = {"copies": lambda: np.tile(unit_rows(91, 325, 7), (4, 1)),        # rows r, r + 325, r + 650, r + 975 equal
             "1500x16": lambda: unit_rows(92, 1500, 16),
             "63x7": lambda: unit_rows(93, 63, 7)}[name]()
        _EXACT[name] = (X, g.DeviceMatrix.from_host(X))
    return _EXACT[name]


def exact_reference(ix, X, exprs, k):
    """The contract on the host for the handle `ix` over rows [ix.frm, ix.until) of X."""
    Q = ix.compose_rows([[(r, 1.0)] for e in exprs for r, _ in e])
    D = exact_distances(X[ix.frm:ix.until], Q)
    return reference_lists(per_expression(D, exprs), exprs, np.arange(ix.frm, ix.until), k), per_expression(D, exprs)


@pytest.mark.parametrize("patterns", [("+", "+-", "+-+", "-+++-", "8"), ("+", "+-")])
def test_exact_several_groups_per_workgroup(g, patterns):
    """1300 rows are six 256-row groups; 2048 questions make three chunks of two groups, so a workgroup carries its
    lists from one group into the next.  Equal rows 325 apart meet inside a workgroup, 650 apart across chunks."""
    X, dm = exact_world(g, "copies")
    ix = g.ExactIndex(dm, "cosine")
    try:
        exprs = mixed_batch(9 + len(patterns), 1300, 2048, patterns=patterns)
        assert exact_shape(g, ix, 2048) == [4096, 3, 2]
        want, _ = exact_reference(ix, X, exprs, 10)
        pairs = [p for l in equal_neighbours(want) for p in l]
        assert any(b - a == 325 and a // 512 == b // 512 and a // 256 != b // 256 for a, b in pairs)
        assert any(a // 512 != b // 512 for a, b in pairs)
        same(ix.batch_query_cosmul_raw(10, exprs), want)
    finally:
        ix.close()


def test_exact_range_starts_past_the_first_group(g):
    """Rows [300, 1301): the scan starts at row 256 and rows 256 .. 299 are staged but not valid."""
    X, dm = exact_world(g, "1500x16")
    ix = g.ExactIndex(dm, "cosine", 300, 1301)
    try:
        exprs = mixed_batch(3, 1500, 17)                     # operands anywhere in the matrix
        exprs += [[(5, 1.0), (1400, -1.0), (299, 1.0)], [(1301, 1.0), (300, -1.0), (1300, 1.0)]]
        assert exact_shape(g, ix, 19) == [4096, 5, 1]
        got = ix.batch_query_cosmul_raw(10, exprs)
        same(got, exact_reference(ix, X, exprs, 10)[0])
        assert got[0].min() >= 300 and got[0].max() < 1301
        many = mixed_batch(4, 1500, 2048)
        assert exact_shape(g, ix, 2048) == [4096, 3, 2]
        got = ix.batch_query_cosmul_raw(10, many)
        same(got, exact_reference(ix, X, many, 10)[0])
        assert got[0].min() >= 300 and got[0].max() < 1301
    finally:
        ix.close()


def test_exact_short_ranges(g):
    X, dm = exact_world(g, "1500x16")
    exprs = mixed_batch(5, 1500, 5)
    for at in (300, 512, 0, 1500):                           # from == until, at a multiple of 256 and not
        ix = g.ExactIndex(dm, "cosine", at, at)
        try:
            assert padding(ix.batch_query_cosmul_raw(10, exprs))
        finally:
            ix.close()
    ix = g.ExactIndex(dm, "cosine", 300, 311)                # 11 rows at k = 20
    try:
        short = mixed_batch(6, 311, 9, lo=300) + mixed_batch(7, 1500, 4)
        want, _ = exact_reference(ix, X, short, 20)
        left = [11 - len({r for r, _ in e if 300 <= r < 311}) for e in short]
        assert want[2].tolist() == left and min(left) < 11 and max(left) == 11
        got = ix.batch_query_cosmul_raw(20, short)
        same(got, want)
        for q, c in enumerate(left):
            assert (got[0][q, c:] == -1).all() and np.isneginf(got[1][q, c:]).all()
    finally:
        ix.close()


def test_exact_non_finite_rows(g):
    """An l2 handle over rows with a NaN, +inf, -inf and 1e30 (its squared difference overflows), as candidates and as
    positive and negative terms: their factors are 0, every score stays finite."""
    X = np.random.default_rng(5).standard_normal((257, 33)).astype(np.float32) * np.float32(0.35)
    A, RN, RP, RM, RB = 1, 10, 20, 30, 40
    X[RN, 5], X[RP, 0], X[RM, 32], X[RB, 3] = np.nan, np.inf, -np.inf, 1e30
    dm = g.DeviceMatrix.from_host(X)
    ix = g.ExactIndex(dm)
    try:
        exprs = [[(A, 1.0)], [(RN, 1.0)], [(RP, 1.0)], [(A, 1.0), (RN, -1.0)], [(A, 1.0), (RP, -1.0)], [(RM, 1.0)],
                 [(RB, 1.0)], [(A, 1.0), (RM, -1.0)], [(A, 1.0), (RB, -1.0)], [(RN, 1.0), (A, -1.0)],
                 [(RP, 1.0), (A, -1.0), (RB, 1.0)], [(RM, -1.0), (A, 1.0), (RN, -1.0), (RB, 1.0)]]
        exprs += mixed_batch(9, 257, 8)
        want, D = exact_reference(ix, X, exprs, 10)
        assert np.isnan(D[0][0][[RN, RP, RM]]).sum() == 1 and np.isposinf(D[0][0][[RP, RM, RB]]).all()
        assert np.isnan(D[1][0]).all()
        for q in (2, 5, 6):                                  # inf to every row but itself: NaN (inf - inf) or 0
            assert np.isposinf(np.delete(D[q][0], exprs[q][0][0])).sum() >= 253
        assert np.isnan(D[2][0][RP]) and D[6][0][RB] == 0
        nonfinite_assertions(D, exprs, 1, 3)
        nonfinite_assertions(D, exprs, 2, 4)
        nonfinite_assertions(D, exprs, 6, 8)
        same(ix.batch_query_cosmul_raw(10, exprs), want)
        want55, _ = exact_reference(ix, X, exprs[:10], 55)
        same(ix.batch_query_cosmul_raw(55, exprs[:10]), want55)
    finally:
        ix.close()
        dm.close()


def test_exact_dev_form_bad_expression_in_the_second_pass(g):
    """4096 questions per pass.  Of 4100, number 4097 has no positive term and number 4099 a row outside the matrix:
    those two come back empty and set *d_err, the rest equal the reference."""
    N = g.native
    X, dm = exact_world(g, "63x7")
    ix = g.ExactIndex(dm, "cosine")
    try:
        k = 3
        exprs = mixed_batch(21, 63, 4100, patterns=("+", "+-"))
        exprs[4097] = [(4, -1.0), (5, -1.0)]
        exprs[4099] = [(7, 1.0), (63, -1.0)]
        good = [q for q in range(4100) if q not in (4097, 4099)]
        assert exact_shape(g, ix, 4100)[0] == 4096
        call = lambda off, rows, w, b, oi, os_, oc, err: N.lib().gulon_exact_index_query_cosmul_dev(
            ix._h, off, rows, w, b, k, 1, oi, os_, oc, err, None)
        (oi, os_, oc), err = run_dev(g, call, exprs, k, True)
        assert err == 1
        assert padding((oi, os_, oc), [4097, 4099])
        same((oi[good], os_[good], oc[good]), exact_reference(ix, X, [exprs[q] for q in good], k)[0])
    finally:
        ix.close()
