"""Expression queries on the device (csrc/compose.hip): rows composed into query vectors, the index's own answer at
k + E with the operands dropped.  compose_rows against compose_reference(lookup_rows(...)); batch_query_expressions
against the restatement -- the library's own plain batch_query of the reference-composed vector at k + E, the operands
dropped on the host, the first k kept -- and, per index kind, against the same restatement fed the CPU oracle's index
query.  Everything bit for bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

N_ROWS, ITERS = 3000, 5
KS = (1, 10, 62, 63, 100)
WEIGHTS = (1.0, -1.0, 0.3, -1.7)


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


class Kind:
    """One index with what the checks need of it: lookup, the plain query, the flags of its metric, the oracle's query."""

    def __init__(self, name, index, cosine, n, d, codes, k, cents, oracle_query):
        self.name, self.index, self.cosine, self.n, self.d = name, index, cosine, n, d
        self.codes, self.k, self.cents, self.oracle_query = codes, k, cents, oracle_query

    def lookup(self, rows):
        return self.index.lookup_rows(np.asarray(rows, np.int32))

    def plain_raw(self, Q, depth, frm=0, until=None):
        """(rows, distances, counts, flags) of the index's plain query of prepared vectors."""
        if hasattr(self.index, "vector_index"):
            return self.index.vector_index.batch_query_raw(depth, Q, frm, until)
        oi, od, oc = self.index.batch_query_raw(depth, Q)
        return oi, od, oc, np.zeros(len(oc), np.int32)

    def expressions_raw(self, k, exprs, frm=0, until=None):
        if hasattr(self.index, "vector_index"):
            return self.index.vector_index.batch_query_terms_partitioned(k, exprs, frm, until, self.cosine, self.cosine)
        return self.index.batch_query_expressions_raw(k, exprs)

    def composed(self, exprs):
        """compose_reference over ONE lookup of all the term rows."""
        from gulon_amd.expressions import compose_reference
        vectors = self.lookup([r for e in exprs for r, _ in e])
        ends = np.cumsum([len(e) for e in exprs])
        return np.stack([compose_reference(vectors[end - len(e):end], [w for _, w in e], self.cosine, self.cosine)
                         for e, end in zip(exprs, ends)])


def _flat(g, oracle, name, d, m, k, metric, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N_ROWS, d)).astype(np.float32)
    if metric == "cosine":
        X = np.stack([oracle.normalize(r) for r in X])
    dm = g.DeviceMatrix.from_host(X)
    pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(k, m, ITERS))
    index = g.Index.sorted(dm, pq, metric)
    vi = index.vector_index
    codes, cents = vi.data.indices(), pq.flat_centroids()

    def oracle_query(Q, depth):
        return oracle.pq_batch_query(codes, d, k, cents, Q, depth)
    return Kind(name, index, metric == "cosine", N_ROWS, d, codes, k, cents, oracle_query), X, dm


@pytest.fixture(scope="module")
def world(g, oracle):
    from gulon_amd.grouped import GroupedIndex, group
    from gulon_amd.kmeans import Config as KMeansConfig
    out = {}
    out["l2"], X, dm = _flat(g, oracle, "l2", 48, 8, 256, "l2", 1)
    out["X"], out["dm"] = X, dm
    out["cosine"], _, _ = _flat(g, oracle, "cosine", 7, 3, 16, "cosine", 2)      # uneven sub-vectors, narrow codes
    out["wide"], _, _ = _flat(g, oracle, "wide", 48, 8, 1024, "l2", 3)
    assert out["wide"].index.vector_index.data.coder.width in (10, 12, 16)
    # grouped: 30 coarse clusters of the l2 vectors, the product quantizer on the residuals; then an EMPTY group put in
    # the middle (a repeated offset with a centroid of its own), so that the binarySearch rule of the lookup matters
    clustering = g.KMeans.compute_clusters(g.Vectors(dm), KMeansConfig(30, ITERS))
    gv = group(dm, clustering)
    pq = g.ProductQuantizer.apply(gv.residuals, g.ProductQuantizerConfig(256, 8, ITERS))
    enc = pq.encode(gv.residuals)
    at = len(gv.offsets) // 2
    offsets = np.insert(gv.offsets, at, gv.offsets[at]).astype(np.int32)
    centroids = np.insert(gv.centroids, at + 1, np.full(48, 0.5, np.float32), axis=0).astype(np.float32)
    assert (np.diff(np.r_[0, offsets, N_ROWS]) == 0).any() and 20 <= len(centroids) <= 40
    codes, cents = enc.indices(), pq.flat_centroids()
    for name, strategy, code, limit in (("grouped", g.LimitGroups(4), 0, 4),
                                        ("grouped_vectors", g.LimitVectors(N_ROWS // 4), 1, N_ROWS // 4)):
        gx = GroupedIndex(pq, enc, centroids, offsets, strategy, "l2")

        def oracle_query(Q, depth, code=code, limit=limit):
            return oracle.grouped_query(codes, 48, 256, cents, centroids, offsets, Q, depth, code, limit)
        out[name] = Kind(name, gx, False, N_ROWS, 48, codes, 256, cents, oracle_query)
    return out


KINDS = ["l2", "cosine", "wide", "grouped", "grouped_vectors"]


def _expressions(n, b, rng, weights=WEIGHTS):
    """1 to 4 terms; weights +-1 mostly, fractional ones among them; one in five repeats a row."""
    out = []
    for q in range(b):
        t = 1 + q % 4
        rows = rng.integers(0, n, t).tolist()
        if q % 5 == 4 and t > 1:
            rows[-1] = rows[0]
        w = [weights[int(i)] for i in rng.integers(0, 2 if q % 3 else len(weights), t)]
        out.append(list(zip(rows, w)))
    return out


def _same_vectors(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


# ---- composition -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["l2", "cosine", "wide", "grouped"])
@pytest.mark.parametrize("b", [1, 17, 1000])
def test_compose_rows_equals_the_reference(world, name, b):
    kind = world[name]
    rng = np.random.default_rng(b)
    exprs = _expressions(kind.n, b, rng)
    exprs[0] = [(5, 1.0), (5, -1.0)]                                   # x - x
    if b > 1:
        exprs[1] = [(0, 0.3), (kind.n - 1, -1.7), (0, 1.0), (kind.n - 1, 1.0)]
    got = kind.index.compose_rows(exprs)
    want = kind.composed(exprs)
    assert got.shape == (b, kind.d) and _same_vectors(got, want)
    if kind.cosine:
        assert np.isnan(got[0]).all()                                  # a zero vector normalises to NaN
    else:
        assert (got[0] == 0).all()                                     # and is a legitimate l2 query


def test_the_two_flags_are_independent(world):
    from gulon_amd.expressions import compose_reference
    kind = world["cosine"]
    vi = kind.index.vector_index
    exprs = _expressions(kind.n, 17, np.random.default_rng(4))
    for nt, nq in ((False, False), (True, False), (False, True), (True, True)):
        got = vi.compose_rows(exprs, nt, nq)
        want = np.stack([compose_reference(kind.lookup([r for r, _ in e]), [w for _, w in e], nt, nq) for e in exprs])
        assert _same_vectors(got, want), (nt, nq)
    gx = world["grouped"].index
    got = gx.compose_rows(exprs[:5], True, True)
    want = np.stack([compose_reference(gx.lookup_rows([r for r, _ in e]), [w for _, w in e], True, True)
                     for e in exprs[:5]])
    assert _same_vectors(got, want)


def test_compose_rows_at_the_largest_dimension(g):
    """d * 4 = 64 KiB: 64 running sums per thread, and with normalised terms two staged rows."""
    from gulon_amd.expressions import compose_reference
    n, d, m, k = 130, 16384, 4, 4
    rng = np.random.default_rng(9)
    pq = g.ProductQuantizer.from_flat(k, d, m, rng.standard_normal(k * d).astype(np.float32))
    coder = pq.coder_factory(n)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    ix = g.PQIndex(pq, g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(m)]))
    exprs = [[(3, 1.0), (129, -1.0), (64, 0.3)], [(0, -1.7)]]
    for flag in (False, True):
        got = ix.compose_rows(exprs, flag, flag)
        want = np.stack([compose_reference(ix.decode_rows([r for r, _ in e]), [w for _, w in e], flag, flag)
                         for e in exprs])
        assert _same_vectors(got, want), flag
    ix.close()


# ---- queries ---------------------------------------------------------------------------------------------------------

def _drop(rows, dist, count, operands, k):
    keep = [p for p in range(count) if int(rows[p]) not in operands][:k]
    return rows[keep], dist[keep]


def _restate(kind, exprs, k, query, frm=0, until=None):
    """Per expression: query(composed vector, k + E) -> its term rows dropped -> the first k.  `query(Q, depth)` gives
    (rows, distances, counts[, flags])."""
    from gulon_amd.expressions import partition_by_operands
    composed = kind.composed(exprs)
    out = [None] * len(exprs)
    for extra, where in partition_by_operands(exprs).items():
        got = query(composed[where], k + extra)
        for j, i in enumerate(where):
            operands = {r for r, _ in exprs[i]}
            assert len(operands) == extra
            rows, dist = _drop(got[0][j], got[1][j], int(got[2][j]), operands, k)
            hit = len(operands & set(got[0][j][:int(got[2][j])].tolist()))        # operands among the k + E nearest
            out[i] = (rows, dist, int(got[3][j]) if len(got) > 3 else 0, hit)
    return out


def _assert_lists(got, want, k, where, rows_too=True):
    oi, od, oc, of = got
    for q, (rows, dist, flags, _) in enumerate(want):
        n = len(rows)
        assert oc[q] == n, (where, q)
        if rows_too:
            assert oi[q, :n].tolist() == rows.tolist(), (where, q)
        nan = np.isnan(dist)
        assert np.array_equal(np.isnan(od[q, :n]), nan), (where, q)
        assert np.array_equal(bits(od[q, :n][~nan]), bits(dist[~nan])), (where, q)
        assert (oi[q, n:] == -1).all() and np.isposinf(od[q, n:]).all(), (where, q)      # the padding
        if rows_too:
            assert of[q] == flags, (where, q)


def _query_batch(kind, rng):
    """1-, 2- and 3-operand expressions, a repeated row, fractional weights; `-x` (far from x: nothing to drop) and
    plain `x` (x itself is the nearest: dropped) among them."""
    exprs = [e for e in _expressions(kind.n, 24, rng) if len({r for r, _ in e}) <= 3]
    exprs += [[(int(r), -1.0)] for r in rng.integers(0, kind.n, 4)]
    exprs += [[(int(r), 1.0)] for r in rng.integers(0, kind.n, 4)]
    exprs += [[(7, 1.0), (8, 1.0), (7, -1.0)], [(20, 1.0), (21, -1.0), (22, 1.0)]]
    return exprs


@pytest.mark.parametrize("name", KINDS)
def test_expression_queries_equal_the_restatement(world, name):
    kind = world[name]
    exprs = _query_batch(kind, np.random.default_rng(11))
    dropped_none = dropped_all = 0
    for k in KS:
        want = _restate(kind, exprs, k, kind.plain_raw)
        got = kind.expressions_raw(k, exprs)
        _assert_lists(got, want, k, (name, k))
        assert all(len(w[0]) == k for w in want)
        for e, w in zip(exprs, want):                                    # how many operands each answer lost
            dropped_none += w[3] == 0
            dropped_all += w[3] == len({r for r, _ in e})
        if k == 10:                                                      # the Result form
            results = kind.index.batch_query_expressions(k, exprs)
            assert [r.rows.tolist() for r in results] == [w[0].tolist() for w in want]
            assert all(np.array_equal(bits(r.distances), bits(w[1])) for r, w in zip(results, want))
    assert dropped_none > 0 and dropped_all > 0                          # both ends are met: truncated / all dropped


@pytest.mark.parametrize("name,k", [("l2", 10), ("l2", 63), ("cosine", 10), ("cosine", 62), ("wide", 100),
                                    ("grouped", 63), ("grouped_vectors", 100)])
def test_expression_queries_equal_the_oracle_index_query(world, g, name, k):
    """The same restatement over the ORACLE's index query of the composed vector.  Distances and counts always; rows
    where the library's answer IS the reference heap's -- a grouped index (literal heaps), a flat one without a tie
    flag or with the exact replay (depth k + E <= 63) -- and otherwise up to the order inside a tie group, as
    tests/test_gpu_wide_large_k.py compares them.  (The cosine index has 16^3 codes for 3000 rows: most of its lists
    hold equal distances, and at k = 62 every expression of two or three operands is past the replay's depth.)"""
    N = g.native
    kind = world[name]
    exprs = _query_batch(kind, np.random.default_rng(12))
    want = _restate(kind, exprs, k, kind.oracle_query)
    got = kind.expressions_raw(k, exprs)
    _assert_lists(got, want, k, (name, k, "distances"), rows_too=False)
    exact = 0
    for q, (rows, dist, _, _) in enumerate(want):
        flags = int(got[3][q])
        mine = got[0][q, :len(rows)]
        if name.startswith("grouped") or flags == 0 or flags & N.FLAG_EXACT_REPLAY:
            assert mine.tolist() == rows.tolist(), (name, k, q)
            exact += 1
        else:
            assert flags & (N.FLAG_BOUNDARY_TIE | N.FLAG_INTERIOR_TIE), (name, k, q)
            inner = dist < dist[-1]
            assert set(mine[inner].tolist()) == set(rows[inner].tolist()), (name, k, q)
            assert len(set(mine.tolist())) == len(mine)
    print(name, k, "compared row for row:", exact, "of", len(exprs))
    assert exact > 0
    if name != "cosine":
        assert exact >= len(exprs) - 2                                   # (an unreplayed tie is rare in 256^8 codes)


def test_a_range_shorter_than_the_depth(world):
    """k + E above the rows in range: a short count, (-1, +inf) after it."""
    kind = world["l2"]
    exprs = [[(101, 1.0)], [(101, 1.0), (500, -1.0)], [(100, 1.0), (102, 1.0), (104, -1.0)], [(2000, 1.0)]]
    want = _restate(kind, exprs, 10, lambda Q, depth: kind.plain_raw(Q, depth, 100, 105))
    got = kind.expressions_raw(10, exprs, 100, 105)
    _assert_lists(got, want, 10, "range")
    assert got[2].tolist() == [4, 4, 2, 5]
    assert (got[0][2, 2:] == -1).all() and np.isposinf(got[1][2, 2:]).all()


def test_a_nan_query_is_answered_by_the_non_finite_path(world, g):
    kind = world["cosine"]
    exprs = [[(5, 1.0), (5, -1.0)], [(2, 0.3), (2, -0.3)], [(9, 1.0)]]
    assert np.isnan(kind.composed(exprs[:2])).all()
    for k in (10, 62):                                                   # (depth k + 1 <= 63: the one-scan contract)
        want = _restate(kind, exprs, k, kind.plain_raw)
        got = kind.expressions_raw(k, exprs)
        _assert_lists(got, want, k, ("nan", k))
        assert np.isnan(got[1][0]).all() and got[2][0] == k
        assert 5 not in got[0][0].tolist() and 2 not in got[0][1].tolist()
        assert got[3][0] & g.native.FLAG_NONFINITE and got[3][1] & g.native.FLAG_NONFINITE


@pytest.mark.parametrize("name", ["l2", "cosine", "grouped"])
def test_an_answer_does_not_depend_on_the_batch(world, name):
    kind = world[name]
    exprs = _query_batch(kind, np.random.default_rng(13))
    for k in (10, 63):
        together = kind.expressions_raw(k, exprs)
        for q in (0, 1, 2, 5, len(exprs) - 1):
            alone = kind.expressions_raw(k, [exprs[q]])
            for a, b in zip(alone, together):
                x, y = np.asarray(a[0]), np.asarray(b[q])
                assert np.array_equal(bits(x), bits(y)) if x.dtype == np.float32 else np.array_equal(x, y), (name, k, q)


# ---- errors ----------------------------------------------------------------------------------------------------------

def test_bad_input_is_refused_by_the_host_forms(world, g):
    N = g.native
    for name in ("l2", "grouped"):
        kind = world[name]
        for bad in (-1, kind.n):
            with pytest.raises(ValueError, match="outside"):
                kind.index.compose_rows([[(0, 1.0), (bad, 1.0)]])
            with pytest.raises(ValueError, match="outside"):
                kind.expressions_raw(5, [[(1, 1.0)], [(bad, -1.0)]])
    # an empty expression, offsets that do not start at 0 -- through the C ABI (the Python types do not build them)
    vi, gx = world["l2"].index.vector_index, world["grouped"].index
    rows, w = np.asarray([1, 2], np.int32), np.ones(2, np.float32)
    out = np.zeros(2 * 48, np.float32)
    oi, od, oc = np.zeros(20, np.int32), np.zeros(20, np.float32), np.zeros(2, np.int32)
    for off in ([0, 0, 2], [0, 2, 2], [1, 2, 2], [0, 2, 1]):
        off = np.asarray(off, np.int32)
        assert N.lib().gulon_index_compose_rows(vi._h, off, rows, w, 2, 0, 0, out) == N.ERR_INVALID_ARGUMENT
        assert N.lib().gulon_grouped_index_compose_rows(gx._h, off, rows, w, 2, 0, 0, out) == N.ERR_INVALID_ARGUMENT
        assert N.lib().gulon_index_query_terms(vi._h, off, rows, w, 2, 10, 1, 0, 0, 0, N_ROWS, oi, od, oc,
                                               oc.copy()) == N.ERR_INVALID_ARGUMENT
        assert N.lib().gulon_grouped_index_query_terms(gx._h, off, rows, w, 2, 10, 1, 0, 0, 0, 4, oi, od,
                                                       oc) == N.ERR_INVALID_ARGUMENT
    assert N.lib().gulon_index_query_terms(vi._h, np.asarray([0, 1, 2], np.int32), rows, w, 2, 10, -1, 0, 0, 0, N_ROWS,
                                           oi, od, oc, oc.copy()) == N.ERR_INVALID_ARGUMENT
    assert world["l2"].index.batch_query_expressions(5, []) == []
    assert vi.compose_rows([]).shape == (0, 48)


def test_the_depth_counts_against_the_limits_of_the_index_form(world):
    with pytest.raises(NotImplementedError, match="k_nn = 8192 > 8191 is not supported"):
        world["l2"].expressions_raw(8191, [[(1, 1.0)]])
    with pytest.raises(NotImplementedError, match="k_nn = 2049 > 2048 is not supported by the grouped index"):
        world["grouped"].expressions_raw(2047, [[(1, 1.0), (2, -1.0)]])
    oi, od, oc, _ = world["grouped"].expressions_raw(2047, [[(1, 1.0)]])         # 2048: the largest depth answers
    assert 63 < oc[0] <= 2047 and 1 not in oi[0, :oc[0]].tolist()


@pytest.mark.parametrize("name", ["l2", "grouped"])
def test_device_forms_on_a_stream(world, g, name):
    """The _dev forms equal the host forms; a term row outside [0, n) gives a NaN vector (and the answer to a NaN
    query) and sets the row-error word."""
    import torch
    from gulon_amd.expressions import to_csr
    N = g.native
    L = N.lib()
    kind = world[name]
    grouped = name == "grouped"
    h = kind.index._h if grouped else kind.index.vector_index._h
    exprs = [e for e in _query_batch(kind, np.random.default_rng(14)) if len({r for r, _ in e}) == 2]
    b, k, d = len(exprs), 10, kind.d
    host_vectors = kind.index.compose_rows(exprs)
    host = (kind.index.batch_query_terms_raw(k, exprs, 2) + (None,)) if grouped else \
        kind.index.vector_index.batch_query_terms_raw(k, exprs, 2)
    off, rows, w = to_csr(exprs)
    dev = torch.device("cuda:0")
    toff, trows, tw = (torch.from_numpy(a).to(dev) for a in (off, rows, w))
    tv = torch.full((b, d), -7.0, dtype=torch.float32, device=dev)
    oi = torch.full((b, k), -7, dtype=torch.int32, device=dev)
    od = torch.full((b, k), -7.0, dtype=torch.float32, device=dev)
    oc = torch.full((b,), -7, dtype=torch.int32, device=dev)
    of = torch.full((b,), -7, dtype=torch.int32, device=dev)
    err = C.c_int32(-1)
    row_error = L.gulon_grouped_index_row_error if grouped else L.gulon_index_row_error
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)

    def run():
        with torch.cuda.stream(stream):
            if grouped:
                N.check(L.gulon_grouped_index_compose_rows_dev(h, toff.data_ptr(), trows.data_ptr(), tw.data_ptr(), b, 0,
                                                               0, tv.data_ptr(), st))
                N.check(L.gulon_grouped_index_query_terms_dev(h, toff.data_ptr(), trows.data_ptr(), tw.data_ptr(), b, k,
                                                              2, 0, 0, 0, 4, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                                              st))
            else:
                N.check(L.gulon_index_compose_rows_dev(h, toff.data_ptr(), trows.data_ptr(), tw.data_ptr(), b, 0, 0,
                                                       tv.data_ptr(), st))
                N.check(L.gulon_index_query_terms_dev(h, toff.data_ptr(), trows.data_ptr(), tw.data_ptr(), b, k, 2, 0, 0,
                                                      0, kind.n, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                                      of.data_ptr(), st))
        stream.synchronize()
    run()
    assert np.array_equal(bits(tv.cpu().numpy()), bits(host_vectors))
    assert np.array_equal(oi.cpu().numpy(), host[0]) and np.array_equal(bits(od.cpu().numpy()), bits(host[1]))
    assert np.array_equal(oc.cpu().numpy(), host[2])
    if not grouped:
        assert np.array_equal(of.cpu().numpy(), host[3])
    N.check(row_error(h, C.byref(err)))
    assert err.value == 0
    trows[int(off[3])] = kind.n                                          # expression 3 names a row past the end
    run()
    N.check(row_error(h, C.byref(err)))
    assert err.value == 1
    vectors = tv.cpu().numpy()
    assert np.isnan(vectors[3]).all()
    assert np.array_equal(bits(np.delete(vectors, 3, 0)), bits(np.delete(host_vectors, 3, 0)))
    assert np.array_equal(np.delete(oi.cpu().numpy(), 3, 0), np.delete(host[0], 3, 0))
    assert np.isnan(od.cpu().numpy()[3, :int(oc[3])]).all()              # the answer to an all-NaN query
    N.check(row_error(h, C.byref(err)))
    assert err.value == 0                                                # read and cleared


# ---- refined ---------------------------------------------------------------------------------------------------------

def test_refined_expression_queries(world, g, oracle):
    """RefinedIndex.batch_query_expressions = TopKHeap(k) over the candidate list with the operands dropped, by the
    exact distance from the composed vector to the original vectors (the _restate of tests/test_gpu_refine.py)."""
    from gulon_amd.word_vectors import DeviceWordVectors, KeyIndexSorted
    kind, X = world["l2"], world["X"]
    words = [f"w{i:05d}" for i in range(N_ROWS)]
    index = g.WordIndex(words, kind.index)
    vectors = DeviceWordVectors(words, world["dm"], KeyIndexSorted(words))
    refined = index.refined(vectors, 50)
    exprs = _query_batch(kind, np.random.default_rng(15))
    worded = [[(words[r], w) for r, w in e] for e in exprs] + [[("w00001", 1.0), ("absent", -1.0)], "w00007 - w00008"]
    composed = kind.composed(exprs + [[(7, 1.0), (8, -1.0)]])
    for k, c in ((10, 50), (5, 100), (63, 10)):
        c_eff = max(c, k)
        cands = _restate(kind, exprs + [[(7, 1.0), (8, -1.0)]], c_eff, kind.plain_raw)
        got = refined.batch_query_expressions(k, worded, candidates=c)
        assert got[len(exprs)] is None and len(got) == len(worded)
        got = got[:len(exprs)] + got[len(exprs) + 1:]
        for q, (res, (cand, _, flags, _)) in enumerate(zip(got, cands)):
            heap = oracle.TopKHeap(k)
            for r in cand.tolist():
                heap.update(r, oracle.distance_sq(composed[q], X[r]))
            ids, ds = heap.drain()
            assert res.rows.tolist() == ids.tolist(), (k, c, q)
            assert np.array_equal(bits(res.distances), bits(ds)) and res.flags == flags
            assert res.words == [words[i] for i in ids.tolist()]
    plain = index.batch_query_expressions(10, worded)
    assert plain[len(exprs)] is None
    assert plain[0].rows.tolist() == _restate(kind, exprs[:1], 10, kind.plain_raw)[0][0].tolist()
    assert index.query_expression(10, "w00007 - w00008").rows.tolist() == plain[-1].rows.tolist()
    assert refined.query_expression(10, worded[0], candidates=50).rows.tolist() == \
        refined.batch_query_expressions(10, worded[:1], candidates=50)[0].rows.tolist()
    refined.close()
