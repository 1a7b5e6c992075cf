"""Refined queries on the device.  gulon_refine_topk (csrc/refine.hip) against the oracle's pieces -- for every candidate
list TopKHeap(k), update(row, distance_sq) in list order, drain -- and RefinedIndex over a sorted l2, a sorted cosine and
a grouped index against the same restatement fed the oracle's own index results."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

F = np.float32
N_ROWS, DIM, K, M, ITERS = 6000, 48, 256, 8, 5          # the shapes of tests/test_gpu_recall.py
QUERIES = 120
CASES = [(10, 100), (1, 1), (63, 64), (100, 10), (1000, 1000)]      # (k, c)


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def _restate(oracle, k, query, cand, V, row_map=None):
    """The definition: heap = TopKHeap(k); update(id, distanceSq(query, V[map[id]])) in list order, negative ids
    skipped; Result.fromHeap."""
    heap = oracle.TopKHeap(k)
    for r in cand.tolist():
        if r >= 0:
            heap.update(r, oracle.distance_sq(query, V[r if row_map is None else row_map[r]]))
    return heap.drain()


def _assert_equal(got, want, where):
    rows, dist, counts = got
    for q, (ids, ds) in enumerate(want):
        n = len(ids)
        assert counts[q] == n, (where, q)
        assert rows[q, :n].tolist() == ids.tolist(), (where, q)
        nan = np.isnan(ds)
        assert np.array_equal(np.isnan(dist[q, :n]), nan), (where, q)
        assert np.array_equal(bits(dist[q, :n][~nan]), bits(ds[~nan])), (where, q)
        assert (rows[q, n:] == -1).all(), (where, q)


def _data(d, n, rng):
    X = rng.standard_normal((n, d)).astype(np.float32)
    if d == 1:
        X = (np.round(X * 4) / 4).astype(np.float32)                # one dimension: most distances tie
    X[100:110] = X[100]                                             # groups of identical vectors at different rows
    X[200:203] = X[200]
    X[7, d // 2] = np.nan                                           # a NaN row, +inf and -inf rows
    X[8, 0], X[9, d - 1] = np.inf, -np.inf
    return X


def _lists(b, c, n, rng):
    rows = rng.integers(10, n, (b, c)).astype(np.int32)
    if c > 1:
        rows[:, 1] = rows[:, 0]                                     # duplicate candidate ids
    special = np.asarray([7, 8, 9, 100, 104, 109, 101, 200, 202, 201], np.int32)
    for q in range(b):
        at = rng.integers(0, c, len(special))
        rows[q, at] = special
        if q % 3 == 0:
            rows[q, 0] = 7                                          # the NaN row first: it gets into the filling heap
        if q % 3 == 1:
            rows[q, c - 1] = 7                                      # and last: offered to a full heap
        if q % 4 == 2 and c > 12:
            rows[q, rng.integers(0, c, c // 3)] = np.arange(100, 110)[rng.integers(0, 10, c // 3)]   # mostly ties
    counts = rng.integers(0, c + 1, b)                              # short lists, -1 padding; some empty
    counts[0] = c
    if b > 1:
        counts[b - 1] = 0
    rows[np.arange(c)[None, :] >= counts[:, None]] = -1
    if b > 2 and c > 4:
        rows[2, rng.integers(0, c, 3)] = -1                         # and negative entries inside a list
    return rows


@pytest.mark.parametrize("d,b,c,k", [
    (1, 1, 1, 1), (7, 17, 63, 10), (48, 17, 64, 64), (300, 17, 100, 63), (48, 1000, 100, 10), (7, 1000, 64, 1),
    (4100, 17, 100, 100), (1, 17, 1000, 1000), (48, 17, 8191, 1000), (300, 1, 8191, 8191), (48, 17, 1000, 64),
    (7, 17, 8191, 10), (1, 1000, 63, 63),
])
def test_refine_topk_equals_the_heap_restatement(g, oracle, d, b, c, k):
    n = 3000
    rng = np.random.default_rng(1000 * d + b + c + k)
    X = _data(d, n, rng)
    Q = rng.standard_normal((b, d)).astype(np.float32)
    cand = _lists(b, c, n, rng)
    dm = g.DeviceMatrix.from_host(X)
    want = [_restate(oracle, k, Q[q], cand[q], X) for q in range(b)]
    assert any(np.isnan(ds).any() for _, ds in want) or c == 1
    _assert_equal(g.refine_topk(dm, Q, cand, k), want, "identity")
    # a non-identity map: candidate id i stands for row perm[i] of a shuffled copy of the matrix
    perm = rng.permutation(n).astype(np.int32)
    shuffled = np.empty_like(X)
    shuffled[perm] = X
    dm2 = g.DeviceMatrix.from_host(shuffled)
    _assert_equal(g.refine_topk(dm2, Q, cand, k, row_map=perm), want, "mapped")
    for q in range(min(b, 3)):                                      # (the restatement reads the map the same way)
        assert _restate(oracle, k, Q[q], cand[q], shuffled, perm)[0].tolist() == want[q][0].tolist()
    dm.close()
    dm2.close()


def test_a_nan_inside_the_heap_lets_the_root_rise(g, oracle):
    """Seven slots filled with 5, 1, NaN, 0.5, 0.25, 3, 9: the 9 sits under the NaN.  7 is then refused (5 > 7 is false),
    4 replaces the root -- which becomes 9 -- and the next 7 is taken.  A replay that drops what fails against an
    earlier root would lose it."""
    d2 = np.asarray([5, 1, np.nan, 0.5, 0.25, 3, 9, 7, 4, 7, 8.5, 100, 2], np.float32)
    X = np.sqrt(d2).reshape(-1, 1).astype(np.float32)
    cand = np.arange(len(d2), dtype=np.int32).reshape(1, -1)
    Q = np.zeros((1, 1), np.float32)
    ids, ds = _restate(oracle, 7, Q[0], cand[0], X)
    assert 9 in ids.tolist() and 7 not in ids.tolist()              # the second 7 (id 9) got in, the first did not
    dm = g.DeviceMatrix.from_host(X)
    _assert_equal(g.refine_topk(dm, Q, cand, 7), [(ids, ds)], "nan")
    dm.close()


def test_refine_topk_rejects_bad_arguments(g):
    X = np.arange(40, dtype=np.float32).reshape(10, 4)
    dm = g.DeviceMatrix.from_host(X)
    Q = X[:3].copy()
    cand = np.asarray([[0, 1, 2], [3, 10, 4], [5, 6, -1]], np.int32)             # 10 == n
    with pytest.raises(ValueError, match="row 10 out of range"):
        g.refine_topk(dm, Q, cand, 2)
    cand[1, 1] = 9
    rows, dist, counts = g.refine_topk(dm, Q, cand, 2)
    assert counts.tolist() == [2, 2, 2] and rows.tolist() == [[0, 1], [3, 4], [5, 6]]
    with pytest.raises(ValueError, match="outside the row map"):
        g.refine_topk(dm, Q, cand, 2, row_map=np.arange(9, dtype=np.int32))      # candidate 9, a map of 9 entries
    for bad in (10, -1):
        rmap = np.arange(10, dtype=np.int32)
        rmap[5] = bad
        with pytest.raises(ValueError, match="out of range"):
            g.refine_topk(dm, Q, cand, 2, row_map=rmap)
    for k in (0, 4):                                                             # 1 <= k <= c
        with pytest.raises(ValueError):
            g.refine_topk(dm, Q, cand, k)
    with pytest.raises(NotImplementedError):
        g.refine_topk(dm, Q, np.zeros((3, 8192), np.int32), 1)
    assert [a.shape for a in g.refine_topk(dm, Q[:0], cand[:0], 2)] == [(0, 2), (0, 2), (0,)]
    dm.close()


@pytest.mark.parametrize("d,c,k", [(48, 100, 10), (7, 1000, 200)])
def test_device_form_on_a_stream_equals_the_host_form(g, d, c, k):
    import torch
    N = g.native
    n, b = 2000, 33
    rng = np.random.default_rng(c)
    X = _data(d, n, rng)
    Q = rng.standard_normal((b, d)).astype(np.float32)
    cand = _lists(b, c, n, rng)
    perm = rng.permutation(n).astype(np.int32)
    shuffled = np.empty_like(X)
    shuffled[perm] = X
    dm = g.DeviceMatrix.from_host(shuffled)
    host = g.refine_topk(dm, Q, cand, k, row_map=perm)
    dev = torch.device("cuda:0")
    tq, tc, tm = (torch.from_numpy(a).to(dev) for a in (Q, cand, perm))
    oi = torch.full((b, k), -7, dtype=torch.int32, device=dev)
    od = torch.full((b, k), -7.0, dtype=torch.float32, device=dev)
    oc = torch.full((b,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        N.check(N.lib().gulon_refine_topk_dev(dm._h, tq.data_ptr(), b, tc.data_ptr(), c, tm.data_ptr(), n, k,
                                              oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                              C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    assert np.array_equal(oc.cpu().numpy(), host[2]) and np.array_equal(oi.cpu().numpy(), host[0])
    assert np.array_equal(od.cpu().numpy().view(np.uint32), host[1].view(np.uint32))
    # the status word: a candidate outside the map marks its query with -1 and leaves the others alone
    tc[5, 0] = n
    with torch.cuda.stream(stream):
        N.check(N.lib().gulon_refine_topk_dev(dm._h, tq.data_ptr(), b, tc.data_ptr(), c, tm.data_ptr(), n, k,
                                              oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                              C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    counts = oc.cpu().numpy()
    assert counts[5] == -1 and np.array_equal(np.delete(counts, 5), np.delete(host[2], 5))
    dm.close()


# ---- end to end: indexes built from one set of vectors, at the shapes tests/test_gpu_recall.py uses -----------------

def _vectors():
    """Three clusters whose rows lie at log-uniform scales 0.25 .. 4 around their centre.  A query next to a centre then
    sees its thousand nearest rows over a wide RANGE of distances; a narrow band of a thousand binary32 sums holds an
    equal pair for one query in six (tests/test_gpu_recall.py counts them), this one for one in a hundred."""
    rng = np.random.default_rng(32)
    centres = rng.uniform(-4, 4, (3, DIM))
    scale = np.exp(rng.uniform(np.log(0.25), np.log(4), (N_ROWS, 1)))
    x = centres[rng.integers(0, 3, N_ROWS)] + rng.normal(0, 1, (N_ROWS, DIM)) * scale
    X = np.asarray([[float("%.6f" % v) for v in row] for row in x], np.float32)
    r5 = np.random.default_rng(5)
    Q = (centres[r5.integers(0, 3, QUERIES)] + r5.normal(0, 0.05, (QUERIES, DIM))).astype(np.float32)
    return X, Q, [f"w{i:05d}" for i in range(N_ROWS)]              # the words ascend: word order = row order


@pytest.fixture(scope="module")
def world(g, oracle):
    """name -> (WordIndex, the DeviceWordVectors to refine against, their host copy, the prepared queries)."""
    from gulon_amd.build import Partitioned, build_index
    from gulon_amd.product_quantizer import Config
    from gulon_amd.word_vectors import DeviceWordVectors, KeyIndexSorted
    X, Q, words = _vectors()
    Xn = np.stack([oracle.normalize(r) for r in X])
    Qn = np.stack([oracle.normalize(r) for r in Q])
    out = {"raw": DeviceWordVectors(words, g.DeviceMatrix.from_host(X), KeyIndexSorted(words)), "X": X, "Q": Q}
    for name, metric, part, V, prepared in (("l2", "l2", None, X, Q), ("cosine", "cosine", None, Xn, Qn),
                                            ("grouped", "l2", Partitioned(12, 3), X, Q)):
        vectors = DeviceWordVectors(words, g.DeviceMatrix.from_host(V), KeyIndexSorted(words))
        index_words, index = build_index(vectors, metric, part, Config(K, M, ITERS))
        out[name] = (g.WordIndex(index_words, index), vectors, V, prepared)
    return out


def _oracle_candidates(oracle, index, prepared, c):
    ix = index.index
    if index._grouped:
        return oracle.grouped_query(ix.data.indices(), DIM, K, ix.quantizer.flat_centroids(), ix.centroids, ix.offsets,
                                    prepared, c, 0, ix.strategy.count)
    vi = ix.vector_index
    return oracle.pq_batch_query(vi.data.indices(), DIM, K, vi.product_quantizer.flat_centroids(), prepared, c)


@pytest.mark.parametrize("name", ["l2", "cosine", "grouped"])
def test_refined_index_equals_the_composition(g, oracle, world, name):
    N = g.native
    index, vectors, V, prepared = world[name]
    Q = world["Q"]
    refined = index.refined(vectors, 50)
    row_of = {w: i for i, w in enumerate(vectors.words)}
    row_map = np.asarray([row_of[w] for w in index.words], np.int32)
    assert (name == "grouped") == (not np.array_equal(row_map, np.arange(N_ROWS)))
    for k, c in CASES:
        c_eff = max(c, k)
        oi, od, oc = _oracle_candidates(oracle, index, prepared, c_eff + 1)
        # the oracle's own lists: how many hold an equal pair among their c_eff + 1 nearest (known without a device)
        tied = [q for q in range(QUERIES) if (np.diff(od[q, :oc[q]]) == 0).any()]
        assert len(tied) <= 0.05 * QUERIES or name == "grouped", (name, k, c, len(tied))    # (its heaps are literal)
        gi, _, gc, flags = index.batch_query_raw(c_eff, Q)
        own = (flags & (N.FLAG_BOUNDARY_TIE | N.FLAG_INTERIOR_TIE) != 0) & (flags & N.FLAG_EXACT_REPLAY == 0)
        print(name, k, c, "oracle lists with a tie:", len(tied), "queries fed the device's own list:", int(own.sum()))
        assert own.sum() <= 0.05 * QUERIES, (name, k, c, int(own.sum()))
        want = []
        for q in range(QUERIES):
            cand = gi[q, :gc[q]] if own[q] else oi[q, :min(oc[q], c_eff)]
            want.append(_restate(oracle, k, prepared[q], cand, V, row_map))
        got = refined.batch_query_raw(k, Q, candidates=c)
        assert np.array_equal(got[3], flags)
        _assert_equal(got[:3], want, (name, k, c))
        assert all(len(w[0]) == min(k, N_ROWS) for w in want) or name == "grouped"
    # the other entry points are the same results with their words
    k, c = 10, 100
    rows, dist, counts, _ = refined.batch_query_raw(k, Q[:9], candidates=c)
    results = refined.batch_query(k, Q[:9], candidates=c)
    assert [r.rows.tolist() for r in results] == [rows[q, :counts[q]].tolist() for q in range(9)]
    assert results[0].words == [index.words[i] for i in rows[0, :counts[0]]]
    one = refined.query(k, Q[3], candidates=c)
    assert one.rows.tolist() == results[3].rows.tolist() and np.array_equal(bits(one.distances), bits(results[3].distances))
    assert [r.rows.tolist() for r in index.refined(vectors, c).batch_query(k, Q[:9])] == [r.rows.tolist() for r in results]
    # by word: the index's decoded vector as the query, re-ranked against the originals
    asked = [index.words[5], "no such word", index.words[4000]]
    by_word = refined.batch_query_by_words(k, asked, candidates=c)
    assert by_word[1] is None and refined.query_by_word(k, asked[2], candidates=c).rows.tolist() == by_word[2].rows.tolist()
    for word, res in ((asked[0], by_word[0]), (asked[2], by_word[2])):
        decoded = index.lookup(word)
        if index.metric == "cosine":
            decoded = oracle.normalize(decoded)
        plain = index.query_by_word(c, word)
        ids, ds = _restate(oracle, k, decoded, plain.rows, V, row_map)
        assert res.rows.tolist() == ids.tolist() and np.array_equal(bits(res.distances), bits(ds))
    refined.close()


def test_refined_index_needs_every_word_and_keeps_the_library_limits(g, world):
    from gulon_amd.word_vectors import DeviceWordVectors, KeyIndexSorted
    index, vectors, V, _ = world["l2"]
    fewer = DeviceWordVectors(vectors.words[1:], g.DeviceMatrix.from_host(V[1:]), KeyIndexSorted(vectors.words[1:]))
    with pytest.raises(LookupError, match="the index holds the word 'w00000', the word vectors do not"):
        index.refined(fewer, 10)
    grouped, gvec, _, _ = world["grouped"]
    refined = grouped.refined(gvec, 2049)                          # a grouped index answers up to 2048: never clamped
    with pytest.raises(NotImplementedError, match="k_nn = 2049 > 2048 is not supported by the grouped index"):
        refined.batch_query_raw(10, world["Q"][:2])
    refined.close()


def _distances(X, Q, rows):
    safe = np.where(rows >= 0, rows, 0)
    acc = np.zeros(rows.shape, np.float32)
    for i in range(X.shape[1]):
        dx = Q[:, i][:, None] - X[safe, i]
        acc = acc + dx * dx
    return np.where(rows >= 0, acc, F(0))


@pytest.mark.parametrize("name", ["l2", "cosine", "grouped"])
def test_recall_of_the_refined_index(g, world, name):
    """Tests.recall_of over a RefinedIndex equals the numpy restatement fed the refined results; the recall distances
    are taken on the RAW vectors, for the cosine index too (Test.scala:48).
    And no query loses a hit at any k against the plain index: the plain first k are among the candidates, the refined
    first k are the k nearest of them.  That argument speaks of the distances the candidates are RE-RANKED by -- from
    the query as the index prepares it to the vectors the index is refined over -- so the hits of both results are
    counted with those: for the cosine index the normalised query and vectors, not the raw ones of the recall figures
    (where a refined cosine result can lose a hit: the two metrics order the rows differently; the count is printed)."""
    from gulon_amd import tests_recall as tr
    from gulon_amd.index import normalize
    index, vectors, _, _ = world[name]
    raw, X = world["raw"], world["X"]
    tests = tr.Tests.sample(raw, 100)
    refined = index.refined(vectors, 1000)
    seen = {}

    def recording(key):
        def evaluate(*args):
            seen.setdefault(key, []).append(tr.recall_counts(*args))
            return seen[key][-1]
        return evaluate
    plain = tests.recall_of(index, evaluate=recording("plain"))
    got = tests.recall_of(refined, evaluate=recording("refined"))
    assert sorted(got) == list(tr.DEFAULT_KS)
    rows, _, counts, _ = refined.batch_query_raw(1000, tests.queries)
    assert vectors.words == raw.words
    row_of = {w: i for i, w in enumerate(raw.words)}
    row_map = np.asarray([row_of[w] for w in index.words], np.int32)

    def vector_rows(r):
        return np.where(r >= 0, row_map[np.where(r >= 0, r, 0)], -1).astype(np.int32)
    vrows = vector_rows(rows)
    dist = _distances(X, tests.queries, vrows)
    for j, k in enumerate(tr.DEFAULT_KS):
        tp = ((vrows[:, :k] >= 0) & (dist[:, :k] <= tests.kth[:, j][:, None])).sum(axis=1)
        want = tr.fold(tp.astype(np.float32) / F(k))
        print(name, k, "plain", plain[k].mean, "refined", got[k].mean)
        assert got[k].count == want.count == 100
        assert bits(got[k].mean) == bits(want.mean) and bits(got[k].s) == bits(want.s), (name, k)
    raw_plain, raw_refined = np.concatenate(seen["plain"]), np.concatenate(seen["refined"])
    assert raw_plain.shape == raw_refined.shape == (100, len(tr.DEFAULT_KS))
    print(name, "(query, k) pairs that lose a hit on the raw vectors:", int((raw_refined < raw_plain).sum()))
    # the hits in the metric of the re-ranking
    prepared = np.stack([normalize(r) for r in tests.queries]) if index.metric == "cosine" else tests.queries
    own = tr.Tests.for_queries(vectors, prepared)
    ks = np.asarray(own.ks, np.int32)
    tp_plain = tr.recall_counts(vectors.matrix, prepared, vector_rows(index.batch_query_raw(1000, tests.queries)[0]), ks,
                                own.kth)
    tp_refined = tr.recall_counts(vectors.matrix, prepared, vrows, ks, own.kth)
    if index.metric != "cosine":                                   # the same vectors and queries: the same counts
        assert np.array_equal(tp_plain, raw_plain) and np.array_equal(tp_refined, raw_refined)
    assert (tp_refined >= tp_plain).all()
    assert (tp_refined > tp_plain).any()
    refined.close()
