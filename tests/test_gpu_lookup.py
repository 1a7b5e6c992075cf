"""Decoding stored rows and querying by them on the device (decode.hip): ProductQuantizer.decode
(ProductQuantizer.scala:37-78), GroupedIndex.lookup (Index.scala:247-253, with the reference's Arrays.binarySearch
partition rule), Index.queryByWord (Index.scala:38-45) on row ids, WordIndex over a saved index file, and the
`python -m gulon_amd` query commands -- against the CPU oracle, bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, bits
from test_gpu_query import _check, _make

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def java_binary_search(a, key):
    """java.util.Arrays.binarySearch(int[], int), literally."""
    low, high = 0, len(a) - 1
    while low <= high:
        mid = (low + high) >> 1
        v = int(a[mid])
        if v < key:
            low = mid + 1
        elif v > key:
            high = mid - 1
        else:
            return mid
    return -(low + 1)


def ref_partition(offsets, row):
    i = java_binary_search(offsets, row)
    return -i - 1 if i < 0 else i + 1


def ref_lookup(oracle, codes, d, k, pq_cents, group_centroids, offsets, rows):
    """GroupedIndex.lookup (Index.scala:247-253): centroids(partition) + decode(row), one fp32 add."""
    dec = oracle.pq_decode(codes, d, k, pq_cents)
    gc = np.asarray(group_centroids, np.float32)
    return np.stack([gc[ref_partition(offsets, int(r))] + dec[int(r)] for r in rows]).astype(np.float32) \
        if len(rows) else np.zeros((0, d), np.float32)


def _rows(n, rng, extra=()):
    """random rows, the first and last, rows of the last (partial) 64-row block, repeated ids"""
    r = list(rng.integers(0, n, 20)) + [0, n - 1, max(0, n - 3), n - 1, 0] + [(n // 64) * 64 + i for i in range(3)
                                                                          if (n // 64) * 64 + i < n] + list(extra)
    return np.asarray(r, np.int32)


def _canon(a):
    """distance bits with every NaN as the same NaN (the reference's Float comparisons do not see NaN payloads)"""
    a = np.array(a, np.float32)
    a[np.isnan(a)] = np.float32("nan")
    return bits(a)


# ---------------------------------------------------------------- 1. row decode
@pytest.mark.parametrize("n,d,m,k", [(1000, 128, 16, 256), (777, 100, 25, 256), (500, 32, 8, 16), (130, 12, 6, 4),
                                     (65, 8, 4, 1), (3000, 64, 16, 1024), (300, 16, 4, 65536)])
def test_decode_rows_equals_oracle(oracle, g, n, d, m, k):
    cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=n + k)
    ix = g.PQIndex(pq, enc)
    rows = _rows(n, np.random.default_rng(k))
    out = ix.decode_rows(rows)
    want = oracle.pq_decode(idx, d, k, cents)[rows]
    assert np.array_equal(bits(out), bits(want))
    for r, o in zip(rows[:6], out[:6]):                 # the host gather as a second check
        assert np.array_equal(bits(o), bits(ix.decode(int(r))))
    assert ix.decode_rows(np.zeros(0, np.int32)).shape == (0, d)
    ix.close()


def test_decode_rows_normalised_equals_oracle(oracle, g):
    n, d, m, k = 900, 48, 12, 256
    cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=11)
    ix = g.PQIndex(pq, enc)
    rows = _rows(n, np.random.default_rng(2))
    dec = oracle.pq_decode(idx, d, k, cents)
    want = np.stack([oracle.normalize(dec[r]) for r in rows])
    assert np.array_equal(bits(ix.decode_rows(rows, normalize=True)), bits(want))
    ix.close()


# ---------------------------------------------------------------- 2. bulk decode
@pytest.mark.parametrize("n,d,m,k,frm,until", [(1000, 128, 16, 256, 0, None), (1000, 128, 16, 256, 70, 999),
                                               (777, 100, 25, 256, 63, 65), (500, 30, 7, 16, 1, 129),
                                               (3000, 64, 16, 1024, 100, 2950), (200, 8, 4, 1, 0, None),
                                               (300, 16, 4, 65536, 5, 300), (640, 32, 8, 4, 128, 128)])
def test_decode_matrix_equals_host_decode(oracle, g, n, d, m, k, frm, until):
    cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=n + d)
    ix = g.PQIndex(pq, enc)
    until_ = n if until is None else until
    dm = ix.decode_matrix(frm, until)
    assert (dm.rows, dm.cols) == (until_ - frm, d)
    want = pq.decode(enc).data[frm:until_]
    assert np.array_equal(bits(dm.to_host()), bits(want))
    assert np.array_equal(bits(want), bits(oracle.pq_decode(idx, d, k, cents)[frm:until_]))
    dm.close()
    ix.close()


# ---------------------------------------------------------------- 3. grouped lookup
REPEATED_OFFSETS = [0, 5, 5, 5, 5, 5, 9, 9, 9, 40, 40, 100, 150, 150, 150, 150, 220]


def _direct_grouped(g, n, d, m, k, offsets, seed, strategy=None, metric="l2", dup=0):
    """A GroupedIndex built directly from random residual codes, group centroids and (repeating) offsets."""
    rng = np.random.default_rng(seed)
    cents = rng.standard_normal(k * d).astype(np.float32)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    if dup:
        idx[:, -dup:] = idx[:, :dup]
    gc = (rng.standard_normal((len(offsets) + 1, d)) * 3).astype(np.float32)
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    coder = pq.coder_factory(n)
    enc = g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(m)])
    gx = g.GroupedIndex(pq, enc, gc, np.asarray(offsets, np.int32), strategy or g.LimitGroups(4), metric)
    return gx, cents, idx, gc


@pytest.mark.parametrize("k", [16, 256, 1024])
def test_grouped_lookup_uses_the_reference_partition(oracle, g, k):
    n, d, m = 300, 16, 4
    gx, cents, idx, gc = _direct_grouped(g, n, d, m, k, REPEATED_OFFSETS, seed=k)
    rows = np.arange(n, dtype=np.int32)
    offsets = np.asarray(REPEATED_OFFSETS, np.int32)
    own = np.searchsorted(offsets, rows, side="right")
    ref = np.array([ref_partition(offsets, int(r)) for r in rows])
    assert (own != ref).any()                     # the binarySearch quirk is exercised
    out = gx.lookup_rows(rows)
    assert np.array_equal(bits(out), bits(ref_lookup(oracle, idx, d, k, cents, gc, offsets, rows)))
    for r in (5, 40, 150, 0, n - 1):
        assert np.array_equal(bits(gx.lookup_row(r)), bits(out[r]))
    gx.close()


def test_grouped_lookup_of_the_pipeline(oracle, g):
    from test_gpu_grouped import _build
    n, d, groups, m, k = 6000, 16, 12, 4, 16
    X, dm, coarse, gv, pq = _build(oracle, g, n, d, groups, m, k, seed=n + d)
    index = g.Index.grouped(gv, pq, g.LimitGroups(3))
    rows = _rows(n, np.random.default_rng(4), extra=list(gv.offsets[:6]))
    want = ref_lookup(oracle, index.data.indices(), d, k, pq.flat_centroids(), gv.centroids, gv.offsets, rows)
    assert np.array_equal(bits(index.lookup_rows(rows)), bits(want))
    index.close()


# ---------------------------------------------------------------- 4. query by rows
def _same(a, b):
    (ai, ad, ac, af), (bi, bd, bc, bf) = a, b
    assert np.array_equal(ac, bc) and np.array_equal(af, bf)
    for q in range(len(ac)):
        assert ai[q, :ac[q]].tolist() == bi[q, :bc[q]].tolist(), q
        assert np.array_equal(_canon(ad[q, :ac[q]]), _canon(bd[q, :bc[q]])), q


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("K", [1, 10, 100])
@pytest.mark.parametrize("frm,until", [(0, None), (130, 4000)])
def test_sorted_query_rows_equals_host_lookup_and_oracle(oracle, g, metric, K, frm, until):
    n, d, m, k = 5000, 32, 8, 64
    rng = np.random.default_rng(K)
    cents = rng.standard_normal(k * d).astype(np.float32)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    idx[:, -600:] = idx[:, :600]                        # exact duplicate rows: ties, the replay runs
    zero = 7
    fr, un = oracle.subvectors(d, m)
    for j in range(m):                                  # centroid 0 of every quantizer is 0; row `zero` decodes to 0
        cents[k * fr[j]:k * fr[j] + (un[j] - fr[j])] = 0
    idx[:, zero] = 0
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    coder = pq.coder_factory(n)
    enc = g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(m)])
    index = g.SortedIndex(g.PQIndex(pq, enc), metric)
    rows = np.r_[_rows(n, rng, extra=[n - 1, 3]), zero].astype(np.int32)
    cos = metric == "cosine"
    vi = index.vector_index
    got = vi.batch_query_rows_raw(K, rows, frm, until, normalize=cos)
    host = np.stack([vi.decode(int(r)) for r in rows])
    Q = index._prepare(host)                            # SortedIndex.prepare: the host normalisation
    _same(got, vi.batch_query_raw(K, Q, frm, until))
    res = index.batch_query_rows(K, rows) if (frm, until) == (0, None) else vi.batch_query_rows(K, rows, frm, until, cos)
    dec = oracle.pq_decode(idx, d, k, cents)[rows]
    Qo = np.stack([oracle.normalize(r) for r in dec]) if cos else dec
    live = [i for i, r in enumerate(rows) if not (cos and r == zero)]
    oi, od, oc = oracle.pq_batch_query(idx, d, k, cents, Qo[live], K, frm, n if until is None else until)
    _check(oracle, [res[i] for i in live], oi, od, oc)
    index.vector_index.close()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("strategy,limit,K", [("groups", 3, 1), ("groups", 5, 10), ("vectors", 900, 100),
                                              ("groups", 12, 1000)])
def test_grouped_query_rows_of_the_pipeline(oracle, g, metric, strategy, limit, K):
    from test_gpu_grouped import _build
    n, d, groups, m, k = 8000, 24, 10, 6, 64
    X, dm, coarse, gv, pq = _build(oracle, g, n, d, groups, m, k, seed=8024, dup=1500)
    strat = g.LimitGroups(limit) if strategy == "groups" else g.LimitVectors(limit)
    index = g.Index.grouped(gv, pq, strat, metric)
    rng = np.random.default_rng(K)
    rows = _rows(n, rng, extra=[n - 1500, 0])
    codes = index.data.indices()
    look = ref_lookup(oracle, codes, d, k, pq.flat_centroids(), gv.centroids, gv.offsets, rows)
    oi, od, oc = index.batch_query_rows_raw(K, rows)
    hi, hd, hc = index.batch_query_raw(K, look)
    z = np.zeros(len(rows), np.int32)
    _same((oi, od, oc, z), (hi, hd, hc, z))
    Qo = np.stack([oracle.normalize(r) for r in look]) if metric == "cosine" else look
    ei, ed, ec = oracle.grouped_query(codes, d, k, pq.flat_centroids(), gv.centroids, gv.offsets, Qo, K,
                                      0 if strategy == "groups" else 1, limit)
    assert np.array_equal(oc, ec)
    for q in range(len(rows)):
        assert oi[q, :oc[q]].tolist() == ei[q, :ec[q]].tolist(), q
        assert np.array_equal(bits(od[q, :oc[q]]), bits(ed[q, :ec[q]])), q
    res = index.batch_query_rows(K, rows)
    assert [r.rows.tolist() for r in res] == [oi[q, :oc[q]].tolist() for q in range(len(rows))]
    index.close()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("k,strategy,limit,K", [(16, "groups", 4, 10), (16, "vectors", 60, 5), (256, "groups", 18, 1),
                                                (1024, "groups", 3, 10)])
def test_grouped_query_rows_with_repeated_offsets(oracle, g, metric, k, strategy, limit, K):
    n, d, m = 300, 16, 4
    strat = g.LimitGroups(limit) if strategy == "groups" else g.LimitVectors(limit)
    gx, cents, idx, gc = _direct_grouped(g, n, d, m, k, REPEATED_OFFSETS, seed=k + K, strategy=strat, metric=metric,
                                         dup=40)
    offsets = np.asarray(REPEATED_OFFSETS, np.int32)
    rows = np.asarray([5, 9, 40, 150, 0, 299, 3, 5, 220, 100, 270], np.int32)
    assert any(ref_partition(offsets, int(r)) != np.searchsorted(offsets, r, side="right") for r in rows)
    look = ref_lookup(oracle, idx, d, k, cents, gc, offsets, rows)
    oi, od, oc = gx.batch_query_rows_raw(K, rows)
    hi, hd, hc = gx.batch_query_raw(K, look)
    z = np.zeros(len(rows), np.int32)
    _same((oi, od, oc, z), (hi, hd, hc, z))
    Qo = np.stack([oracle.normalize(r) for r in look]) if metric == "cosine" else look
    ei, ed, ec = oracle.grouped_query(idx, d, k, cents, gc, offsets, Qo, K, 0 if strategy == "groups" else 1, limit)
    assert np.array_equal(oc, ec)
    for q in range(len(rows)):
        assert oi[q, :oc[q]].tolist() == ei[q, :ec[q]].tolist(), q
        assert np.array_equal(bits(od[q, :oc[q]]), bits(ed[q, :ec[q]])), q
    gx.close()


# ---------------------------------------------------------------- 5. out-of-range rows
def test_out_of_range_rows_are_rejected(oracle, g):
    from gulon_amd import native as N
    n, d, m, k = 200, 16, 4, 16
    cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=3)
    ix = g.PQIndex(pq, enc)
    gx, _, _, _ = _direct_grouped(g, n, d, m, k, [0, 50, 50, 120], seed=3)
    for bad in ([n], [-1], [0, 5, n + 100]):
        with pytest.raises(ValueError):
            ix.decode_rows(bad)
        with pytest.raises(ValueError):
            ix.batch_query_rows(3, bad)
        with pytest.raises(ValueError):
            gx.lookup_rows(bad)
        with pytest.raises(ValueError):
            gx.batch_query_rows(3, bad)
    with pytest.raises(ValueError):
        ix.decode_matrix(0, n + 1)
    with pytest.raises(ValueError):
        ix.decode_matrix(10, 5)
    err = C.c_int32(-1)
    N.check(N.lib().gulon_index_row_error(ix._h, C.byref(err)))
    assert err.value == 0                               # nothing was launched for them
    # the device form cannot check on the host: an out-of-range row decodes to NaN and sets the row-error word
    rows = np.array([3, n, -7, 0], np.int32)
    d_rows, d_out = C.c_void_p(), C.c_void_p()
    N.check(N.lib().gulon_dev_malloc(C.byref(d_rows), rows.nbytes))
    N.check(N.lib().gulon_dev_malloc(C.byref(d_out), 4 * d * len(rows)))
    try:
        N.check(N.lib().gulon_memcpy_h2d(d_rows, rows.ctypes.data, rows.nbytes))
        for h, fn, ferr in ((ix._h, "gulon_index_decode_rows_dev", "gulon_index_row_error"),
                            (gx._h, "gulon_grouped_index_lookup_rows_dev", "gulon_grouped_index_row_error")):
            N.check(getattr(N.lib(), fn)(h, d_rows, len(rows), 0, d_out, None))
            N.check(N.lib().gulon_device_synchronize())
            out = np.zeros((len(rows), d), np.float32)
            N.check(N.lib().gulon_memcpy_d2h(out.ctypes.data, d_out, out.nbytes))
            assert np.isnan(out[1:3]).all() and not np.isnan(out[[0, 3]]).any()
            N.check(getattr(N.lib(), ferr)(h, C.byref(err)))
            assert err.value == 1
            N.check(getattr(N.lib(), ferr)(h, C.byref(err)))
            assert err.value == 0
    finally:
        N.lib().gulon_dev_free(d_rows)
        N.lib().gulon_dev_free(d_out)
    ix.close()
    gx.close()


# ---------------------------------------------------------------- 6. WordIndex
def _word_indexes(g, oracle):
    """(kind, WordIndex, restated lookup of every row, oracle query function) for a sorted and a grouped index"""
    from gulon_amd.index_file import dump_index
    from gulon_amd.word_index import WordIndex
    out = []
    n, d, m, k = 2000, 16, 4, 32
    cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=21, dup=200)
    words = [f"w{i:05d}" for i in range(n)]                  # String order = row order
    srt = g.SortedIndex(g.PQIndex(pq, enc), "l2")
    wi = WordIndex.load(dump_index(srt, words))
    dec = oracle.pq_decode(idx, d, k, cents)
    out.append(("sorted", wi, words, dec, lambda Q, K: oracle.pq_batch_query(idx, d, k, cents, Q, K)))
    srt.vector_index.close()
    offsets = [0, 300, 300, 900, 1500]
    gx, gcents, gidx, gc = _direct_grouped(g, n, d, m, k, offsets, seed=22, strategy=g.LimitGroups(3), metric="cosine")
    rng = np.random.default_rng(5)
    gwords = [None] * n
    names = [f"g{i:05d}" for i in rng.permutation(n)]
    for a, b in zip([0] + offsets, offsets + [n]):          # keys sorted inside every group (KeyIndex.Grouped)
        gwords[a:b] = sorted(names[a:b])
    wg = WordIndex.load(dump_index(gx, gwords))
    look = ref_lookup(oracle, gidx, d, k, gcents, gc, offsets, np.arange(n))
    out.append(("grouped", wg, gwords, look,
                lambda Q, K: oracle.grouped_query(gidx, d, k, gcents, gc, np.asarray(offsets, np.int32),
                                                  np.stack([oracle.normalize(r) for r in Q]), K, 0, 3)))
    gx.close()
    return out


def test_word_index_lookup_and_query_by_words(oracle, g):
    K = 5
    for kind, wi, words, look, oq in _word_indexes(g, oracle):
        n = len(words)
        assert wi.lookup("absent") is None
        for r in (0, 17, n - 1, 300, 299):
            assert np.array_equal(bits(wi.lookup(words[r])), bits(look[r])), (kind, r)
        qwords = [words[3], "nope", words[n - 1], words[3], "", words[300], words[1999], "w", words[299]]
        got = wi.batch_query_by_words(K, qwords)
        loop = [wi.query_by_word(K, w) for w in qwords]
        assert [r is None for r in got] == [w not in set(words) for w in qwords]
        for a, b in zip(got, loop):
            assert (a is None) == (b is None)
            if a is not None:
                assert a.words == b.words and np.array_equal(bits(a.distances), bits(b.distances))
        present = [(w, r) for w, r in zip(qwords, got) if r is not None]
        rows = [words.index(w) for w, _ in present]
        oi, od, oc = oq(look[rows], K)
        for q, (w, r) in enumerate(present):
            assert r.rows.tolist() == oi[q, :oc[q]].tolist(), (kind, w)
            assert r.words == [words[i] for i in oi[q, :oc[q]]]
            assert np.array_equal(bits(r.distances), bits(od[q, :oc[q]]))
        wi.close()


# ---------------------------------------------------------------- 7. CLI
def _run_cli(args, stdin=None):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "gulon_amd"] + args, input=stdin, capture_output=True, cwd=ROOT, env=env,
                       timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")
    return p.stdout


def test_cli_query_words_and_query(oracle, g, tmp_path):
    from gulon_amd.index_file import dump_index
    from gulon_amd.word_index import WordIndex
    K = 3
    for kind, wi, words, look, oq in _word_indexes(g, oracle):
        path = tmp_path / f"{kind}.index"
        path.write_bytes(dump_index(wi.index, words))
        qwords = [words[10], "not-a-word", words[10], words[-1], words[300]]
        want = "".join(f"{w}: not found\n" if r is None else f"{w}: {','.join(r.words)}\n"
                       for w, r in zip(qwords, wi.batch_query_by_words(K, qwords))).encode()
        qfile = tmp_path / f"{kind}.words"
        qfile.write_bytes("\r\n".join(qwords).encode() + b"\r\n")
        assert _run_cli(["query-words", "-i", str(path), "-k", str(K), str(qfile)]) == want
        assert _run_cli(["query-words", "-k", str(K), "-i", str(path)], stdin="\n".join(qwords).encode()) == want
        # query: a word2vec text file of query vectors
        vecs = look[[1, 2, 300]]
        text = "3 16\n" + "".join(f"q{i} " + " ".join(np.format_float_positional(x, unique=True) for x in v) + "\n"
                                  for i, v in enumerate(vecs))
        vfile = tmp_path / f"{kind}.vec"
        vfile.write_text(text)
        res = wi.batch_query(K, vecs)
        want = "".join(f"q{i}: {','.join(r.words)}\n" for i, r in enumerate(res)).encode()
        assert _run_cli(["query", "-i", str(path), "-k", str(K), str(vfile)]) == want
        wi.close()
