"""Index updates on the device (update.hip): encoding against an index's own code books, combining the code buffers of
two indexes, and reading codes back.

The contract: the reference has no mutation, so everything is stated through what it has.  PQIndex.encode(X) is
PQIndex(pq, pq.encode(X)) -- `oracle.pq_encode` bit for bit, tie-break stream included; PQIndex.merged is the PQIndex over
the numpy gather of the two code arrays -- `oracle.pq_batch_query` on it, and a natively created index of those codes."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits
from test_gpu_query import _check, _make
from test_gpu_subset import LAYOUTS as BYTE_LAYOUTS, _filter_stats

pytestmark = pytest.mark.gpu

ENCODE_SHAPES = [(1, 8, 4, 16),                                          # a single row
                 (63, 26, 4, 16), (64, 26, 4, 16), (65, 26, 4, 16),      # ragged last block, uneven sub-vectors, 4-bit codes
                 (1000, 32, 16, 256),                                    # one 16-byte word per row
                 (1000, 32, 8, 256),                                     # two 4-byte words
                 (1000, 40, 20, 64),                                     # ng > 1 with padding
                 (5000, 128, 16, 256),                                   # the benchmark's sub-vector shape (MFMA assign)
                 (1000, 32, 8, 1024),                                    # wide codes
                 (0, 16, 4, 16)]                                         # no rows
LAYOUTS = dict(BYTE_LAYOUTS, wide=(1000, 32, 8, 1024))
NA, NB = 1000, 130


def _interleaving(length, seed):
    """`length` entries drawn from both sources, in no order: >= 0 rows of a, < 0 row -1 - e of b."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(length) < 0.7, rng.integers(0, NA, length), -1 - rng.integers(0, NB, length))


TAKES = {
    "empty": (np.zeros(0, np.int64), True),
    "one_of_b": (np.array([-1 - 77]), True),
    "all_a_then_all_b": (np.concatenate([np.arange(NA), -1 - np.arange(NB)]), True),
    "mix63": (_interleaving(63, 63), True),
    "mix64": (_interleaving(64, 64), True),
    "mix65": (_interleaving(65, 65), True),
    "mix1130": (_interleaving(1130, 1130), True),
    "repeats": (np.array([5, 5, -3, 5, -3, 999, 0, 0, -130, -130, 64, 63, 64]), True),
    "a_alone_permuted": (np.random.default_rng(9).permutation(NA), False),     # b = NULL, not ascending
}


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def _native(g, pq, idx):
    """The index gulon_index_create makes of the codes idx [m][n]."""
    coder = pq.coder_factory(idx.shape[1])
    return g.PQIndex(pq, g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(idx.shape[0])]))


def _holder(g, pq):
    """An index of no rows that holds the quantizer on the device."""
    return _native(g, pq, np.zeros((len(pq.quantizers), 0), np.int32))


def _same_answers(x, y):
    assert np.array_equal(x[0], y[0]) and np.array_equal(bits(x[1]), bits(y[1]))
    assert np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3])


# ---------------------------------------------------------------- 1. encode_dataset
@pytest.mark.parametrize("n,d,m,k", ENCODE_SHAPES)
def test_encode_equals_the_reference(oracle, g, n, d, m, k):
    rng = np.random.default_rng(n * 7 + m + k)
    cents = rng.standard_normal(k * d).astype(np.float32)
    X = rng.standard_normal((n, d)).astype(np.float32)
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    holder = _holder(g, pq)
    enc = holder.encode(X)
    want = oracle.pq_encode(X, m, k, cents)
    assert isinstance(enc, g.DevicePQIndex) and enc.length == n and enc.row_base == 0
    got = enc.indices()
    assert got.shape == (m, n) and got.dtype == np.int32
    assert np.array_equal(got, want)
    # the lazily built EncodedMatrix is the one ProductQuantizer.encode gives
    assert enc.data == pq.encode(X)
    holder.close()                                              # the encoded index owns its code books
    native = _native(g, pq, want)
    Q = rng.standard_normal((6, d)).astype(np.float32)
    for K in (1, 10, 63, 100):
        _same_answers(enc.batch_query_raw(K, Q), native.batch_query_raw(K, Q))
        if n:
            _check(oracle, enc.batch_query(K, Q), *oracle.pq_batch_query(want, d, k, cents, Q, K))
    native.close()
    enc.close()


def test_encode_draws_the_reference_tie_break_stream(oracle, g):
    """Code books in which several centroids are exact duplicates, rows that sit exactly on them: which duplicate a row
    gets is java.util.Random(0) per quantizer, over the rows in order."""
    n, d, m, k = 700, 16, 4, 16
    rng = np.random.default_rng(31)
    pq0 = g.ProductQuantizer.from_flat(k, d, m, rng.standard_normal(k * d).astype(np.float32))
    for q in pq0.quantizers:
        c = q.clusters.centroids
        c[[3, 7, 11]] = c[1]                                    # four copies of one centroid
        c[14] = c[2]                                            # and two of another
    cents = pq0.flat_centroids()
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    X = oracle.pq_decode(idx, d, k, cents)                      # every slice of every row IS a centroid
    X[::5] += rng.standard_normal((len(X[::5]), d)).astype(np.float32)   # some rows off them: no draw there
    want = oracle.pq_encode(X, m, k, cents)
    assert len({int(v) for v in want[0][np.isin(idx[0], [1, 3, 7, 11])]}) > 1    # the draws do pick different copies
    holder = _holder(g, pq)
    enc = holder.encode(X)
    assert np.array_equal(enc.indices(), want)
    enc.close()
    holder.close()


def test_encode_errors(oracle, g):
    from gulon_amd import native as N
    n, d, m, k = 100, 16, 4, 16
    cents, idx, pq, encm = _make(oracle, g, n, d, m, k, seed=1)
    ix = g.PQIndex(pq, encm)
    with pytest.raises(ValueError, match="dimensions"):
        ix.encode(np.zeros((5, d + 1), np.float32))
    wrong = g.DeviceMatrix.from_host(np.zeros((5, d + 1), np.float32))
    out = C.c_void_p()
    L = N.lib()
    assert L.gulon_index_encode_dataset(ix._h, wrong._h, C.byref(out)) == N.ERR_INVALID_ARGUMENT
    assert "dimensions" in N.last_error() and not out.value
    assert L.gulon_index_encode_dataset(None, wrong._h, C.byref(out)) == N.ERR_INVALID_ARGUMENT
    assert L.gulon_index_encode_dataset(ix._h, None, C.byref(out)) == N.ERR_INVALID_ARGUMENT
    assert L.gulon_index_encode_dataset(ix._h, wrong._h, None) == N.ERR_INVALID_ARGUMENT
    wrong.close()
    ix.close()


# ---------------------------------------------------------------- 2. merge
_SOURCES = {}


def _sources(oracle, g, layout):
    """Per layout for the whole module: (cents, codes of a, codes of b, pq, a, b, queries)."""
    if layout not in _SOURCES:
        _, d, m, k = LAYOUTS[layout]
        cents, ia, pq, ea = _make(oracle, g, NA, d, m, k, seed=sum(map(ord, layout)))
        ib = np.random.default_rng(5).integers(0, k, (m, NB)).astype(np.int32)
        Q = np.random.default_rng(17).standard_normal((8, d)).astype(np.float32)
        _SOURCES[layout] = (cents, ia, ib, pq, g.PQIndex(pq, ea), _native(g, pq, ib), Q)
    return _SOURCES[layout]


def _gathered(ia, ib, take):
    take = np.asarray(take, np.int64)
    both = np.concatenate([ia, ib], axis=1)
    return np.ascontiguousarray(both[:, np.where(take >= 0, take, ia.shape[1] + (-1 - take))])


@pytest.mark.parametrize("take_name", list(TAKES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_merge_equals_a_natively_created_index(oracle, g, layout, take_name):
    _, d, m, k = LAYOUTS[layout]
    cents, ia, ib, pq, a, b, Q = _sources(oracle, g, layout)
    take, with_b = TAKES[take_name]
    s = len(take)
    merged = a.merged(b if with_b else None, take)
    assert isinstance(merged, g.DevicePQIndex) and not isinstance(merged, g.PQIndexView)
    assert merged.length == s and merged.row_base == 0
    want = _gathered(ia, ib, take)
    assert np.array_equal(merged.indices(), want)
    native = _native(g, pq, want)
    x, y = merged.decode_matrix(), native.decode_matrix()
    assert np.array_equal(bits(x.to_host()), bits(y.to_host()))
    x.close(), y.close()
    assert merged.data == native.data
    ranges = {(0, s), (min(s, 7), s), (max(s - 13, 0), s), (s // 64 * 64, s), (min(1, s), max(s - 1, min(1, s)))}
    for frm, until in sorted(ranges):                           # they cut the ragged last block
        for K in (10, 100):
            _same_answers(merged.batch_query_raw(K, Q, frm, until), native.batch_query_raw(K, Q, frm, until))
    if s:
        for K in (1, 10, 63, 100):
            _check(oracle, merged.batch_query(K, Q), *oracle.pq_batch_query(want, d, k, cents, Q, K))
    native.close()
    merged.close()


def test_merged_index_takes_the_filtered_path(oracle, g):
    n, nb, d, m, k, B, K = 150000, 20000, 128, 16, 256, 32, 10
    cents, ia, pq, ea = _make(oracle, g, n, d, m, k, seed=150)
    ib = np.random.default_rng(20).integers(0, k, (m, nb)).astype(np.int32)
    a, b = g.PQIndex(pq, ea), _native(g, pq, ib)
    rng = np.random.default_rng(47)
    slots = np.sort(rng.choice(n + nb, nb, replace=False))      # where b's rows land among a's
    take = np.zeros(n + nb, np.int64)
    from_b = np.zeros(n + nb, bool)
    from_b[slots] = True
    take[from_b] = -1 - rng.permutation(nb)
    take[~from_b] = np.arange(n)
    merged = a.merged(b, take)
    a.close(), b.close()                                        # the merged index owns what it reads
    want = np.ascontiguousarray(np.concatenate([ia, ib], axis=1)[:, np.where(take >= 0, take, n + (-1 - take))])
    s = n + nb
    Q = np.random.default_rng(8).standard_normal((B, d)).astype(np.float32)
    for frm, until in ((0, s), (1000, s - 777)):                # the second cuts 256-row ordering windows
        res = merged.batch_query(K, Q, frm, until)
        assert _filter_stats(merged)[0] > 0
        _check(oracle, res, *oracle.pq_batch_query(want, d, k, cents, Q, K, frm, until))
    assert np.array_equal(merged.indices(70000, 70300), want[:, 70000:70300])
    merged.close()


def test_merge_errors(oracle, g):
    cents, ia, ib, pq, a, b, Q = _sources(oracle, g, "vec4x2")
    _, d, m, k = LAYOUTS["vec4x2"]
    for take, position in (([0, NA, 3], 1), ([5, -1, -1 - NB], 2), ([2 ** 40, 0], 0)):
        with pytest.raises(ValueError, match=rf"take\[{position}\]"):
            a.merged(b, take)
    with pytest.raises(ValueError, match=r"take\[1\]"):
        a.merged(None, [4, -1])                                  # a negative entry and no second index
    with pytest.raises(ValueError):
        a.merged(b, [0.5, 1.0])
    other_m = _sources(oracle, g, "vec16")[5]                    # m = 16 against m = 8
    with pytest.raises(ValueError, match="shape"):
        a.merged(other_m, [0, -1])
    other_k = _sources(oracle, g, "packed4")[5]                  # k = 16 against k = 256
    with pytest.raises(ValueError, match="shape"):
        a.merged(other_k, [0, -1])
    flipped = cents.copy()
    flipped.view(np.uint32)[k * d // 2] ^= 1                     # the same shapes, one centroid bit
    pqf = g.ProductQuantizer.from_flat(k, d, m, flipped)
    bf = _native(g, pqf, ib)
    with pytest.raises(ValueError, match="codebooks"):
        a.merged(bf, [0, -1])
    bf.close()
    assert a.merged(b, [0, -1]).length == 2                      # and nothing was left broken


def test_merge_reads_views_and_contexts_and_outlives_its_sources(oracle, g):
    n, d, m, k = LAYOUTS["vec16"]
    cents, ia, pq, ea = _make(oracle, g, n, d, m, k, seed=77)
    ib = np.random.default_rng(6).integers(0, k, (m, NB)).astype(np.int32)
    a, b = g.PQIndex(pq, ea, row_base=5000), _native(g, pq, ib)
    rows = np.arange(1, n, 2)
    view, ctx = a.select(rows=rows), b.context()
    take = np.array([499, -1, 0, -130, 63, 64, -64])            # positions of the view, rows of the context
    merged = view.merged(ctx, take)
    want = np.ascontiguousarray(np.concatenate([ia[:, rows], ib], axis=1)[:, np.where(take >= 0, take, len(rows) - 1 - take)])
    assert np.array_equal(merged.indices(), want)
    Q = np.random.default_rng(9).standard_normal((8, d)).astype(np.float32)
    first = merged.batch_query_raw(10, Q)
    assert first[0].max() < len(take)                            # row_base 0: no map, no base
    view.close(), ctx.close(), a.close(), b.close()
    _same_answers(merged.batch_query_raw(10, Q), first)
    _check(oracle, merged.batch_query(5, Q), *oracle.pq_batch_query(want, d, k, cents, Q, 5))
    again = merged.context()
    assert again.length == len(take) and np.array_equal(again.indices(), want)
    merged.close()                                               # the context keeps the buffers alive
    _same_answers(again.batch_query_raw(10, Q), first)
    again.close()


# ---------------------------------------------------------------- 3. get_codes
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_indices_reads_the_plain_code_buffer(oracle, g, layout):
    from gulon_amd import native as N
    cents, ia, ib, pq, a, b, Q = _sources(oracle, g, layout)
    assert np.array_equal(a.indices(), ia)
    assert np.array_equal(a.indices(70, 330), ia[:, 70:330])
    assert a.indices(64, 64).shape == (ia.shape[0], 0)
    rows = np.sort(np.random.default_rng(3).choice(NA, 333, replace=False))
    view = a.select(rows=rows)
    assert np.array_equal(view.indices(), ia[:, rows])           # a view in its own positions
    assert np.array_equal(view.indices(70, 330), ia[:, rows[70:330]])
    view.close()
    for frm, until in ((-1, 5), (5, 4), (0, NA + 1)):
        with pytest.raises(ValueError, match="outside"):
            a.indices(frm, until)
    assert N.lib().gulon_index_get_codes(None, 0, 0, np.zeros(1, np.uint16)) == N.ERR_INVALID_ARGUMENT


def test_indices_with_the_filter_copy_present(oracle, g):
    """An index large enough to carry the filter's reordered copy still answers from the plain one."""
    n, d, m, k = 40000, 32, 16, 256
    cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=40)
    ix = g.PQIndex(pq, enc)
    assert np.array_equal(ix.indices(), idx)
    ix.close()
