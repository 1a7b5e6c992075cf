"""3CosMul on the flat index (csrc/cosmul.hip, gulon_index_query_cosmul): rows and score BITS against
numpy.  The per-term distances are restated from the oracle's Index.prepareQuery tables of every term vector (the
handle's own compose_rows of the one-term expression), summed over the quantizers in the order of scan.hip's exact scan;
once they are also compared with the handle's own batch_query at k = n.  Then expressions.cosmul_reference and
np.lexsort((rows, -score)) with the term rows removed.

Quantizer counts: one 4-byte code word, one 16-byte word, two words with padding (m = 25); code books of 16 and 256."""
import numpy as np
import pytest

from conftest import bits
from cosmul_ref import adc_distances, mixed_batch, per_expression, reference_lists, same, unit_rows

pytestmark = pytest.mark.gpu

N_ROWS, ITERS = 2000, 2
UP_TO_FIVE = ("+", "+-", "+-+", "-+++-")     # m = 25 is m_pad = 28: 28 KiB of tables per term, five terms in 144 KiB


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


_WORLDS = {}


def world(g, d, m, k, metric="cosine"):
    """A SortedIndex over N_ROWS unit rows, its codes [n][m] and flat centroids: trained once per shape."""
    key = (d, m, k, metric)
    if key not in _WORLDS:
        X = unit_rows(d + m + k, N_ROWS, d)
        dm = g.DeviceMatrix.from_host(X)
        pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(k, m, ITERS))
        index = g.Index.sorted(dm, pq, metric)
        codes = np.ascontiguousarray(index.vector_index.data.indices().T)
        _WORLDS[key] = (index, pq, codes, pq.flat_centroids())
    return _WORLDS[key]


def term_distances(oracle, index, codes, cents, k, exprs):
    d, m = index.dimension, codes.shape[1]
    Q = index.compose_rows([[(r, 1.0)] for e in exprs for r, _ in e])
    return Q, adc_distances(oracle.prepare_query(cents, d, m, k, Q), codes)


def reference(oracle, index, codes, cents, k, exprs, knn, frm=0, until=N_ROWS):
    _, D = term_distances(oracle, index, codes, cents, k, exprs)
    return reference_lists(per_expression(D[:, frm:until], exprs), exprs, np.arange(frm, until), knn)


@pytest.mark.parametrize("m", [4, 16, 25])
@pytest.mark.parametrize("k", [16, 256])
def test_matches_numpy(g, oracle, m, k):
    index, _, codes, cents = world(g, 32, m, k)
    exprs = mixed_batch(m + k, N_ROWS, 17, **({"patterns": UP_TO_FIVE} if m == 25 else {}))
    same(index.batch_query_cosmul_raw(10, exprs), reference(oracle, index, codes, cents, k, exprs, 10))
    if m == 25:
        with pytest.raises(NotImplementedError, match="m = 25, E = 6.*LDS"):
            index.batch_query_cosmul_raw(10, [[(r, 1.0) for r in range(6)]])
    exprs = mixed_batch(m, N_ROWS, 5, patterns=("+", "+-", "+-+"))
    for knn in (1, 60):
        same(index.batch_query_cosmul_raw(knn, exprs), reference(oracle, index, codes, cents, k, exprs, knn))


def test_restated_distances_are_the_handles_own(g, oracle):
    """The distances the reference is built from against the parent's batch_query at k = n, bit for bit."""
    index, _, codes, cents = world(g, 32, 25, 256)
    exprs = mixed_batch(1, N_ROWS, 3, patterns=("+-+",))
    Q, D = term_distances(oracle, index, codes, cents, 256, exprs)
    oi, od, oc, _ = index.vector_index.batch_query_raw(N_ROWS, Q)
    assert (oc == N_ROWS).all()
    for t in range(len(Q)):
        by_row = np.zeros(N_ROWS, np.float32)
        by_row[oi[t]] = od[t]
        assert np.array_equal(bits(by_row), bits(D[t]))


def test_128_dimensions(g, oracle):
    index, _, codes, cents = world(g, 128, 32, 256)
    exprs = mixed_batch(2, N_ROWS, 5, patterns=("+", "+-+", "+-"))
    same(index.batch_query_cosmul_raw(10, exprs), reference(oracle, index, codes, cents, 256, exprs, 10))


def test_l2_index_takes_the_rows_as_they_are(g, oracle):
    index, _, codes, cents = world(g, 32, 16, 256, "l2")
    exprs = mixed_batch(4, N_ROWS, 5)
    same(index.batch_query_cosmul_raw(10, exprs), reference(oracle, index, codes, cents, 256, exprs, 10))


def test_row_range(g, oracle):
    index, _, codes, cents = world(g, 32, 16, 256)
    exprs = mixed_batch(5, N_ROWS, 9)                        # operands inside and outside the range
    got = index.vector_index.batch_query_cosmul_raw(10, exprs, 70, 1931, normalize=True)
    same(got, reference(oracle, index, codes, cents, 256, exprs, 10, 70, 1931))
    assert got[0].min() >= 70 and got[0].max() < 1931


def test_lds_limit(g, oracle):
    """m = 64: one term's tables are 64 KiB, so two terms fit in 144 KiB and three do not."""
    index, _, codes, cents = world(g, 128, 64, 256)
    with pytest.raises(NotImplementedError, match="LDS"):
        index.batch_query_cosmul_raw(5, [[(1, 1.0), (2, -1.0), (3, 1.0)]])
    exprs = mixed_batch(6, N_ROWS, 4, patterns=("+-", "+"))
    same(index.batch_query_cosmul_raw(5, exprs), reference(oracle, index, codes, cents, 256, exprs, 5))


def test_more_questions_than_one_pass_holds(g, oracle):
    """At m = 64 the tables of 512 questions (eight slots each) fill the 256 MiB a pass is given: 600 questions take
    two passes, the second reading its terms from where the first ended."""
    index, _, codes, cents = world(g, 128, 64, 256)
    exprs = mixed_batch(12, N_ROWS, 600, patterns=("+", "+-"))
    same(index.batch_query_cosmul_raw(3, exprs), reference(oracle, index, codes, cents, 256, exprs, 3))


def test_dev_form_bad_expression(g, oracle):
    """Device pointers: a good expression answers as the host form does; one without a positive term, one with a row
    outside the index and one beyond the LDS limit (six terms at m = 25) come back empty and set the row-error word."""
    import ctypes as C
    from gulon_amd.expressions import to_csr
    from gulon_amd.refine import _DeviceArray
    N = g.native
    index, _, codes, cents = world(g, 32, 25, 256)
    vi, k = index.vector_index, 7
    exprs = [[(3, 1.0), (4, -1.0), (5, 1.0)], [(6, -1.0)], [(7, 1.0), (N_ROWS, -1.0)], [(r, 1.0) for r in range(6)],
             [(9, 1.0), (8, -1.0)]]
    off, rows, w = to_csr(exprs)
    dev = {name: _DeviceArray() for name in ("off", "rows", "w", "oi", "os", "oc")}
    err = C.c_int32(-1)
    try:
        N.check(N.lib().gulon_index_row_error(vi._h, C.byref(err)))          # cleared
        dev["off"].upload(off), dev["rows"].upload(rows), dev["w"].upload(w)
        for name, nbytes in (("oi", 5 * k * 4), ("os", 5 * k * 4), ("oc", 5 * 4)):
            dev[name].ensure(nbytes)
        N.check(N.lib().gulon_index_query_cosmul_dev(vi._h, dev["off"].ptr, dev["rows"].ptr, dev["w"].ptr, 5, k, 1, 0,
                                                     N_ROWS, dev["oi"].ptr, dev["os"].ptr, dev["oc"].ptr, None))
        N.check(N.lib().gulon_index_row_error(vi._h, C.byref(err)))          # synchronises
        oi = dev["oi"].download(np.zeros((5, k), np.int32))
        os_ = dev["os"].download(np.zeros((5, k), np.float32))
        oc = dev["oc"].download(np.zeros(5, np.int32))
    finally:
        for a in dev.values():
            a.free()
    assert err.value == 1 and oc.tolist() == [k, 0, 0, 0, k]
    assert (oi[1:4] == -1).all() and np.isneginf(os_[1:4]).all()
    good = [exprs[0], exprs[4]]
    same((oi[[0, 4]], os_[[0, 4]], oc[[0, 4]]), reference(oracle, index, codes, cents, 256, good, k))
    N.check(N.lib().gulon_index_row_error(vi._h, C.byref(err)))
    assert err.value == 0


def test_wide_index_and_view_are_refused(g):
    index, _, _, _ = world(g, 32, 4, 1024, "l2")
    with pytest.raises(NotImplementedError):
        index.batch_query_cosmul_raw(5, [[(1, 1.0)]])
    flat, _, _, _ = world(g, 32, 16, 256)
    view = flat.select(rows=np.arange(0, N_ROWS, 2))
    try:
        with pytest.raises(NotImplementedError):
            view.batch_query_cosmul_raw(5, [[(1, 1.0)]])
    finally:
        view.vector_index.close()


def test_limits_and_bad_arguments(g):
    index, _, _, _ = world(g, 32, 16, 256)
    with pytest.raises(NotImplementedError):
        index.batch_query_cosmul_raw(5, [[(r, 1.0) for r in range(9)]])
    with pytest.raises(NotImplementedError):
        index.batch_query_cosmul_raw(61, [[(1, 1.0), (2, -1.0), (3, 1.0)]])
    for bad in ([[(1, -1.0)]], [[(1, 1.0), (2, 2.0)]], [[(1, 1.0), (N_ROWS, -1.0)]]):
        with pytest.raises(ValueError):
            index.batch_query_cosmul_raw(5, bad)


def test_handle_history(g):
    """After cosmul calls the handle's batch_query answers as before them, and as a fresh handle over the same codes."""
    index, pq, _, _ = world(g, 32, 25, 256)
    vi = index.vector_index
    Q = unit_rows(3, 9, 32)
    before = vi.batch_query_raw(10, Q)
    index.batch_query_cosmul_raw(10, mixed_batch(8, N_ROWS, 17, patterns=UP_TO_FIVE))
    index.batch_query_cosmul_raw(3, mixed_batch(9, N_ROWS, 2, patterns=("+",)))
    after = vi.batch_query_raw(10, Q)
    fresh = g.PQIndex(pq, vi.data)
    try:
        other = fresh.batch_query_raw(10, Q)
    finally:
        fresh.close()
    for got in (after, other):
        assert np.array_equal(got[0], before[0]) and np.array_equal(bits(got[1]), bits(before[1]))
        assert np.array_equal(got[2], before[2]) and np.array_equal(got[3], before[3])
