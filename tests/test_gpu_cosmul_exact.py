"""3CosMul on the exact index (csrc/cosmul.hip, gulon_exact_index_query_cosmul): rows and score BITS
against numpy -- the distances of every term vector (the handle's own compose_rows of the one-term expression) restated
in knn_kernel's order of operations, expressions.cosmul_reference, np.lexsort((rows, -score)) with the term rows removed.

Shapes: one partial 64-row tile, odd dimensions below and above the 32-dim staging step, more than one row chunk, 300
dimensions.  Term lists of every slot count the scan is compiled for (1, 2, 4 and 8 slots per question), alone and mixed."""
import numpy as np
import pytest

from cosmul_ref import exact_distances, mixed_batch, per_expression, reference_lists, same, unit_rows

pytestmark = pytest.mark.gpu

SHAPES = ((63, 7), (257, 33), (1500, 16), (5000, 300))


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


_WORLDS = {}


def world(g, n, d):
    """Unit rows, their device copy and a cosine ExactIndex over all of them: made once per shape."""
    if (n, d) not in _WORLDS:
        X = unit_rows(7 * n + d, n, d)
        dm = g.DeviceMatrix.from_host(X)
        _WORLDS[(n, d)] = (X, dm, g.ExactIndex(dm, "cosine"))
    return _WORLDS[(n, d)]


def reference(ix, X, exprs, k):
    """The contract on the host for the handle `ix` over rows [ix.frm, ix.until) of X."""
    Q = ix.compose_rows([[(r, 1.0)] for e in exprs for r, _ in e])
    D = exact_distances(X[ix.frm:ix.until], Q)
    return reference_lists(per_expression(D, exprs), exprs, np.arange(ix.frm, ix.until), k)


@pytest.mark.parametrize("n,d", SHAPES)
def test_mixed_batch_matches_numpy(g, n, d):
    X, _, ix = world(g, n, d)
    exprs = mixed_batch(n + d, n, 17)
    same(ix.batch_query_cosmul_raw(10, exprs), reference(ix, X, exprs, 10))


@pytest.mark.parametrize("pattern", ["+", "+-", "+-+", "-+++-", "8"])
def test_every_slot_count(g, pattern):
    """A batch of one pattern: 1, 2, 4 (three terms), 8 (five terms) and 8 slots per question."""
    X, _, ix = world(g, 1500, 16)
    exprs = mixed_batch(len(pattern), 1500, 5, patterns=(pattern,))
    same(ix.batch_query_cosmul_raw(10, exprs), reference(ix, X, exprs, 10))


@pytest.mark.parametrize("b,k", [(1, 1), (1, 60), (5, 1), (5, 60), (17, 60)])
def test_batch_sizes_and_depths(g, b, k):
    """k = 60 leaves room for three terms (k + E <= 63); on 63 rows it also runs out of rows."""
    for n, d in ((63, 7), (1500, 16)):
        X, _, ix = world(g, n, d)
        exprs = mixed_batch(b + k, n, b, patterns=("+", "+-", "+-+"))
        same(ix.batch_query_cosmul_raw(k, exprs), reference(ix, X, exprs, k))


def test_more_questions_than_one_pass_holds(g):
    """4 096 questions are one pass of the scan: 4 100 take two, the second reading its terms from where the first
    ended."""
    X, _, ix = world(g, 63, 7)
    exprs = mixed_batch(21, 63, 4100, patterns=("+", "+-"))
    same(ix.batch_query_cosmul_raw(3, exprs), reference(ix, X, exprs, 3))


def test_l2_handle_takes_the_rows_as_they_are(g):
    """normalize = 0, on rows that are not unit vectors: distances above 4 clamp to a score of 0, and the rows with
    equal scores come out in row order."""
    X = np.random.default_rng(5).standard_normal((257, 33)).astype(np.float32) * np.float32(0.35)
    dm = g.DeviceMatrix.from_host(X)
    ix = g.ExactIndex(dm)
    try:
        exprs = mixed_batch(9, 257, 17)
        same(ix.batch_query_cosmul_raw(10, exprs), reference(ix, X, exprs, 10))
        far = [[(0, 1.0), (1, -1.0)]]                        # against 3 * row 0 every distance is above 4
        X2 = X.copy()
        X2[0] *= np.float32(3)
        dm2 = g.DeviceMatrix.from_host(X2)
        ix2 = g.ExactIndex(dm2)
        try:
            got = ix2.batch_query_cosmul_raw(10, far)
            same(got, reference(ix2, X2, far, 10))
            assert got[0][0].tolist() == list(range(2, 12)) and (got[1] == 0).all()
        finally:
            ix2.close()
            dm2.close()
    finally:
        ix.close()
        dm.close()


def test_range_handle_with_operands_outside(g):
    X, dm, _ = world(g, 1500, 16)
    ix = g.ExactIndex(dm, "cosine", 100, 1301)
    try:
        exprs = mixed_batch(3, 1500, 17)                     # operands anywhere in the matrix
        exprs += [[(5, 1.0), (1400, -1.0), (99, 1.0)], [(1301, 1.0), (100, -1.0), (1300, 1.0)]]
        got, want = ix.batch_query_cosmul_raw(10, exprs), reference(ix, X, exprs, 10)
        same(got, want)
        assert got[0].min() >= 100 and got[0].max() < 1301
    finally:
        ix.close()


def test_equal_scores_come_out_in_row_order(g):
    base = unit_rows(11, 128, 16)
    X = np.tile(base, (4, 1))                                # rows r, r + 128, r + 256, r + 384 are equal
    dm = g.DeviceMatrix.from_host(X)
    ix = g.ExactIndex(dm, "cosine")
    try:
        exprs = mixed_batch(13, 512, 5, patterns=("+-+", "+"))
        got, want = ix.batch_query_cosmul_raw(6, exprs), reference(ix, X, exprs, 6)
        same(got, want)
        assert any((np.diff(s) == 0).any() for s in got[1])
    finally:
        ix.close()
        dm.close()


def test_fewer_rows_than_k(g):
    X = unit_rows(17, 10, 7)
    dm = g.DeviceMatrix.from_host(X)
    ix = g.ExactIndex(dm, "cosine")
    try:
        exprs = [[(1, 1.0), (2, -1.0), (3, 1.0)], [(4, 1.0)], [(0, 1.0), (9, -1.0), (0, 1.0)]]
        oi, os_, oc = ix.batch_query_cosmul_raw(20, exprs)
        same((oi, os_, oc), reference(ix, X, exprs, 20))
        assert oc.tolist() == [7, 9, 8]
        for q, c in enumerate(oc):
            assert (oi[q, c:] == -1).all() and np.isneginf(os_[q, c:]).all()
        results = ix.batch_query_cosmul(20, exprs)
        assert [len(r.rows) for r in results] == [7, 9, 8] and all(r.flags == 0 for r in results)
        assert all((np.diff(r.distances) <= 0).all() for r in results)      # scores, descending
    finally:
        ix.close()
        dm.close()


def test_limits_and_bad_arguments(g):
    _, _, ix = world(g, 1500, 16)
    with pytest.raises(NotImplementedError):
        ix.batch_query_cosmul_raw(5, [[(r, 1.0) for r in range(9)]])           # 9 terms
    with pytest.raises(NotImplementedError):
        ix.batch_query_cosmul_raw(61, [[(1, 1.0), (2, -1.0), (3, 1.0)]])         # k + E = 64
    assert ix.batch_query_cosmul_raw(60, [[(1, 1.0), (2, -1.0), (3, 1.0)]])[2].tolist() == [60]
    for bad in ([[(1, -1.0), (2, -1.0)]], [[(1, 1.0), (2, 0.5)]], [[(1, 1.0), (1500, -1.0)]], [[(-1, 1.0)]]):
        with pytest.raises(ValueError):
            ix.batch_query_cosmul_raw(5, bad)
    assert ix.batch_query_cosmul_raw(5, [])[0].shape == (0, 5)


def test_dev_form_bad_expression(g):
    """Device pointers: the good expressions answer as the host form does; one without a positive term and one with a
    row outside the matrix come back empty and set *d_err."""
    from gulon_amd.expressions import to_csr
    from gulon_amd.refine import _DeviceArray
    N = g.native
    X, _, ix = world(g, 1500, 16)
    k = 10
    exprs = mixed_batch(23, 1500, 6)
    exprs[2] = [(4, -1.0), (5, -1.0)]
    exprs[4] = [(7, 1.0), (1500, -1.0), (9, 1.0)]
    good = [q for q in range(6) if q not in (2, 4)]
    off, rows, w = to_csr(exprs)
    dev = {name: _DeviceArray() for name in ("off", "rows", "w", "oi", "os", "oc", "err")}
    try:
        dev["off"].upload(off), dev["rows"].upload(rows), dev["w"].upload(w)
        dev["err"].upload(np.zeros(1, np.int32))
        for name, nbytes in (("oi", 6 * k * 4), ("os", 6 * k * 4), ("oc", 6 * 4)):
            dev[name].ensure(nbytes)
        N.check(N.lib().gulon_exact_index_query_cosmul_dev(ix._h, dev["off"].ptr, dev["rows"].ptr, dev["w"].ptr, 6, k, 1,
                                                           dev["oi"].ptr, dev["os"].ptr, dev["oc"].ptr, dev["err"].ptr,
                                                           None))
        oi = dev["oi"].download(np.zeros((6, k), np.int32))
        os_ = dev["os"].download(np.zeros((6, k), np.float32))
        oc = dev["oc"].download(np.zeros(6, np.int32))
        err = dev["err"].download(np.zeros(1, np.int32))
    finally:
        for a in dev.values():
            a.free()
    assert err[0] == 1 and oc[[2, 4]].tolist() == [0, 0]
    assert (oi[[2, 4]] == -1).all() and np.isneginf(os_[[2, 4]]).all()
    same((oi[good], os_[good], oc[good]), reference(ix, X, [exprs[q] for q in good], k))


def test_word_level(g):
    """ExactWordIndex: words in, None where a word is absent, ValueError on an l2 index."""
    X, dm, ix = world(g, 257, 33)
    words = [f"w{i:03d}" for i in range(257)]
    wi = g.ExactWordIndex(words, ix)
    got = wi.batch_query_cosmul(5, ["w001 - w002 + w003", "w001 - nope + w003", [("w010", 1.0)]])
    want = reference(ix, X, [[(1, 1.0), (2, -1.0), (3, 1.0)], [(10, 1.0)]], 5)
    assert got[1] is None
    for r, q in ((got[0], 0), (got[2], 1)):
        assert r.rows.tolist() == want[0][q].tolist() and r.words == [words[i] for i in want[0][q]]
    assert wi.query_cosmul(5, "w001 - w002 + w003").words == got[0].words
    l2 = g.ExactIndex(dm)
    try:
        with pytest.raises(ValueError):
            g.ExactWordIndex(words, l2).batch_query_cosmul(5, ["w001"])
    finally:
        l2.close()
