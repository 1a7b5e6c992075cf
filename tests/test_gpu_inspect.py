"""Index diagnostics on the device (inspect.hip): the code histogram against np.bincount of the codes, the row errors
against a numpy.float32 restatement of MathUtils.distanceSq(original, decoded) -- bit for bit per row, within the
a-priori bound of binary64 summation per quantizer -- for flat indexes, views and grouped indexes, and WordIndex.inspect
end to end."""
import math

import numpy as np
import pytest

import handle_history as hh
from conftest import bits
from test_gpu_lookup import _direct_grouped, _word_indexes, ref_partition
from test_gpu_query import _make

pytestmark = pytest.mark.gpu

LAYOUTS = {"vec16": (32, 16, 256),         # one 16-byte code word per row
           "vec4x2": (32, 8, 256),         # two 4-byte words per row
           "m25": (50, 25, 256),           # seven 4-byte words, three padding quantizers
           "packed4": (32, 8, 16),         # 4-bit codes in the file, one byte per quantizer on the device
           "wide1024": (32, 16, 1024),     # 16-bit codes; the counters fill 64 KiB of LDS exactly
           "wide65536": (16, 4, 65536)}    # the counters do not fit in LDS: global adds
ROW_COUNTS = (1, 63, 64, 65, 1000)
RANGES = ("all", (0, 0), (63, 64), (60, 70), "inner", (250, 262))


def _ranges(n):
    """the ranges of RANGES that lie inside [0, n]"""
    out = []
    for r in RANGES:
        frm, until = (0, n) if r == "all" else (1, n - 1) if r == "inner" else r
        if 0 <= frm <= until <= n and (frm, until) not in out:
            out.append((frm, until))
    return out


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def _bincount(idx, k, frm, until):
    return np.stack([np.bincount(row[frm:until], minlength=k) for row in idx]).astype(np.int64)


# ---------------------------------------------------------------- 1. histogram
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_histogram_equals_bincount(oracle, g, layout):
    d, m, k = LAYOUTS[layout]
    for n in ROW_COUNTS:
        cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=n + k + m)
        ix = g.PQIndex(pq, enc)
        assert np.array_equal(enc.indices(), idx)
        for frm, until in _ranges(n):
            H = ix.code_histogram(frm, until)
            assert H.dtype == np.int64 and H.shape == (m, k)
            assert (H.sum(axis=1) == until - frm).all(), (n, frm, until)      # no padding lane, no padding quantizer
            assert np.array_equal(H, _bincount(idx, k, frm, until)), (n, frm, until)
        assert np.array_equal(ix.code_histogram(), _bincount(idx, k, 0, n))
        assert np.array_equal(g.SortedIndex(ix).code_histogram(), _bincount(idx, k, 0, n))
        ix.close()


# ---------------------------------------------------------------- 2. views
@pytest.mark.parametrize("selection", ["every_third", "s65"])
def test_view_histogram_is_that_of_the_selected_rows(oracle, g, selection):
    n, (d, m, k) = 1000, LAYOUTS["vec16"]
    cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=3)
    rows = {"every_third": np.arange(0, n, 3),
            "s65": np.sort(np.random.default_rng(65).choice(n, 65, replace=False))}[selection]
    parent = g.PQIndex(pq, enc)
    view = parent.select(rows=rows)
    sub = np.ascontiguousarray(idx[:, rows])
    s = len(rows)
    for frm, until in [(0, s), (0, 0), (1, s - 1), (60, 65)]:
        assert np.array_equal(view.code_histogram(frm, until), _bincount(sub, k, frm, until)), (frm, until)
    # and its row errors are those of the selected rows, over the view's own positions
    V = np.random.default_rng(4).standard_normal((n, d)).astype(np.float32)
    dm = g.DeviceMatrix.from_host(V)
    err, qerr = view.row_errors(dm, row_map=rows)
    perr, _ = parent.row_errors(dm)
    assert np.array_equal(bits(err), bits(perr[rows]))
    view.close()
    parent.close()
    dm.close()


# ---------------------------------------------------------------- 3. row errors, flat
def _restate(g, V, Y, m):
    """MathUtils.distanceSq(V[r], Y[r]) for every r as the issue states it: binary32, t = x_e - y_e; sum += t * t,
    unfused, e ascending -- every numpy operation below rounds once to float32.  -> (row_error, row_norm_sq, p[n][m])"""
    n, d = V.shape
    fr, un = g.subvector_bounds(d, m)
    err, nrm, p = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, m), np.float32)
    for j in range(m):
        for e in range(int(fr[j]), int(un[j])):
            t = V[:, e] - Y[:, e]
            tt = t * t
            err = err + tt
            p[:, j] = p[:, j] + tt
            nrm = nrm + V[:, e] * V[:, e]
    assert err.dtype == np.float32 and p.dtype == np.float32
    return err, nrm, p


def _check_errors(got, want, frm, until):
    """per row bit for bit; per quantizer |got - S| <= n * 2^-52 * S with S = fsum of the restated p[:, j] and n the rows
    summed: twice the a-priori bound (n - 1) * 2^-53 * S of binary64 summation of non-negative terms in any order"""
    err, qerr, nrm = got
    werr, wnrm, wp = want
    rows = until - frm
    assert err.dtype == np.float32 and nrm.dtype == np.float32 and qerr.dtype == np.float64
    assert err.shape == (rows,) and nrm.shape == (rows,) and qerr.shape == (wp.shape[1],)
    assert np.array_equal(bits(err), bits(werr[frm:until]))
    assert np.array_equal(bits(nrm), bits(wnrm[frm:until]))
    for j in range(wp.shape[1]):
        S = math.fsum(wp[frm:until, j].astype(np.float64).tolist())
        assert abs(qerr[j] - S) <= rows * 2.0 ** -52 * S, (j, qerr[j], S)


FLAT_SHAPES = {"n1000_d32_m8": (1000, 32, 8, 256),
               "n200_d300_m32": (200, 300, 32, 256),      # ragged sub-vectors: 12 x 10 + 20 x 9 coordinates
               "n65_wide": (65, 32, 16, 1024),
               "n130_d50_m25": (130, 50, 25, 256)}        # d % 4 != 0: the 4-byte loads of the tile


@pytest.mark.parametrize("shape", list(FLAT_SHAPES))
def test_row_errors_flat(oracle, g, shape):
    n, d, m, k = FLAT_SHAPES[shape]
    cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=n + d)
    ix = g.PQIndex(pq, enc)
    Y = ix.decode_rows(np.arange(n))
    rng = np.random.default_rng(d)
    V = (rng.standard_normal((n + 37, d)) * 2).astype(np.float32)
    shuffled = rng.permutation(n + 37)[:n].astype(np.int32)
    dm = g.DeviceMatrix.from_host(V)
    for row_map in (None, shuffled):
        want = _restate(g, V[:n] if row_map is None else V[row_map], Y, m)
        for frm, until in _ranges(n):
            _check_errors(ix.row_errors(dm, row_map, frm, until, norms=True), want, frm, until)
        err, qerr = ix.row_errors(dm, row_map)                           # without the norms: the same numbers
        assert np.array_equal(bits(err), bits(want[0]))
        assert g.reference_quality(err) == np.cumsum(want[0], dtype=np.float32)[-1]
    ix.close()
    dm.close()


# ---------------------------------------------------------------- 4. row errors, grouped
@pytest.mark.parametrize("k", [256, 1024])
def test_row_errors_grouped_use_the_rows_own_group(oracle, g, k):
    n, d, m = 300, 16, 4
    offsets = [0, 5, 5, 5, 9, 40, 40, 100, 150, 150, 150, 220]        # a leading empty group, interior empty groups
    gx, cents, idx, gc = _direct_grouped(g, n, d, m, k, offsets, seed=k + 1)
    rows = np.arange(n)
    own = np.searchsorted(np.asarray(offsets), rows, side="right")    # the group whose range holds the row
    ref = np.array([ref_partition(offsets, int(r)) for r in rows])
    assert (own != ref).any()                                         # else the test would not tell the two rules apart
    Y = (gc[own] + oracle.pq_decode(idx, d, k, cents)).astype(np.float32)
    assert not np.array_equal(bits(Y), bits(gx.lookup_rows(rows)))
    rng = np.random.default_rng(k)
    V = (rng.standard_normal((n + 11, d)) * 3).astype(np.float32)
    shuffled = rng.permutation(n + 11)[:n].astype(np.int32)
    dm = g.DeviceMatrix.from_host(V)
    for row_map in (None, shuffled):
        want = _restate(g, V[:n] if row_map is None else V[row_map], Y, m)
        for frm, until in _ranges(n):
            _check_errors(gx.row_errors(dm, row_map, frm, until, norms=True), want, frm, until)
    assert np.array_equal(gx.code_histogram(), _bincount(idx, k, 0, n))
    assert np.array_equal(gx.code_histogram(3, 77), _bincount(idx, k, 3, 77))
    gx.close()
    dm.close()


# ---------------------------------------------------------------- 5. argument errors
def test_argument_errors(oracle, g):
    n, d, m, k = 200, 32, 8, 256
    cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=9)
    ix = g.PQIndex(pq, enc)
    V = np.random.default_rng(1).standard_normal((n, d)).astype(np.float32)
    dm = g.DeviceMatrix.from_host(V)
    for bad in (n, -1, 2 ** 31 - 1):
        row_map = np.arange(n, dtype=np.int32)
        row_map[131] = bad
        with pytest.raises(ValueError, match="row map entry 131"):
            ix.row_errors(dm, row_map)
        ix.row_errors(dm, row_map, 0, 131)                            # the entry is outside the range: not looked at
    with pytest.raises(ValueError, match="dimension"):
        ix.row_errors(g.DeviceMatrix.from_host(V[:, :d - 4]))
    with pytest.raises(ValueError, match="row map of 199 entries"):
        ix.row_errors(dm, np.arange(n - 1, dtype=np.int32))
    with pytest.raises(ValueError, match="no row map"):
        ix.row_errors(g.DeviceMatrix.from_host(V[:n - 1]))                # the identity needs n vectors
    for frm, until in ((10, 5), (0, n + 1), (-1, 5)):
        with pytest.raises(ValueError, match="from <= until <= length"):
            ix.row_errors(dm, None, frm, until)
        with pytest.raises(ValueError, match="from <= until <= length"):
            ix.code_histogram(frm, until)
    # the handle is as usable as before
    want = _restate(g, V, ix.decode_rows(np.arange(n)), m)
    _check_errors(ix.row_errors(dm, norms=True), want, 0, n)
    ix.close()
    # an index without rows: empty outputs, an all-zero histogram
    cents, idx, pq, enc = _make(oracle, g, 0, d, m, k, seed=9)
    empty = g.PQIndex(pq, enc)
    assert not empty.code_histogram().any() and empty.code_histogram().shape == (m, k)
    err, qerr, nrm = empty.row_errors(dm, norms=True)
    assert err.shape == (0,) and nrm.shape == (0,) and qerr.tolist() == [0.0] * m
    err, qerr = empty.row_errors(dm, np.zeros(0, np.int32))
    assert err.shape == (0,)
    empty.close()
    dm.close()


def test_device_forms_equal_the_host_forms(oracle, g):
    """gulon_*_row_errors_dev: the map and the per-row outputs in device memory, quantizer_error on the host; an entry
    outside the vectors is found on the device and reported when the call returns."""
    import ctypes as C
    from gulon_amd import native as N
    L = N.lib()
    n, d, m, k = 300, 16, 4, 256
    gx, cents, idx, gc = _direct_grouped(g, n, d, m, k, [0, 100, 100, 230], seed=12)
    cents2, idx2, pq, enc = _make(oracle, g, n, d, m, k, seed=13)
    ix = g.PQIndex(pq, enc)
    rng = np.random.default_rng(14)
    V = rng.standard_normal((n + 5, d)).astype(np.float32)
    dm = g.DeviceMatrix.from_host(V)
    row_map = rng.permutation(n + 5)[:n].astype(np.int32)
    frm, until = 60, 262
    d_map, d_err, d_nrm = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for p in (d_map, d_err, d_nrm):
        N.check(L.gulon_dev_malloc(C.byref(p), 4 * n))
    try:
        for index, fn in ((ix, L.gulon_index_row_errors_dev), (gx, L.gulon_grouped_index_row_errors_dev)):
            N.check(L.gulon_memcpy_h2d(d_map, row_map.ctypes.data, row_map.nbytes))
            want = index.row_errors(dm, row_map, frm, until, norms=True)
            err, nrm = np.zeros(until - frm, np.float32), np.zeros(until - frm, np.float32)
            qerr = np.zeros(m, np.float64)
            N.check(fn(index._h, dm._h, d_map, n, frm, until, d_err, d_nrm, qerr, None))
            N.check(L.gulon_memcpy_d2h(err.ctypes.data, d_err, err.nbytes))
            N.check(L.gulon_memcpy_d2h(nrm.ctypes.data, d_nrm, nrm.nbytes))
            assert np.array_equal(bits(err), bits(want[0])) and np.array_equal(bits(nrm), bits(want[2]))
            assert np.array_equal(qerr, want[1])                      # the block sums are added in a fixed order
            N.check(fn(index._h, dm._h, d_map, n, frm, until, d_err, None, qerr, None))      # row_norm_sq is optional
            assert np.array_equal(qerr, want[1])
            bad = row_map.copy()
            bad[frm + 3] = n + 5
            N.check(L.gulon_memcpy_h2d(d_map, bad.ctypes.data, bad.nbytes))
            with pytest.raises(ValueError, match="outside the 305 vectors"):
                N.check(fn(index._h, dm._h, d_map, n, frm, until, d_err, d_nrm, qerr, None))
            with pytest.raises(ValueError, match="row map of 299 entries"):
                N.check(fn(index._h, dm._h, d_map, n - 1, frm, until, d_err, d_nrm, qerr, None))
    finally:
        for p in (d_map, d_err, d_nrm):
            L.gulon_dev_free(p)
        ix.close()
        gx.close()
        dm.close()


# ---------------------------------------------------------------- 6. WordIndex.inspect
def test_word_index_inspect(oracle, g):
    from gulon_amd.inspect import entropy_bits
    from gulon_amd.word_vectors import DeviceWordVectors, KeyIndexSorted
    seen = set()
    for kind, wi, words, _, _ in _word_indexes(g, oracle):
        index = wi.index
        grouped = kind == "grouped"
        seen.add((kind, index.metric))
        n, d = len(words), index.dimension
        data = index.data if grouped else index.vector_index.data
        pq = index.quantizer if grouped else index.vector_index.product_quantizer
        m, k = len(pq.quantizers), pq.num_clusters
        idx = data.indices()
        # without vectors: the shape and the code usage
        rep = wi.inspect()
        assert (rep.n, rep.d, rep.m, rep.k, rep.metric, rep.form) == (n, d, m, k, index.metric, kind)
        H = _bincount(idx, k, 0, n)
        assert rep.centroids_used == (H > 0).sum(axis=1).tolist()
        assert rep.largest_share == (H.max(axis=1) / n).tolist()
        assert rep.entropy == [entropy_bits(h) for h in H]
        assert rep.mean_row_error is None and rep.worst is None
        if grouped:
            sizes = np.diff(np.r_[0, index.offsets, n])
            assert (rep.groups, rep.group_size_min, rep.group_size_max) == (len(index.centroids), sizes.min(), sizes.max())
            assert rep.group_size_median == float(np.median(sizes)) and rep.group_size_min == 0
        else:
            assert rep.groups == 0 and rep.group_size_min is None
        # with vectors that hold the index's words among others, in another order
        all_words = sorted(words + ["a-first", "m-middle", "zz-last"])
        at = {w: i for i, w in enumerate(all_words)}
        V = np.random.default_rng(n).standard_normal((len(all_words), d)).astype(np.float32)
        vectors = DeviceWordVectors(all_words, g.DeviceMatrix.from_host(V), KeyIndexSorted(all_words))
        row_map = np.array([at[w] for w in words])
        dec = oracle.pq_decode(idx, d, k, pq.flat_centroids())
        if grouped:
            own = np.searchsorted(index.offsets, np.arange(n), side="right")
            dec = (index.centroids[own] + dec).astype(np.float32)
        err, nrm, p = _restate(g, V[row_map], dec, m)
        rep = wi.inspect(vectors, worst=7)
        assert rep.mean_row_error == float(err.astype(np.float64).sum()) / n
        assert rep.relative_error == float(err.astype(np.float64).sum()) / float(nrm.astype(np.float64).sum())
        for j in range(m):
            S = math.fsum(p[:, j].astype(np.float64).tolist())
            assert abs(rep.quantizer_mean_error[j] * n - S) <= (n + 1) * 2.0 ** -52 * S     # (+ the division and product)
        order = np.lexsort((np.arange(n), -err.astype(np.float64)))[:7]
        assert order[0] == int(np.argmax(err))
        assert rep.worst == [(int(r), float(err[r]), words[r]) for r in order]
        assert len(rep.lines()) == 1 + grouped + m + 2 + m + 7
        # a word the vectors lack, a wrong dimension: as RefinedIndex
        fewer = [w for w in all_words if w != words[5]]
        lacking = DeviceWordVectors(fewer, g.DeviceMatrix.from_host(V[:len(fewer)]), KeyIndexSorted(fewer))
        with pytest.raises(LookupError, match=f"the index holds the word '{words[5]}', the word vectors do not"):
            wi.inspect(lacking)
        with pytest.raises(LookupError, match=f"the index holds the word '{words[5]}', the word vectors do not"):
            wi.refined(lacking, 10)
        narrow = DeviceWordVectors(all_words, g.DeviceMatrix.from_host(V[:, :d - 1]), KeyIndexSorted(all_words))
        with pytest.raises(ValueError, match="vectors of dimension"):
            wi.inspect(narrow)
        wi.close()
    assert ("grouped", "cosine") in seen


# ---------------------------------------------------------------- 7. the reference's property
def test_more_clusters_and_quantizers_approximate_better(g):
    """ProductQuantizerSpec.scala:75-104, once.  k-means guarantees nothing, so the case is fixed: for oracle.synth kind 1,
    seed 42, 20 centres, 2000 x 16 and 5 iterations the oracle's own training, encoding and decoding give, with the
    reference's arithmetic on the CPU, quality 32095.8 at (m = 4, k = 16) and 4831.4 at (m = 8, k = 32) -- checked before
    the seed was written down here."""
    n, d = 2000, 16
    dm = g.DeviceMatrix.synthetic(n, d, 1, 42, 20)
    quality = []
    for m, k in ((4, 16), (8, 32)):
        pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(k, m, 5))
        index = g.Index.sorted(dm, pq)
        err, _ = index.row_errors(dm)
        quality.append(g.reference_quality(err))
        index.vector_index.close()
    print("quality", quality)
    assert quality[1] < quality[0]
    dm.close()


# ---------------------------------------------------------------- 8. handle history
def test_a_handle_answers_like_a_fresh_one_after_the_diagnostics(oracle, g):
    w = hh.world("m16")
    pq = g.ProductQuantizer.from_flat(w.k, w.d, w.m, w.cents)
    coder = pq.coder_factory(w.n)
    enc = g.EncodedMatrix(coder, [coder.build_code(w.idx[j]) for j in range(w.m)])
    used, fresh = g.PQIndex(pq, enc), g.PQIndex(pq, enc)
    dm = g.DeviceMatrix.synthetic(w.n, w.d, 0, 5, 1)
    try:
        assert np.array_equal(used.code_histogram(17, w.n - 9), _bincount(w.idx, w.k, 17, w.n - 9))
        used.row_errors(dm, np.arange(w.n - 1, -1, -1, dtype=np.int32), 64 * 5 + 17, w.n, norms=True)
        with pytest.raises(ValueError):
            used.row_errors(dm, np.full(w.n, w.n, np.int32))
        for call in hh.probes(w):
            Q = hh.queries(oracle, w, call)
            want = hh.expected(oracle, w, call)
            got = used.batch_query_raw(call.K, Q, call.frm, call.until)
            hh.same_answer(got, want)
            hh.same_as_fresh(got, fresh.batch_query_raw(call.K, Q, call.frm, call.until), want)
    finally:
        used.close()
        fresh.close()
        dm.close()
