"""Index views (subset.hip): a chosen subset of an index's rows as an index of its own, gathered on the device.

The contract: a view of P over rows r_0 < r_1 < ... equals the reference's PQIndex over the EncodedMatrix whose columns
are those rows -- `oracle.pq_batch_query(idx[:, rows], ...)` with the ids mapped through `rows`, bit for bit, flags and
order under ties as for any index."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits
from test_gpu_query import _check, _make

pytestmark = pytest.mark.gpu

LAYOUTS = {"vec16": (1000, 32, 16, 256),       # one 16-byte code word per row
           "vec4x2": (1000, 32, 8, 256),       # two 4-byte words per row
           "packed4": (1000, 32, 8, 16)}       # 4-bit codes in the file, one byte per quantizer on the device
N_ROWS = 1000
SELECTIONS = {
    "s0": np.zeros(0, np.int64),
    "s1": np.array([517]),
    "s63": np.sort(np.random.default_rng(63).choice(N_ROWS, 63, replace=False)),
    "s64": np.sort(np.random.default_rng(64).choice(N_ROWS, 64, replace=False)),
    "s65": np.sort(np.random.default_rng(65).choice(N_ROWS, 65, replace=False)),
    "identity": np.arange(N_ROWS),
    "first_last": np.array([0, N_ROWS - 1]),
    "every_third": np.arange(0, N_ROWS, 3),
    "straddle": np.concatenate([np.arange(60, 70), np.arange(250, 262)]),   # rows 63|64 and 255|256
}


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


_PARENTS = {}


def _parent(oracle, g, name):
    """One parent per layout for the whole module: (cents, idx, pq, PQIndex, queries)."""
    if name not in _PARENTS:
        n, d, m, k = LAYOUTS[name]
        cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=sum(map(ord, name)))
        Q = np.random.default_rng(17).standard_normal((8, d)).astype(np.float32)
        _PARENTS[name] = (cents, idx, pq, g.PQIndex(pq, enc), Q)
    return _PARENTS[name]


def _oracle_view(oracle, idx, rows, d, k, cents, Q, K, frm=0, until=None):
    """The oracle on the gathered codes, ids mapped through `rows`."""
    rows = np.asarray(rows, np.int64)
    sub = np.ascontiguousarray(idx[:, rows])
    oi, od, oc = oracle.pq_batch_query(sub, d, k, cents, Q, K, frm, len(rows) if until is None else until)
    oi = np.array(oi)
    for q in range(len(oc)):
        oi[q, :oc[q]] = rows[oi[q, :oc[q]]]
    return oi, od, oc


def _check_empty(res, raw, K):
    oi, od, oc, of = raw
    assert all(len(r) == 0 for r in res)
    assert not oc.any() and (oi == -1).all()


def _filter_stats(ix):
    from gulon_amd import native as N
    t, r = C.c_int32(-1), C.c_int32(-1)
    N.check(N.lib().gulon_index_filter_stats(ix._h, C.byref(t), C.byref(r)))
    return t.value, r.value


@pytest.mark.parametrize("selection", list(SELECTIONS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_view_layouts_and_edges(oracle, g, layout, selection):
    n, d, m, k = LAYOUTS[layout]
    cents, idx, pq, parent, Q = _parent(oracle, g, layout)
    rows = SELECTIONS[selection]
    s = len(rows)
    view = parent.select(rows=rows)
    assert isinstance(view, g.PQIndexView) and view.length == s
    assert view.rows.dtype == np.int32 and view.rows.tolist() == rows.tolist()
    assert np.array_equal(bits(view.decode_rows(np.arange(s))), bits(parent.decode_rows(rows)))
    for K in (1, 10, 63, 100):
        res = view.batch_query(K, Q)
        if s == 0:
            _check_empty(res, view.batch_query_raw(K, Q), K)
            continue
        _check(oracle, res, *_oracle_view(oracle, idx, rows, d, k, cents, Q, K))
        if selection == "identity":
            for a, b in zip(res, parent.batch_query(K, Q)):
                assert a.rows.tolist() == b.rows.tolist() and a.flags == b.flags
                assert np.array_equal(bits(a.distances), bits(b.distances))
    view.close()


@pytest.mark.parametrize("layout", ["vec16", "vec4x2"])
def test_view_codes_are_those_of_a_native_index(oracle, g, layout):
    """The library has no accessor for an index's plain code buffer: the bulk decode of both and queries whose from /
    until cut the ragged last block must agree instead."""
    n, d, m, k = LAYOUTS[layout]
    cents, idx, pq, parent, Q = _parent(oracle, g, layout)
    rows = np.sort(np.random.default_rng(3).choice(n, 333, replace=False))
    view = parent.select(rows=rows)
    coder = pq.coder_factory(len(rows))
    native = g.PQIndex(pq, g.EncodedMatrix(coder, [coder.build_code(idx[j, rows]) for j in range(m)]))
    a, b = view.decode_matrix(), native.decode_matrix()
    assert np.array_equal(bits(a.to_host()), bits(b.to_host()))
    a.close(), b.close()
    assert view.data == native.data
    for frm, until in ((0, 333), (70, 330), (320, 333), (321, 322)):
        for K in (10, 100):
            x, y = view.positions_raw(K, Q, frm, until), native.batch_query_raw(K, Q, frm, until)
            assert np.array_equal(x[0], y[0]) and np.array_equal(bits(x[1]), bits(y[1]))
            assert np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3])
    native.close()
    view.close()


def test_view_of_wide_codes(oracle, g):
    n, d, m, k = 1000, 32, 8, 1024
    cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=1024)
    parent = g.PQIndex(pq, enc)
    rows = np.sort(np.random.default_rng(4).choice(n, 333, replace=False))
    view = parent.select(rows=rows)
    assert np.array_equal(bits(view.decode_rows(np.arange(333))), bits(parent.decode_rows(rows)))
    Q = np.random.default_rng(6).standard_normal((8, d)).astype(np.float32)
    for K in (10, 100):
        _check(oracle, view.batch_query(K, Q), *_oracle_view(oracle, idx, rows, d, k, cents, Q, K))
    view.close()
    parent.close()


@pytest.mark.parametrize("n", [1000, 64 * 64 * 3 + 5])
def test_mask_forms(oracle, g, n):
    """A bool mask, a packed host mask and a device mask whose bits at and above n are garbage: the rows of
    np.flatnonzero, and the view of the row list.  64 * 64 * 3 + 5 rows: more than one group of 64 mask words."""
    import torch
    from gulon_amd.index import pack_mask
    d, m, k = 16, 8, 16
    cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=n)
    parent = g.PQIndex(pq, enc)
    keep = np.random.default_rng(n).random(n) < 0.4
    keep[[0, n - 1]] = True
    rows = np.flatnonzero(keep)
    packed = pack_mask(keep, n)
    dirty = packed.copy()
    dirty[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)        # n is no multiple of 64 here
    device = torch.from_numpy(dirty.view(np.int64)).cuda()
    want = parent.select(rows=rows)
    dec = want.decode_rows(np.arange(len(rows)))
    for mask in (keep, packed, dirty, device, device.view(torch.uint64)):
        view = parent.select(mask=mask)
        assert view.length == len(rows) and view.rows.tolist() == rows.tolist()
        assert np.array_equal(bits(view.decode_rows(np.arange(len(rows)))), bits(dec))
        view.close()
    empty = parent.select(mask=np.zeros(n, bool))
    assert empty.length == 0 and empty.rows.tolist() == []
    empty.close()
    full = parent.select(mask=np.ones(n, bool))
    assert full.rows.tolist() == list(range(n))
    full.close()
    want.close()
    parent.close()


def test_view_takes_the_filtered_path(oracle, g):
    n, d, m, k, B, K = 150000, 128, 16, 256, 32, 10
    cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=150)
    parent = g.PQIndex(pq, enc)
    keep = np.random.default_rng(47).random(n) < 0.47
    rows = np.flatnonzero(keep)
    s = len(rows)
    view = parent.select(mask=keep)
    Q = np.random.default_rng(8).standard_normal((B, d)).astype(np.float32)
    for frm, until in ((0, s), (1000, s - 777)):                          # the second cuts 256-row ordering windows
        res = view.batch_query(K, Q, frm, until)
        assert _filter_stats(view)[0] > 0
        _check(oracle, res, *_oracle_view(oracle, idx, rows, d, k, cents, Q, K, frm, until))
    view.close()
    parent.close()


def test_view_ties_are_replayed_in_the_reference_order(oracle, g):
    from gulon_amd import native as N
    n, d, m, k, K = 4096, 32, 8, 256, 10
    rng = np.random.default_rng(12)
    cents = rng.standard_normal(k * d).astype(np.float32)
    idx = np.ascontiguousarray(rng.integers(0, k, (m, 512)).astype(np.int32)[:, rng.integers(0, 512, n)])
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    coder = pq.coder_factory(n)
    parent = g.PQIndex(pq, g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(m)]))
    rows = np.flatnonzero(rng.random(n) < 0.6)
    view = parent.select(rows=rows)
    Q = np.concatenate([view.decode_rows(np.arange(0, 800, 100)), np.zeros((1, d), np.float32)])
    Q[8, 5] = np.nan
    res = view.batch_query(K, Q)
    oi, od, oc = _oracle_view(oracle, idx, rows, d, k, cents, Q, K)
    flagged = 0
    for q, r in enumerate(res[:8]):
        assert len(r) == oc[q] and np.array_equal(bits(r.distances), bits(od[q, :oc[q]]))
        if r.flags & (N.FLAG_BOUNDARY_TIE | N.FLAG_INTERIOR_TIE):
            flagged += 1
            assert r.flags & N.FLAG_EXACT_REPLAY
        assert r.rows.tolist() == oi[q, :oc[q]].tolist(), q              # ids AND order
    assert flagged >= 4                                                  # ~5 copies of every code among the rows kept
    assert res[8].flags & N.FLAG_NONFINITE and np.isnan(res[8].distances).all()
    assert res[8].rows.tolist() == oi[8, :oc[8]].tolist()
    view.close()
    parent.close()


def _dev_query(view, entry, Q, K, stream):
    """One *_dev batch query (torch tensors on `stream`) -> (idx, dist, count, flags) as numpy, and the idx tensor."""
    import torch
    from gulon_amd import native as N
    B = len(Q)
    with torch.cuda.stream(stream):
        q = torch.from_numpy(Q).cuda()
        oi = torch.zeros((B, K), dtype=torch.int32, device="cuda")
        od = torch.zeros((B, K), dtype=torch.float32, device="cuda")
        oc = torch.zeros(B, dtype=torch.int32, device="cuda")
        of = torch.zeros(B, dtype=torch.int32, device="cuda")
        N.check(entry(view._h, q.data_ptr(), B, K, 0, view.length, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                      of.data_ptr(), C.c_void_p(stream.cuda_stream)))
    return q, oi, od, oc, of


def test_views_of_views_contexts_and_lifetimes(oracle, g):
    import torch
    from gulon_amd import native as N
    n, d, m, k = LAYOUTS["vec16"]
    cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=77)
    parent = g.PQIndex(pq, enc, row_base=5000)
    Q = np.random.default_rng(9).standard_normal((8, d)).astype(np.float32)
    K = 10
    A = np.arange(1, n, 2)
    Bpos = np.array([0, 3, 63, 64, 65, 200, 499])
    va = parent.select(rows=A)
    vab = va.select(rows=Bpos)
    direct = parent.select(rows=A[Bpos])
    assert vab.rows.tolist() == A[Bpos].tolist() == direct.rows.tolist()
    x, y = vab.batch_query_raw(K, Q), direct.batch_query_raw(K, Q)
    assert np.array_equal(x[0], y[0]) and np.array_equal(bits(x[1]), bits(y[1])) and np.array_equal(x[2], y[2])
    # the ids are the root's: its row_base included, padding kept
    oi, od, oc = _oracle_view(oracle, idx, A[Bpos], d, k, cents, Q, K)
    assert (x[2] == 7).all() and (x[0][:, 7:] == -1).all()
    assert np.array_equal(x[0][:, :7], oi[:, :7] + 5000)
    # a view of a view by mask
    keep = np.zeros(len(A), bool)
    keep[Bpos] = True
    vmask = va.select(mask=keep)
    assert vmask.rows.tolist() == direct.rows.tolist()
    vmask.close(), vab.close(), direct.close()
    # a context of the view, on a second stream, answers as the view
    want = va.batch_query_raw(K, Q)
    ctx = va.context()
    assert ctx.length == va.length and ctx.rows.tolist() == A.tolist()
    stream = torch.cuda.Stream()
    _, ti, td, tc, tf = _dev_query(ctx, N.lib().gulon_index_view_batch_query_dev, Q, K, stream)
    stream.synchronize()
    assert np.array_equal(ti.cpu().numpy(), want[0]) and np.array_equal(bits(td.cpu().numpy()), bits(want[1]))
    assert np.array_equal(tc.cpu().numpy(), want[2]) and np.array_equal(tf.cpu().numpy(), want[3])
    got = ctx.batch_query_raw(K, Q)
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    # the parent goes first; the view and its context own what they read
    parent.close()
    again = va.batch_query_raw(K, Q)
    assert np.array_equal(again[0], want[0]) and np.array_equal(bits(again[1]), bits(want[1]))
    va.close()                                                   # the context keeps the view's buffers alive
    last = ctx.batch_query_raw(K, Q)
    assert np.array_equal(last[0], want[0]) and np.array_equal(bits(last[1]), bits(want[1]))
    ctx.close()


def test_select_errors(oracle, g):
    from gulon_amd import native as N
    cents, idx, pq, parent, Q = _parent(oracle, g, "vec4x2")
    n = N_ROWS
    for rows, position in (([5, 4, 6], 1), ([1, 2, 2, 3], 2), ([-1, 2], 0), ([3, 7, n], 2), ([0, 2 ** 40], 1)):
        with pytest.raises(ValueError, match=rf"rows\[{position}\]"):
            parent.select(rows=rows)
    with pytest.raises(ValueError):
        parent.select()
    with pytest.raises(ValueError):
        parent.select(rows=[1], mask=np.ones(n, bool))
    with pytest.raises(ValueError):
        parent.select(mask=np.ones(n + 1, bool))
    with pytest.raises(ValueError):
        parent.select(rows=[0.5, 2.0])
    out = np.zeros(n, np.int32)
    assert N.lib().gulon_index_view_rows(parent._h, out) == N.ERR_INVALID_ARGUMENT
    s, p = C.c_int32(0), C.c_void_p()
    assert N.lib().gulon_index_view_size(parent._h, C.byref(s)) == N.ERR_INVALID_ARGUMENT
    assert N.lib().gulon_index_view_rows_dev(parent._h, C.byref(p)) == N.ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError, match="not a view"):
        N.check(N.lib().gulon_index_view_batch_query(parent._h, Q.reshape(-1), 8, 1, 0, n, np.zeros(8, np.int32),
                                                     np.zeros(8, np.float32), np.zeros(8, np.int32),
                                                     np.zeros(8, np.int32)))


def test_map_rows_after_the_unmapped_answer(oracle, g):
    """positions_raw followed by gulon_index_view_map_rows_dev == batch_query_raw; -1 stays -1.  The same for the
    device form of the plain query, and for query by row."""
    import torch
    from gulon_amd import native as N
    cents, idx, pq, parent, Q = _parent(oracle, g, "packed4")
    rows = np.arange(2, N_ROWS, 50)                      # 20 rows, K = 63: 43 padding entries per query
    view = parent.select(rows=rows)
    K = 63
    want = view.batch_query_raw(K, Q)
    pos = view.positions_raw(K, Q)
    assert (pos[0][:, 20:] == -1).all() and (want[0][:, 20:] == -1).all() and (pos[2] == 20).all()
    assert np.array_equal(rows[pos[0][:, :20]], want[0][:, :20])
    t = torch.from_numpy(np.ascontiguousarray(pos[0])).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    N.check(N.lib().gulon_index_view_map_rows_dev(view._h, t.data_ptr(), t.numel(), st))
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), want[0])
    assert np.array_equal(view.map_positions(pos[0]), want[0])
    stream = torch.cuda.Stream()
    _, ti, td, tc, tf = _dev_query(view, N.lib().gulon_index_batch_query_dev, Q, K, stream)
    N.check(N.lib().gulon_index_view_map_rows_dev(view._h, ti.data_ptr(), ti.numel(), C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    assert np.array_equal(ti.cpu().numpy(), want[0]) and np.array_equal(bits(td.cpu().numpy()), bits(want[1]))
    # query by row: positions in, the root's ids out
    byrow = view.batch_query_rows_raw(5, [0, 19])
    byvec = view.batch_query_raw(5, view.decode_rows([0, 19]))
    assert np.array_equal(byrow[0], byvec[0]) and np.array_equal(bits(byrow[1]), bits(byvec[1]))
    # a sorted index over the view keeps the metric and answers in the parent's rows
    srt = g.SortedIndex(parent, "cosine").select(rows=rows)
    assert srt.metric == "cosine" and srt.size == 20
    assert set(srt.query(3, Q[0]).rows.tolist()) <= set(rows.tolist())
    srt.vector_index.close()
    view.close()
