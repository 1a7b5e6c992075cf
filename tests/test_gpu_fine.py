"""Fine codes on the device (csrc/fine.hip, gulon_amd/fine.py).  The residual matrix against V[vector_rows] - y[rows] in
numpy float32, bit for bit; gulon_*_refine_codes_topk against the heap restatement -- z = (y + f) in numpy float32, then
oracle.TopKHeap(k).update(id, oracle.distance_sq(q, z[id])) in list order -- over every code layout on either side; and
build_fine_index / FineRefinedIndex end to end over a sorted l2, a sorted cosine and a grouped index."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits
from test_gpu_refine import DIM, ITERS, K, M, N_ROWS, QUERIES, _assert_equal, _lists, _vectors

pytestmark = pytest.mark.gpu

F32 = np.float32
# name -> (m, k) of a code layout (m is cut to d where d is smaller): the device keeps 4-byte words unless m % 16 == 0,
# 16-bit codes above 256 centroids
LAYOUTS = {"vec4": (4, 16),          # one 4-byte word
           "vec16": (16, 256),       # one 16-byte word
           "ng": (6, 64),            # two 4-byte words, two padding quantizers
           "vec16x2": (32, 64),      # two 16-byte words
           "wide": (8, 1024),        # 16-bit codes
           "tiny16": (16, 8)}        # a 16-byte word over a tiny code book
# a leading empty group (the reference's) and interior empty groups: the offsets of test_gpu_inspect.py, where the
# binarySearch rule of GroupedIndex.lookup names another group than the row's own for some rows
GROUP_OFFSETS = [0, 5, 5, 5, 9, 40, 40, 100, 150, 150, 150, 220]


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def _shape(layout, d):
    m, k = LAYOUTS[layout]
    return min(m, d), k


def _codes(g, n, d, m, k, rng, scale=1.0):
    cents = (rng.standard_normal(k * d) * scale).astype(F32)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    return cents, idx


def _encoded(g, d, m, k, cents, idx):
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    coder = pq.coder_factory(idx.shape[1])
    return pq, g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(m)])


def _flat(g, d, m, k, cents, idx):
    return g.PQIndex(*_encoded(g, d, m, k, cents, idx))


def _own_group(offsets, n):
    """cluster_of: the group whose row range holds the row"""
    return np.searchsorted(np.asarray(offsets), np.arange(n), side="right")


def _same_bits(got, want, where):
    assert got.shape == want.shape and got.dtype == np.float32, where
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), where
    assert np.array_equal(bits(got[~nan]), bits(want[~nan])), where


# ---------------------------------------------------------------- 1. residuals
def _originals(n, d, rng):
    V = (rng.standard_normal((n + 37, d)) * 2).astype(F32)
    V[n + 7, d // 2] = np.nan                                       # a NaN row, +inf and -inf rows
    V[n + 8, 0], V[n + 9, d - 1] = np.inf, -np.inf
    return V


def _row_lists(n, nv, s, rng):
    """shuffled, repeated rows; the non-finite originals among the vector rows"""
    rows = rng.integers(0, n, s).astype(np.int32)
    vrows = rng.integers(0, nv, s).astype(np.int32)
    if s > 1:
        rows[1] = rows[0]
        vrows[-1] = vrows[0]
    if s:
        at = rng.choice(s, 3, replace=False) if s >= 3 else rng.integers(0, s, 3)
        vrows[at] = [nv - 37 + 7, nv - 37 + 8, nv - 37 + 9]
        rows[rng.integers(0, s)] = 0
        rows[rng.integers(0, s)] = n - 1
    return rows, vrows


RESIDUAL_SHAPES = [(1, 8, 4, 16), (65, 26, 4, 16), (1000, 32, 16, 256), (1000, 40, 20, 64), (1000, 32, 8, 1024)]
S_VALUES = (0, 1, 63, 64, 65, 1000)


@pytest.mark.parametrize("n,d,m,k", RESIDUAL_SHAPES)
def test_residuals_flat_bit_for_bit(g, oracle, n, d, m, k):
    from gulon_amd.fine import index_row_residuals
    rng = np.random.default_rng(n + d + m + k)
    cents, idx = _codes(g, n, d, m, k, rng)
    ix = _flat(g, d, m, k, cents, idx)
    Y = oracle.pq_decode(idx, d, k, cents)
    V = _originals(n, d, rng)
    dm = g.DeviceMatrix.from_host(V)
    seen_nan = False
    for s in S_VALUES:
        rows, vrows = _row_lists(n, len(V), s, rng)
        with np.errstate(invalid="ignore"):
            want = (V[vrows] - Y[rows]).astype(F32)
        E = index_row_residuals(ix, dm, rows, vrows)
        assert (E.rows, E.cols) == (s, d)
        got = E.to_host()
        _same_bits(got, want, (n, d, m, k, s))
        seen_nan = seen_nan or bool(np.isnan(want).any() and np.isinf(want).any())
        E.close()
    assert seen_nan
    # through a SortedIndex, the identity lists: every row against its own original
    E = index_row_residuals(g.SortedIndex(ix), dm, np.arange(n), np.arange(n))
    _same_bits(E.to_host(), (V[:n] - Y).astype(F32), "identity")
    E.close()
    ix.close()
    dm.close()


def _grouped(g, oracle, n, d, m, k, rng):
    cents, idx = _codes(g, n, d, m, k, rng)
    idx[:, 100:110] = idx[:, 100:101]                               # rows with identical codes inside one group
    idx[:, 200:203] = idx[:, 200:201]
    gc = (rng.standard_normal((len(GROUP_OFFSETS) + 1, d)) * 3).astype(F32)
    pq, enc = _encoded(g, d, m, k, cents, idx)
    gx = g.GroupedIndex(pq, enc, gc, np.asarray(GROUP_OFFSETS, np.int32), g.LimitGroups(4), "l2")
    Y = (gc[_own_group(GROUP_OFFSETS, n)] + oracle.pq_decode(idx, d, k, cents)).astype(F32)
    return gx, cents, idx, Y


@pytest.mark.parametrize("m,k", [(4, 16), (8, 1024)])
def test_residuals_grouped_use_the_rows_own_group(g, oracle, m, k):
    from gulon_amd.fine import index_row_residuals
    n, d = 1000, 26
    rng = np.random.default_rng(k)
    gx, cents, idx, Y = _grouped(g, oracle, n, d, m, k, rng)
    assert not np.array_equal(bits(Y), bits(gx.lookup_rows(np.arange(n))))      # not the binarySearch rule of lookup
    V = _originals(n, d, rng)
    dm = g.DeviceMatrix.from_host(V)
    for s in (0, 1, 65, 600):
        rows, vrows = _row_lists(n, len(V), s, rng)
        with np.errstate(invalid="ignore"):
            want = (V[vrows] - Y[rows]).astype(F32)
        E = index_row_residuals(gx, dm, rows, vrows)
        _same_bits(E.to_host(), want, (m, k, s))
        E.close()
    gx.close()
    dm.close()


def test_residuals_grouped_with_the_references_leading_empty_group(g, oracle):
    """A grouped index as the reference builds it: row 0 outside the lowest cluster gives a leading empty group."""
    from gulon_amd.fine import index_row_residuals
    n, d, m, k, clusters = 600, 16, 4, 16, 7
    rng = np.random.default_rng(600)
    assign = rng.integers(0, clusters, n).astype(np.int32)
    assign[0] = 3
    coarse = (rng.standard_normal((clusters, d)) * 3).astype(F32)
    perm, gc, offsets = oracle.group_rows(assign, coarse)
    assert offsets[0] == 0 and len(gc) == len(offsets) + 1 == clusters + 1
    cents, idx = _codes(g, n, d, m, k, rng)
    pq, enc = _encoded(g, d, m, k, cents, idx)
    gx = g.GroupedIndex(pq, enc, gc, offsets, g.LimitGroups(4), "l2")
    Y = (gc[_own_group(offsets, n)] + oracle.pq_decode(idx, d, k, cents)).astype(F32)
    V = _originals(n, d, rng)
    dm = g.DeviceMatrix.from_host(V)
    rows, vrows = _row_lists(n, len(V), n, rng)
    E = index_row_residuals(gx, dm, rows, vrows)
    with np.errstate(invalid="ignore"):
        _same_bits(E.to_host(), (V[vrows] - Y[rows]).astype(F32), "reference grouping")
    E.close()
    gx.close()
    dm.close()


def test_residuals_of_a_view_are_in_its_own_positions(g, oracle):
    from gulon_amd.fine import index_row_residuals
    n, d, m, k = 1000, 32, 16, 256
    rng = np.random.default_rng(3)
    cents, idx = _codes(g, n, d, m, k, rng)
    parent = _flat(g, d, m, k, cents, idx)
    sel = np.arange(0, n, 3)
    view = parent.select(rows=sel)
    Y = oracle.pq_decode(np.ascontiguousarray(idx[:, sel]), d, k, cents)
    V = _originals(n, d, rng)
    dm = g.DeviceMatrix.from_host(V)
    rows, vrows = _row_lists(len(sel), len(V), 200, rng)
    E = index_row_residuals(view, dm, rows, vrows)
    with np.errstate(invalid="ignore"):
        _same_bits(E.to_host(), (V[vrows] - Y[rows]).astype(F32), "view")
    with pytest.raises(ValueError, match=r"rows\[0\] = %d outside" % len(sel)):
        index_row_residuals(view, dm, [len(sel)], [0])
    E.close()
    view.close()
    parent.close()
    dm.close()


def test_residuals_reject_bad_arguments(g):
    from gulon_amd.fine import index_row_residuals
    N = g.native
    n, d, m, k = 200, 32, 8, 256
    rng = np.random.default_rng(9)
    cents, idx = _codes(g, n, d, m, k, rng)
    ix = _flat(g, d, m, k, cents, idx)
    V = rng.standard_normal((150, d)).astype(F32)
    dm = g.DeviceMatrix.from_host(V)
    for bad in (n, -1, 2 ** 31 - 1):
        rows = np.arange(100, dtype=np.int32)
        rows[31] = bad
        rows[77] = -5                                               # the FIRST offending position is named
        with pytest.raises(ValueError, match=r"rows\[31\] = %d outside \[0, 200\)" % bad):
            index_row_residuals(ix, dm, rows, np.arange(100))
    for bad in (150, -1):
        vrows = np.arange(100, dtype=np.int32)
        vrows[42] = bad
        with pytest.raises(ValueError, match=r"vector_rows\[42\] = %d outside \[0, 150\)" % bad):
            index_row_residuals(ix, dm, np.arange(100), vrows)
    narrow = g.DeviceMatrix.from_host(V[:, :d - 4])
    with pytest.raises(ValueError, match="dimension"):
        index_row_residuals(ix, narrow, [0], [0])
    with pytest.raises(ValueError):
        index_row_residuals(ix, dm, [0, 1], [0])
    out = C.c_void_p()
    one = np.zeros(1, np.int32)
    assert N.lib().gulon_index_row_residuals(None, dm._h, one, one, 1, C.byref(out)) == N.ERR_INVALID_ARGUMENT
    assert N.lib().gulon_index_row_residuals(ix._h, None, one, one, 1, C.byref(out)) == N.ERR_INVALID_ARGUMENT
    assert N.lib().gulon_index_row_residuals(ix._h, dm._h, one, one, 1, None) == N.ERR_INVALID_ARGUMENT
    assert N.lib().gulon_grouped_index_row_residuals(None, dm._h, one, one, 1, C.byref(out)) == N.ERR_INVALID_ARGUMENT
    assert N.lib().gulon_index_row_residuals(ix._h, dm._h, one, one, -1, C.byref(out)) == N.ERR_INVALID_ARGUMENT
    narrow.close()
    ix.close()
    dm.close()


# ---------------------------------------------------------------- 2. re-ranking against codes
N_RERANK = 1000


class _Pair:
    """A coarse index (flat layout or grouped) and a fine index of another shape over N_RERANK ids, with the restated
    two-level reconstruction Z[id].  Rows 100..109 and 200..202 carry identical coarse AND fine codes (ties); ids 7, 8, 9
    decode to a NaN, a +inf and a -inf through planted fine code-book entries.  `fine` holds the fine rows in id order,
    `fine_mapped` holds row perm[id] for id (and five spare rows)."""

    def __init__(self, g, oracle, d, coarse, fine, seed):
        n = N_RERANK
        rng = np.random.default_rng(seed)
        self.g, self.d, self.grouped = g, d, coarse == "grouped"
        if self.grouped:
            m1, k1 = _shape("vec16" if d >= 16 else "vec4", d)
            self.coarse, _, _, Y = _grouped(g, oracle, n, d, m1, k1, rng)
        else:
            m1, k1 = _shape(coarse, d)
            cents, idx = _codes(g, n, d, m1, k1, rng)
            idx[:, 100:110] = idx[:, 100:101]
            idx[:, 200:203] = idx[:, 200:201]
            self.coarse = _flat(g, d, m1, k1, cents, idx)
            Y = oracle.pq_decode(idx, d, k1, cents)
        m2, k2 = _shape(fine, d)
        assert (m2, k2) != (m1, k1)
        fcents, fidx = _codes(g, n, d, m2, k2, rng, scale=0.25)
        fidx[0] = rng.integers(0, k2 - 3, n)
        fidx[0, 7], fidx[0, 8], fidx[0, 9] = k2 - 1, k2 - 2, k2 - 3
        fidx[:, 100:110] = fidx[:, 100:101]
        fidx[:, 200:203] = fidx[:, 200:201]
        s0 = -(-d // m2)                                            # the width of quantizer 0
        fcents[(k2 - 1) * s0], fcents[(k2 - 2) * s0], fcents[(k2 - 3) * s0] = np.nan, np.inf, -np.inf
        self.fine = _flat(g, d, m2, k2, fcents, fidx)
        self.perm = rng.permutation(n + 5)[:n].astype(np.int32)
        mapped = rng.integers(0, k2 - 3, (m2, n + 5)).astype(np.int32)
        mapped[:, self.perm] = fidx
        self.fine_mapped = _flat(g, d, m2, k2, fcents, mapped)
        with np.errstate(invalid="ignore"):
            self.Z = (Y + oracle.pq_decode(fidx, d, k2, fcents)).astype(F32)     # y first, the fine coordinate last
        assert np.isnan(self.Z[7]).any() and np.isinf(self.Z[8]).any() and np.isinf(self.Z[9]).any()
        assert np.array_equal(bits(self.Z[100]), bits(self.Z[109])) and np.isfinite(self.Z[10:]).all()

    def close(self):
        for ix in (self.coarse, self.fine, self.fine_mapped):
            ix.close()


def _restate(oracle, k, query, cand, Z):
    """The definition: heap = TopKHeap(k); update(id, distanceSq(query, z[id])) in list order, negative ids skipped;
    Result.fromHeap."""
    heap = oracle.TopKHeap(k)
    for r in cand.tolist():
        if r >= 0:
            heap.update(r, oracle.distance_sq(query, Z[r]))
    return heap.drain()


RERANK_CASES = [
    (1, 1, 1, 1, "vec4", "wide"), (7, 17, 63, 10, "ng", "wide"), (48, 17, 64, 64, "vec16", "vec4"),
    (300, 17, 100, 63, "wide", "vec16x2"), (48, 1000, 100, 10, "grouped", "ng"), (26, 17, 1000, 64, "vec4", "ng"),
    (48, 17, 8191, 1000, "vec16x2", "wide"), (4100, 17, 100, 100, "vec4", "tiny16"),
    # every coarse layout at one shape, the fine layout rotating
    (48, 17, 100, 10, "vec4", "vec16"), (48, 17, 100, 10, "vec16", "ng"), (48, 17, 100, 10, "ng", "vec16x2"),
    (48, 17, 100, 10, "vec16x2", "vec4"), (48, 17, 100, 10, "wide", "vec4"), (48, 17, 100, 10, "grouped", "wide"),
    (7, 17, 63, 10, "grouped", "ng"), (48, 17, 1000, 64, "grouped", "vec4"),
    # two walks of different layouts in one lane at d % 4 != 0; one pass of 256 lanes, 186 of them without a candidate
    (26, 3, 70, 5, "wide", "vec4"),
]


@pytest.mark.parametrize("d,b,c,k,coarse,fine", RERANK_CASES)
def test_rerank_equals_the_heap_restatement(g, oracle, d, b, c, k, coarse, fine):
    from gulon_amd.fine import refine_codes_topk
    rng = np.random.default_rng(1000 * d + b + c + k)
    pair = _Pair(g, oracle, d, coarse, fine, seed=d + c)
    Q = rng.standard_normal((b, d)).astype(F32)
    cand = _lists(b, c, N_RERANK, rng)
    want = [_restate(oracle, k, Q[q], cand[q], pair.Z) for q in range(b)]
    assert any(np.isnan(ds).any() for _, ds in want) or c == 1
    _assert_equal(refine_codes_topk(pair.coarse, pair.fine, Q, cand, k), want, "identity")
    _assert_equal(refine_codes_topk(pair.coarse, pair.fine_mapped, Q, cand, k, fine_map=pair.perm), want, "mapped")
    if not pair.grouped:                                            # a SortedIndex on either side is the same handle
        got = refine_codes_topk(g.SortedIndex(pair.coarse), g.SortedIndex(pair.fine), Q, cand, k)
        _assert_equal(got, want, "sorted")
    pair.close()


def test_a_nan_inside_the_heap_lets_the_root_rise(g, oracle):
    """test_gpu_refine's sequence, reached through codes: d = 1, one quantizer on either side, the coarse entry 0 and
    the fine entry the square root of 5, 1, NaN, 0.5, 0.25, 3, 9, 7, 4, 7, 8.5, 100, 2."""
    from gulon_amd.fine import refine_codes_topk
    d2 = np.asarray([5, 1, np.nan, 0.5, 0.25, 3, 9, 7, 4, 7, 8.5, 100, 2], F32)
    n = len(d2)
    fcents = np.zeros(16, F32)
    fcents[:n] = np.sqrt(d2)
    fine = _flat(g, 1, 1, 16, fcents, np.arange(n, dtype=np.int32).reshape(1, n))
    coarse = _flat(g, 1, 1, 1024, np.zeros(1024, F32), np.full((1, n), 5, np.int32))
    Z = (np.zeros((n, 1), F32) + fcents[:n, None]).astype(F32)
    cand = np.arange(n, dtype=np.int32).reshape(1, -1)
    Q = np.zeros((1, 1), F32)
    ids, ds = _restate(oracle, 7, Q[0], cand[0], Z)
    assert 9 in ids.tolist() and 7 not in ids.tolist()
    _assert_equal(refine_codes_topk(coarse, fine, Q, cand, 7), [(ids, ds)], "nan")
    coarse.close()
    fine.close()


@pytest.mark.parametrize("coarse,c,k", [("vec16", 100, 10), ("grouped", 1000, 200)])
def test_device_form_on_a_stream_equals_the_host_form(g, oracle, coarse, c, k):
    import torch
    from gulon_amd.fine import _handle, refine_codes_topk
    N = g.native
    d, b, n = 48, 33, N_RERANK
    rng = np.random.default_rng(c)
    pair = _Pair(g, oracle, d, coarse, "ng", seed=c)
    Q = rng.standard_normal((b, d)).astype(F32)
    cand = _lists(b, c, n, rng)
    host = refine_codes_topk(pair.coarse, pair.fine_mapped, Q, cand, k, fine_map=pair.perm)
    fn = N.lib().gulon_grouped_index_refine_codes_topk_dev if pair.grouped else N.lib().gulon_index_refine_codes_topk_dev
    dev = torch.device("cuda:0")
    tq, tc, tm = (torch.from_numpy(a).to(dev) for a in (Q, cand, pair.perm))
    oi = torch.full((b, k), -7, dtype=torch.int32, device=dev)
    od = torch.full((b, k), -7.0, dtype=torch.float32, device=dev)
    oc = torch.full((b,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()

    def run():
        with torch.cuda.stream(stream):
            N.check(fn(_handle(pair.coarse)[0], pair.fine_mapped._h, tq.data_ptr(), b, tc.data_ptr(), c, tm.data_ptr(), n,
                       k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
    run()
    assert np.array_equal(oc.cpu().numpy(), host[2]) and np.array_equal(oi.cpu().numpy(), host[0])
    assert np.array_equal(od.cpu().numpy().view(np.uint32), host[1].view(np.uint32))
    # the status word: a candidate outside the coarse index marks its query with -1 and leaves the others alone
    tc[5, 0] = n
    run()
    counts = oc.cpu().numpy()
    assert counts[5] == -1 and np.array_equal(np.delete(counts, 5), np.delete(host[2], 5))
    pair.close()


def test_rerank_rejects_bad_arguments(g, oracle):
    from gulon_amd.fine import refine_codes_topk
    d, n = 8, 10
    rng = np.random.default_rng(1)
    cents, idx = _codes(g, n, d, 4, 16, rng)
    coarse = _flat(g, d, 4, 16, cents, idx)
    fcents, fidx = _codes(g, n, d, 2, 1024, rng)
    fine = _flat(g, d, 2, 1024, fcents, fidx)
    short = _flat(g, d, 2, 1024, fcents, fidx[:, :9])
    other = _flat(g, 12, 2, 1024, rng.standard_normal(1024 * 12).astype(F32), fidx)
    Q = rng.standard_normal((3, d)).astype(F32)
    cand = np.asarray([[0, 1, 2], [3, 10, 4], [5, 6, -1]], np.int32)             # 10 == n
    with pytest.raises(ValueError, match="row 10 out of range"):
        refine_codes_topk(coarse, fine, Q, cand, 2)
    cand[1, 1] = 9
    rows, dist, counts = refine_codes_topk(coarse, fine, Q, cand, 2)
    assert counts.tolist() == [2, 2, 2] and set(rows[1].tolist()) <= {3, 9, 4}
    with pytest.raises(ValueError, match="outside the fine map"):
        refine_codes_topk(coarse, fine, Q, cand, 2, fine_map=np.arange(9, dtype=np.int32))   # candidate 9, 9 entries
    with pytest.raises(ValueError, match="fine row 9 out of range"):
        refine_codes_topk(coarse, short, Q, cand, 2)                             # the identity leads outside `fine`
    for bad in (10, -1):
        fmap = np.arange(10, dtype=np.int32)
        fmap[5] = bad
        with pytest.raises(ValueError, match="fine row %d out of range" % bad):
            refine_codes_topk(coarse, fine, Q, cand, 2, fine_map=fmap)
    for k in (0, 4):                                                             # 1 <= k <= c
        with pytest.raises(ValueError):
            refine_codes_topk(coarse, fine, Q, cand, k)
    with pytest.raises(NotImplementedError):
        refine_codes_topk(coarse, fine, Q, np.zeros((3, 8192), np.int32), 1)
    with pytest.raises(ValueError, match="dimension"):
        refine_codes_topk(coarse, other, Q, cand, 2)
    assert [a.shape for a in refine_codes_topk(coarse, fine, Q[:0], cand[:0], 2)] == [(0, 2), (0, 2), (0,)]
    for ix in (coarse, fine, short, other):
        ix.close()


# ---------------------------------------------------------------- 3. end to end
K2, M2 = 256, 12
CASES = [(10, 100), (1, 1), (63, 64), (100, 10)]          # (k, c)


def _index_y(oracle, index):
    """y_r of every row of a WordIndex, restated from its codes."""
    ix = index.index
    if index._grouped:
        dec = oracle.pq_decode(ix.data.indices(), DIM, K, ix.quantizer.flat_centroids())
        return (ix.centroids[_own_group(ix.offsets, index.size)] + dec).astype(F32)
    vi = ix.vector_index
    return oracle.pq_decode(vi.data.indices(), DIM, K, vi.product_quantizer.flat_centroids())


@pytest.fixture(scope="module")
def world(g, oracle):
    """name -> dict(index, vectors, V, prepared, fine, Y, E, fmap, Z) for a sorted l2, a sorted cosine and a grouped
    WordIndex over the vectors of test_gpu_refine.py, each with its fine index (k = 256, m = 12, 5 iterations)."""
    from gulon_amd.build import Partitioned, build_index
    from gulon_amd.fine import build_fine_index
    from gulon_amd.product_quantizer import Config
    from gulon_amd.word_vectors import DeviceWordVectors, KeyIndexSorted
    X, Q, words = _vectors()
    Xn = np.stack([oracle.normalize(r) for r in X])
    Qn = np.stack([oracle.normalize(r) for r in Q])
    out = {"Q": Q, "words": words}
    for name, metric, part, V, prepared in (("l2", "l2", None, X, Q), ("cosine", "cosine", None, Xn, Qn),
                                            ("grouped", "l2", Partitioned(12, 3), X, Q)):
        vectors = DeviceWordVectors(words, g.DeviceMatrix.from_host(V), KeyIndexSorted(words))
        index_words, ix = build_index(vectors, metric, part, Config(K, M, ITERS))
        index = g.WordIndex(index_words, ix)
        log = []
        fine = build_fine_index(index, vectors, Config(K2, M2, ITERS), write=log.append)
        Y = _index_y(oracle, index)
        row_of = {w: r for r, w in enumerate(index.words)}
        rows = np.asarray([row_of[w] for w in words])               # the words ascend: sorted word t = words[t] = row t of V
        E = (V - Y[rows]).astype(F32)
        fmap = np.asarray([int(w[1:]) for w in index.words], np.int32)           # "w00042" is row 42 of the fine index
        fv = fine.index.vector_index
        Z = (Y + oracle.pq_decode(fv.data.indices(), DIM, K2, fv.product_quantizer.flat_centroids())[fmap]).astype(F32)
        out[name] = dict(index=index, vectors=vectors, V=V, prepared=prepared, fine=fine, Y=Y, E=E, fmap=fmap, Z=Z,
                         log="".join(log))
    return out


@pytest.mark.parametrize("name", ["l2", "cosine", "grouped"])
def test_fine_index_is_the_references_build_over_the_residuals(g, oracle, world, name):
    from gulon_amd.fine import row_residuals
    from gulon_amd.index_file import dump_index
    w = world[name]
    fine, E = w["fine"], w["E"]
    assert fine.words == world["words"] and fine.metric == "l2" and not fine._grouped
    assert (fine.size, fine.dimension) == (N_ROWS, DIM)
    assert (name == "grouped") == (not np.array_equal(w["fmap"], np.arange(N_ROWS)))
    res = row_residuals(w["index"], w["vectors"])
    assert res.words == world["words"]
    _same_bits(res.matrix.to_host(), E, name)
    res.matrix.close()
    cents, _, _ = oracle.pq_train(E, M2, K2, ITERS)
    fv = fine.index.vector_index
    assert np.array_equal(bits(fv.product_quantizer.flat_centroids()), bits(cents)), "code books differ"
    assert np.array_equal(fv.data.indices(), oracle.pq_encode(E, M2, K2, cents)), "codes differ"
    for line in ("Computing residuals", "Quantizing word vectors", f"Built index for {N_ROWS} word vectors"):
        assert line in w["log"]
    again = g.WordIndex.load(dump_index(fine.index, fine.words))
    assert again.words == fine.words and again.metric == "l2" and not again._grouped
    av = again.index.vector_index
    assert np.array_equal(av.data.indices(), fv.data.indices())
    assert np.array_equal(bits(av.product_quantizer.flat_centroids()), bits(cents))
    again.close()


@pytest.mark.parametrize("name", ["l2", "cosine", "grouped"])
def test_fine_refined_index_equals_the_restatement(g, oracle, world, name):
    w = world[name]
    index, fine, Z, prepared, Q = w["index"], w["fine"], w["Z"], w["prepared"], world["Q"]
    refined = index.fine_refined(fine, 50)
    assert (refined.size, refined.dimension, refined.metric) == (index.size, DIM, index.metric)
    assert refined.words is index.words and refined.row_of(index.words[5]) == 5
    for k, c in CASES:
        c_eff = max(c, k)
        gi, _, gc, flags = index.batch_query_raw(c_eff, Q)          # the index's own candidates
        want = [_restate(oracle, k, prepared[q], gi[q, :gc[q]], Z) for q in range(QUERIES)]
        got = refined.batch_query_raw(k, Q, candidates=c)
        assert np.array_equal(got[3], flags)
        _assert_equal(got[:3], want, (name, k, c))
        results = refined.batch_query(k, Q[:9], candidates=c)
        assert [r.rows.tolist() for r in results] == [want[q][0].tolist() for q in range(9)]
        assert results[0].words == [index.words[i] for i in want[0][0]]
        one = refined.query(k, Q[3], candidates=c)
        assert one.rows.tolist() == want[3][0].tolist() and np.array_equal(bits(one.distances), bits(want[3][1]))
        # by word: the index's decoded vector as the query
        asked = [index.words[5], "no such word", index.words[4000]]
        by_word = refined.batch_query_by_words(k, asked, candidates=c)
        assert by_word[1] is None
        assert refined.query_by_word(k, asked[2], candidates=c).rows.tolist() == by_word[2].rows.tolist()
        for word, res in ((asked[0], by_word[0]), (asked[2], by_word[2])):
            decoded = index.lookup(word)
            if index.metric == "cosine":
                decoded = oracle.normalize(decoded)
            ids, ds = _restate(oracle, k, decoded, index.query_by_word(c_eff, word).rows, Z)
            assert res.rows.tolist() == ids.tolist() and np.array_equal(bits(res.distances), bits(ds)), (name, k, c, word)
        # expressions: the composed vector as the query, the operands dropped by the index
        texts = [f"{index.words[10]} - {index.words[20]} + {index.words[30]}", "nosuchword + " + index.words[1],
                 index.words[77]]
        by_expr = refined.batch_query_expressions(k, texts, candidates=c)
        assert by_expr[1] is None
        assert refined.query_expression(k, texts[2], candidates=c).rows.tolist() == by_expr[2].rows.tolist()
        for text, res in ((texts[0], by_expr[0]), (texts[2], by_expr[2])):
            resolved = index.resolve_expressions([text])
            composed = index.index.compose_rows(resolved)[0]
            ids, ds = _restate(oracle, k, composed, index.query_expression(c_eff, text).rows, Z)
            assert res.rows.tolist() == ids.tolist() and np.array_equal(bits(res.distances), bits(ds)), (name, k, c, text)
    refined.close()


def test_fine_refined_index_checks_its_fine_index(g, world):
    from gulon_amd.word_index import WordIndex
    l2, grouped = world["l2"], world["grouped"]
    with pytest.raises(ValueError, match="sorted l2"):
        l2["index"].fine_refined(grouped["index"], 10)
    with pytest.raises(ValueError, match="sorted l2"):
        l2["index"].fine_refined(world["cosine"]["index"], 10)
    with pytest.raises(ValueError, match="candidates"):
        l2["index"].fine_refined(l2["fine"], 0)
    fewer = WordIndex(l2["fine"].words[1:], l2["fine"].index.select(rows=np.arange(1, N_ROWS)))
    with pytest.raises(LookupError, match="the index holds the word 'w00000', the fine index does not"):
        l2["index"].fine_refined(fewer, 10)
    fewer.close()
    restricted = l2["index"].restrict(l2["index"].words[:100])
    with pytest.raises(NotImplementedError, match="fine_refined is not supported by a restricted index"):
        restricted.fine_refined(l2["fine"], 10)
    restricted.close()


@pytest.mark.parametrize("name", ["l2", "grouped"])
def test_handles_that_served_fine_queries_answer_like_fresh_ones(g, world, name):
    """The calls use scratch of their own: a coarse and a fine index that served fine queries answer plain queries as
    freshly loaded copies of them do."""
    from gulon_amd.index_file import dump_index
    w = world[name]
    index, fine, Q = w["index"], w["fine"], world["Q"]
    refined = index.fine_refined(fine, 100)
    for k, c in CASES:
        refined.batch_query_raw(k, Q, candidates=c)
    refined.batch_query_by_words(5, index.words[:40])
    refined.close()
    for used in (index, fine):
        fresh = g.WordIndex.load(dump_index(used.index, used.words))
        for k in (1, 10, 100):
            a, b = used.batch_query_raw(k, Q), fresh.batch_query_raw(k, Q)
            assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
            assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        assert np.array_equal(bits(used.lookup(used.words[9])), bits(fresh.lookup(fresh.words[9])))
        fresh.close()


def _sum_distance_sq(oracle, A, B):
    return sum(float(oracle.distance_sq(a, b)) for a, b in zip(A, B))


def test_the_fine_level_lowers_the_reconstruction_error(g, oracle, world):
    """sum_r distanceSq(V_r, z_r) < sum_r distanceSq(V_r, y_r): every fine centroid is the mean of its cluster and the
    encoding picks the nearest one, so this holds for any data up to rounding; strictly on this clustered fixture."""
    w = world["l2"]
    V, Y, Z = w["V"], w["Y"], w["Z"]
    coarse, two_level = _sum_distance_sq(oracle, V, Y), _sum_distance_sq(oracle, V, Z)
    print("sum of squared errors: coarse", coarse, "two-level", two_level)
    assert two_level < coarse
