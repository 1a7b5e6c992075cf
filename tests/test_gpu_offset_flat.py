"""Offset queries on the flat byte-code index (csrc/offset.hip, gulon_index_query_offset): rows and key
BITS against csls.offset_query_reference over the handle's own distances -- its ordinary query at k = the rows of the
range.

Shapes: 256 centroids, m = 3 (one 4-byte code word) and m = 16 (one 16-byte word); 64 * 5 + 7 rows and the range
[5, n - 3), so neither end is on a 64-row code block; batches of 5 (eight query slots to a workgroup, three idle), 3, 2
and 1 (four, two and one slot).  A second world of 70 code blocks is cut into two row chunks.  Twenty rows are copies of
others with the same offset, so equal keys occur; a tenth of the offsets are +inf; every other query excludes the row it
was made from.  Rows of several code words, E bound by the LDS, two passes, three row chunks, tie groups larger than a
list, negative and non-finite keys and a row base: test_gpu_offset_paths.py."""
import numpy as np
import pytest

from cosmul_ref import unit_rows
from offset_ref import distances_by_row, draw_offsets, padded, run_dev, same

pytestmark = pytest.mark.gpu

N = 64 * 5 + 7
D, K, ITERS = 32, 256, 2
TWINS = [(20 + i, 200 + i) for i in range(20)]
DEPTHS = (1, 10, 63)


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


_WORLDS = {}


def world(g, m, n=N, b=5):
    """A trained PQIndex over n unit rows, queries made from rows of [5, n - 3), the rows they exclude, and the distances
    [b][n - 8] of the handle's ordinary query over that range."""
    key = (m, n, b)
    if key not in _WORLDS:
        X = unit_rows(3 * m + n, n, D)
        for a, c in TWINS:
            X[c] = X[a]
        dm = g.DeviceMatrix.from_host(X)
        pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(K, m, ITERS))
        vi = g.Index.sorted(dm, pq, "l2").vector_index
        rng = np.random.default_rng(m + b)
        made_from = rng.integers(5, n - 3, b)
        made_from[-1] = 20                                        # a twin, not excluded when b is odd
        Q = (X[made_from] + rng.standard_normal((b, D)).astype(np.float32) * np.float32(0.05)).astype(np.float32)
        exclude = np.where(np.arange(b) % 2 == 1, made_from, -1).astype(np.int32)
        ids = np.arange(5, n - 3)
        dist = distances_by_row(vi.batch_query_raw(len(ids), Q, 5, n - 3), ids)
        _WORLDS[key] = {"vi": vi, "Q": Q, "exclude": exclude, "dist": dist, "ids": ids, "n": n}
    return _WORLDS[key]


def reference(g, w, offsets, k, exclude):
    return g.offset_query_reference(w["dist"], offsets[5:w["n"] - 3], k, exclude, rows=w["ids"])


def ask(w, k, offsets, exclude):
    return w["vi"].batch_query_offset_raw(k, w["Q"], offsets, exclude, 5, w["n"] - 3)


@pytest.mark.parametrize("k", DEPTHS)
@pytest.mark.parametrize("b", (5, 1))
@pytest.mark.parametrize("m", (3, 16))
def test_host_form_matches_the_reference(g, m, b, k):
    w = world(g, m, b=b)
    offsets = draw_offsets(31 + m, N, TWINS)
    offsets[[20, 200]] = 0.5                                     # the twins next to the last query are candidates
    got = ask(w, k, offsets, w["exclude"])
    same(got, reference(g, w, offsets, k, w["exclude"]))
    assert padded(got)
    if k > 1:                                                    # the last query: rows 20 and 200 tie, 20 first
        rows, keys = got[0][b - 1].tolist(), got[1][b - 1]
        assert rows.index(20) + 1 == rows.index(200) and keys[rows.index(20)] == keys[rows.index(200)]
    for q in range(b):
        live = got[0][q, :got[2][q]]
        assert np.isfinite(offsets[live]).all() and w["exclude"][q] not in live.tolist()
        assert live.min() >= 5 and live.max() < N - 3


@pytest.mark.parametrize("b", (3, 2))
def test_four_and_two_query_slots(g, b):
    w = world(g, 16, b=b)
    offsets = draw_offsets(37, N, TWINS)
    same(ask(w, 10, offsets, w["exclude"]), reference(g, w, offsets, 10, w["exclude"]))


@pytest.mark.parametrize("k", DEPTHS)
@pytest.mark.parametrize("m", (3, 16))
def test_dev_form_matches_the_reference(g, m, k):
    w = world(g, m)
    offsets = draw_offsets(41 + m, N, TWINS)
    L = g.native.lib()

    def call(d_q, b, kk, d_off, d_ex, d_oi, d_ok, d_oc):
        return L.gulon_index_query_offset_dev(w["vi"]._h, d_q, b, kk, 5, N - 3, d_off, d_ex, d_oi, d_ok, d_oc, None)
    same(run_dev(g, call, w["Q"], k, offsets, w["exclude"]), reference(g, w, offsets, k, w["exclude"]))
    same(run_dev(g, call, w["Q"], k, offsets, None), reference(g, w, offsets, k, None))


def test_two_row_chunks(g):
    """70 code blocks: the launcher cuts them into two chunks, whose lists are merged."""
    n = 64 * 70 + 7
    w = world(g, 16, n=n)
    offsets = draw_offsets(43, n, TWINS)
    same(ask(w, 10, offsets, w["exclude"]), reference(g, w, offsets, 10, w["exclude"]))
    dev = g.DeviceOffsets.from_host(offsets)
    try:
        same(ask(w, 63, dev, None), reference(g, w, offsets, 63, None))
    finally:
        dev.free()


@pytest.mark.parametrize("k", (10, 63))
def test_fewer_candidates_than_k(g, k):
    w = world(g, 16)
    offsets = draw_offsets(47, N, keep=(5, 63, 64, 200, N - 4))
    offsets[[0, 4, N - 3, N - 1]] = 0.0                          # finite, but outside the range
    got = ask(w, k, offsets, None)
    same(got, reference(g, w, offsets, k, None))
    assert got[2].tolist() == [5] * 5 and padded(got)
    exclude = np.full(5, 64, np.int32)
    got = ask(w, k, offsets, exclude)
    same(got, reference(g, w, offsets, k, exclude))
    assert got[2].tolist() == [4] * 5


def test_a_used_handle_answers_the_same_and_the_sorted_index_prepares(g):
    w = world(g, 3)
    offsets = draw_offsets(53, N, TWINS)
    first = ask(w, 10, offsets, w["exclude"])
    w["vi"].batch_query_raw(5, w["Q"])
    w["vi"].batch_query_raw(100, w["Q"][:2])
    same(ask(w, 10, offsets, w["exclude"]), first)
    same(first, reference(g, w, offsets, 10, w["exclude"]))
    # a cosine SortedIndex over the same handle normalises its queries first, as its ordinary query does
    cosine = g.SortedIndex(w["vi"], "cosine")
    scaled = w["Q"] * np.float32(3)
    same(cosine.batch_query_offset_raw(10, scaled, offsets),
         w["vi"].batch_query_offset_raw(10, cosine._prepare(scaled), offsets))
    results = cosine.batch_query_offset(10, scaled, offsets)
    assert all(r.flags == 0 and len(r.rows) == 10 and (np.diff(r.distances) >= 0).all() for r in results)


def test_wide_index_and_view_are_refused(g):
    X = unit_rows(59, 1500, D)
    dm = g.DeviceMatrix.from_host(X)
    wide = g.Index.sorted(dm, g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(1024, 4, 1)), "l2")
    try:
        with pytest.raises(NotImplementedError, match="byte codes"):
            wide.batch_query_offset_raw(5, X[:2], np.zeros(1500, np.float32))
    finally:
        wide.vector_index.close()
        dm.close()
    w = world(g, 16)
    view = w["vi"].select(rows=np.arange(0, N, 2))
    try:
        with pytest.raises(NotImplementedError, match="view"):
            view.batch_query_offset_raw(5, w["Q"], np.zeros(view.length, np.float32))
    finally:
        view.close()


def test_host_checks(g):
    w = world(g, 16)
    vi, Q = w["vi"], w["Q"]
    offsets = np.zeros(N, np.float32)
    for bad in (np.nan, -np.inf):
        off = offsets.copy()
        off[77] = bad
        with pytest.raises(ValueError, match=r"row_offsets\[77\]"):
            vi.batch_query_offset_raw(10, Q, off)
    for k in (0, 64):
        with pytest.raises(NotImplementedError, match="k_nn"):
            vi.batch_query_offset_raw(k, Q, offsets)
    exclude = np.full(5, -1, np.int32)
    exclude[2] = N
    with pytest.raises(ValueError, match=r"exclude\[2\]"):
        vi.batch_query_offset_raw(10, Q, offsets, exclude)
    for frm, until in ((-1, N), (0, N + 1), (9, 8)):
        with pytest.raises(ValueError):
            vi.batch_query_offset_raw(10, Q, offsets, None, frm, until)
    empty = vi.batch_query_offset_raw(10, Q, offsets, None, 64, 64)
    assert empty[2].tolist() == [0] * 5 and padded(empty)
    assert vi.batch_query_offset_raw(10, np.zeros((0, D), np.float32), offsets)[0].shape == (0, 10)
