"""Offset queries on the exact index (csrc/offset.hip, gulon_exact_index_query_offset): rows and key BITS
against csls.offset_query_reference over the handle's own distances -- its ordinary query at k = the rows of its range.

Shapes: 700 rows are three 256-row groups (several row chunks are merged), 33 dimensions cross the 32-wide staging step
by one, the handle covers [37, 695), 17 queries leave one in the second query tile.  Offsets come from eight values and
twenty rows are copies of others with the same offset, so equal keys occur and the row id decides; a tenth of the
offsets are +inf; every other query excludes the row it was made from.  Negative keys, tie groups larger than a list
and non-finite queries: test_gpu_offset_paths.py."""
import numpy as np
import pytest

from offset_ref import distances_by_row, draw_offsets, padded, run_dev, same

pytestmark = pytest.mark.gpu

N, D, FROM, UNTIL, B = 700, 33, 37, 695, 17
TWINS = [(100 + i, 400 + i) for i in range(20)]
DEPTHS = (1, 10, 63)


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


@pytest.fixture(scope="module")
def world(g):
    """The rows, the handle over [37, 695), the queries (noisy copies of rows of the range), the excluded rows and the
    distances [B][658] by the handle's ordinary query."""
    rng = np.random.default_rng(7)
    X = rng.standard_normal((N, D)).astype(np.float32) * np.float32(0.3)
    for a, b in TWINS:
        X[b] = X[a]
    made_from = rng.integers(FROM, UNTIL, B)
    made_from[1] = 100                                           # a twin, not excluded: its copy ties with it
    Q = (X[made_from] + rng.standard_normal((B, D)).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    exclude = np.where(np.arange(B) % 2 == 0, made_from, -1).astype(np.int32)
    dm = g.DeviceMatrix.from_host(X)
    ix = g.ExactIndex(dm, "l2", FROM, UNTIL)
    ids = np.arange(FROM, UNTIL)
    dist = distances_by_row(ix.batch_query_raw(UNTIL - FROM, Q), ids)
    yield {"ix": ix, "Q": Q, "exclude": exclude, "dist": dist, "ids": ids}
    ix.close()
    dm.close()


def reference(g, w, offsets, k, exclude):
    return g.offset_query_reference(w["dist"], offsets[FROM:UNTIL], k, exclude, rows=w["ids"])


@pytest.mark.parametrize("k", DEPTHS)
def test_host_form_matches_the_reference(g, world, k):
    offsets = draw_offsets(11, N, TWINS)
    offsets[[100, 400]] = 0.25                                   # the twins next to query 1 are candidates
    got = world["ix"].batch_query_offset_raw(k, world["Q"], offsets, world["exclude"])
    same(got, reference(g, world, offsets, k, world["exclude"]))
    assert padded(got)
    if k > 1:                                                    # equal keys did occur, and the smaller row came first
        ties = [(got[0][q, e], got[0][q, e + 1]) for q in range(B) for e in range(got[2][q] - 1)
                if got[1][q, e] == got[1][q, e + 1]]
        assert ties and all(a < b for a, b in ties)
    for q in range(B):                                           # no masked and no excluded row
        live = got[0][q, :got[2][q]]
        assert np.isfinite(offsets[live]).all() and world["exclude"][q] not in live.tolist()
        assert live.min() >= FROM and live.max() < UNTIL


@pytest.mark.parametrize("k", DEPTHS)
def test_dev_form_matches_the_reference(g, world, k):
    offsets = draw_offsets(13, N, TWINS)
    ix = world["ix"]
    L = g.native.lib()

    def call(d_q, b, kk, d_off, d_ex, d_oi, d_ok, d_oc):
        return L.gulon_exact_index_query_offset_dev(ix._h, d_q, b, kk, d_off, d_ex, d_oi, d_ok, d_oc, None)
    same(run_dev(g, call, world["Q"], k, offsets, world["exclude"]), reference(g, world, offsets, k, world["exclude"]))
    same(run_dev(g, call, world["Q"], k, offsets, None), reference(g, world, offsets, k, None))


def test_device_offsets_and_results(g, world):
    offsets = draw_offsets(17, N, TWINS)
    want = reference(g, world, offsets, 10, None)
    dev = g.DeviceOffsets.from_host(offsets)
    try:
        assert np.array_equal(dev.numpy().view(np.uint32), offsets.view(np.uint32))
        same(world["ix"].batch_query_offset_raw(10, world["Q"], dev), want)
        with pytest.raises(ValueError):
            world["ix"].batch_query_offset_raw(10, world["Q"], g.DeviceOffsets.from_host(offsets[:-1]))
    finally:
        dev.free()
    results = world["ix"].batch_query_offset(10, world["Q"], offsets)
    assert [r.rows.tolist() for r in results] == [want[0][q, :want[2][q]].tolist() for q in range(B)]
    assert all(r.flags == 0 and (np.diff(r.distances) >= 0).all() for r in results)


@pytest.mark.parametrize("k", (10, 63))
def test_fewer_candidates_than_k(g, world, k):
    offsets = draw_offsets(19, N, keep=(40, 300, 301, 555, 694))
    offsets[[5, 699]] = 0.0                                      # finite, but outside the handle's range
    got = world["ix"].batch_query_offset_raw(k, world["Q"], offsets)
    same(got, reference(g, world, offsets, k, None))
    assert got[2].tolist() == [5] * B and padded(got)
    exclude = np.full(B, 300, np.int32)
    got = world["ix"].batch_query_offset_raw(k, world["Q"], offsets, exclude)
    same(got, reference(g, world, offsets, k, exclude))
    assert got[2].tolist() == [4] * B
    none = world["ix"].batch_query_offset_raw(k, world["Q"], np.full(N, np.inf, np.float32))
    assert none[2].tolist() == [0] * B and padded(none)


def test_a_used_handle_answers_the_same(g, world):
    offsets = draw_offsets(23, N, TWINS)
    ix = world["ix"]
    first = ix.batch_query_offset_raw(10, world["Q"], offsets, world["exclude"])
    ix.batch_query_raw(5, world["Q"])
    ix.batch_query_raw(100, world["Q"][:3])
    same(ix.batch_query_offset_raw(10, world["Q"], offsets, world["exclude"]), first)
    same(first, reference(g, world, offsets, 10, world["exclude"]))


def test_more_queries_than_one_pass_holds(g, world):
    """4 096 queries are one pass of the scan: 4 100 take two, the second with its own excluded rows."""
    offsets = draw_offsets(29, N, TWINS)
    reps = -(-4100 // B)
    Q = np.tile(world["Q"], (reps, 1))[:4100]
    exclude = np.tile(world["exclude"], reps)[:4100]
    want = reference(g, world, offsets, 10, world["exclude"])
    got = world["ix"].batch_query_offset_raw(10, Q, offsets, exclude)
    pick = np.arange(4100) % B
    same(got, tuple(a[pick] for a in want))


def test_host_checks(g, world):
    ix, Q = world["ix"], world["Q"]
    offsets = np.zeros(N, np.float32)
    for bad in (np.nan, -np.inf):
        off = offsets.copy()
        off[123] = bad
        with pytest.raises(ValueError, match=r"row_offsets\[123\]"):
            ix.batch_query_offset_raw(10, Q, off)
    for k in (0, 64):
        with pytest.raises(NotImplementedError, match="k_nn"):
            ix.batch_query_offset_raw(k, Q, offsets)
    for bad in (N, -2):
        exclude = np.full(B, -1, np.int32)
        exclude[3] = bad
        with pytest.raises(ValueError, match=r"exclude\[3\]"):
            ix.batch_query_offset_raw(10, Q, offsets, exclude)
    with pytest.raises(ValueError):
        ix.batch_query_offset_raw(10, Q, offsets[:-1])
    with pytest.raises(ValueError):
        ix.batch_query_offset_raw(10, Q, offsets, np.full(B - 1, -1, np.int32))
    assert ix.batch_query_offset_raw(10, np.zeros((0, D), np.float32), offsets)[0].shape == (0, 10)
    L = g.native.lib()
    assert L.gulon_exact_index_query_offset_dev(None, None, 0, 1, None, None, None, None, None, None) \
        == g.native.ERR_INVALID_ARGUMENT
