"""Offset queries on the grouped index (csrc/grouped_offset.hip), bit for bit -- ids, keys and counts --
against csls.offset_query_reference over the handle's own distances (grouped_offset_ref.py).  Every case asserts from
the reference's side that what it is meant to exercise occurs."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits
from grouped_offset_ref import build, group_of_rows, queries_from, reference, scattered_distances
from offset_ref import SIGNED_LEVELS, draw_offsets, huge_offsets, padded, plant_nearest, same

pytestmark = pytest.mark.gpu

PASS = 1024                                  # GROUPED_OFFSET_SUB_BATCH (grouped_offset.hpp)

# name -> (n, d, groups, m, k, twins, row0_outside, depth of the ordinary query behind the reference)
SHAPES = {
    "two-words-padded": (1900, 24, 10, 6, 64, 20, False, None),     # VEC 4, two code words, two padding quantizers
    "one-word-16": (2000, 32, 3, 16, 256, 0, False, None),          # VEC 16; groups of ~660 rows: the ring wraps
    # two 16-byte words, the largest LDS form: the tables leave room for 928 heap entries, not for n
    "two-words-16": (2000, 64, 12, 32, 256, 0, False, 920),
    "many-groups": (2000, 16, 300, 4, 16, 0, False, None),          # gq_select_groups; groups under 64 rows
    "leading-empty": (1500, 12, 9, 4, 16, 0, True, None),           # the reference's leading empty group
}
CASES = [("two-words-padded", "groups", 3), ("two-words-padded", "groups", 10), ("two-words-padded", "vectors", 500),
         ("two-words-padded", "vectors", 1), ("one-word-16", "groups", 2), ("two-words-16", "groups", 4),
         ("many-groups", "groups", 70), ("leading-empty", "groups", 2), ("leading-empty", "vectors", 400)]


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


_worlds, _indexes, _dists = {}, {}, {}


def world(g, shape):
    if shape not in _worlds:
        n, d, groups, m, k, twins, row0, depth = SHAPES[shape]
        _worlds[shape] = dict(build(g, n, d, groups, m, k, seed=n + d + m, twins=twins, row0_outside=row0), depth=depth,
                              m=m, k=k)
    return _worlds[shape]


def index_of(g, shape, strategy, limit, metric="l2"):
    key = (shape, strategy, limit, metric)
    if key not in _indexes:
        w = world(g, shape)
        strat = g.LimitGroups(limit) if strategy == "groups" else g.LimitVectors(limit)
        _indexes[key] = g.Index.grouped(w["gv"], w["pq"], strat, metric)
    return _indexes[key]


def asked(g, oracle, shape, strategy, limit, b):
    """-> (index, Q, exclude, dist [b][n]): b queries, the first made from a pair of twins where the shape has them, and
    the handle's own distances, +inf at the rows of the groups a query does not search."""
    key = (shape, strategy, limit, b)
    w = world(g, shape)
    index = index_of(g, shape, strategy, limit)
    if key not in _dists:
        Q, ex = queries_from(7 * b + limit, w["Xg"], b, first=[a for a, _ in w["twins"][:3]])
        _dists[key] = (Q, ex, scattered_distances(index, Q, w["depth"], oracle))
    return (index,) + _dists[key]


def test_shapes_are_what_they_are_meant_to_be(g):
    """Group borders inside 64-row blocks, groups under 64 rows, empty groups, long groups, the leading empty group."""
    w = world(g, "two-words-padded")
    assert len(w["pq"].quantizers) == 6 and (w["gv"].offsets % 64 != 0).any() and len(w["twins"]) == 20
    assert all(group_of_rows(w["gv"], w["n"])[a] == group_of_rows(w["gv"], w["n"])[b] for a, b in w["twins"])
    sizes = np.diff(np.r_[0, world(g, "one-word-16")["gv"].offsets, 2000])
    assert sizes.max() > 4 * 64 + 64                     # more than four code blocks: the prefetch ring wraps
    sizes = np.diff(np.r_[0, world(g, "many-groups")["gv"].offsets, 2000])
    assert (sizes < 64).sum() > 100 and len(sizes) >= 4 * 70
    assert world(g, "leading-empty")["gv"].offsets[0] == 0


def test_distances_are_the_oracles(g, oracle):
    """The scattered distances of one shape against the CPU oracle's GroupedIndex.query at K = n."""
    shape, strategy, limit = "two-words-padded", "groups", 3
    w = world(g, shape)
    index, Q, ex, dist = asked(g, oracle, shape, strategy, limit, 5)
    n = w["n"]
    ei, ed, ec = oracle.grouped_query(index.data.indices(), w["d"], w["k"], w["pq"].flat_centroids(), w["gv"].centroids,
                                      w["gv"].offsets, Q, n, 0, limit)
    want = np.full((len(Q), n), np.inf, np.float32)
    for q in range(len(Q)):
        want[q, ei[q, :ec[q]]] = ed[q, :ec[q]]
    assert np.array_equal(bits(dist), bits(want)) and np.isposinf(dist).any() and np.isfinite(dist).any()


@pytest.mark.parametrize("k", (1, 10, 63))
@pytest.mark.parametrize("b", (1, 5, 17))
@pytest.mark.parametrize("shape,strategy,limit", CASES)
def test_offset_query_equals_reference(g, oracle, shape, strategy, limit, b, k):
    w = world(g, shape)
    index, Q, ex, dist = asked(g, oracle, shape, strategy, limit, b)
    n = w["n"]
    searched = np.isfinite(dist)
    per_query = np.array([len(np.unique(group_of_rows(w["gv"], n)[searched[q]])) for q in range(b)])
    group = group_of_rows(w["gv"], n)
    if (shape, strategy) == ("two-words-padded", "groups"):
        most = min(limit, len(np.unique(group)))         # (a leading empty group may be one of the searched)
        assert (per_query <= most).all() and (per_query >= most - int(w["gv"].offsets[0] == 0)).all()
    if strategy == "vectors" and limit == 1:
        assert per_query.max() == 1                      # fewer live slots than a workgroup has waves
    if shape == "many-groups":
        assert 63 < per_query.max() <= 70                # 70 lists per query, some of them of empty groups
    unsearched = np.flatnonzero(~searched[0])
    if len(unsearched):                                  # excluding a row of an unsearched group changes nothing
        ex = ex.copy()
        ex[0] = unsearched[len(unsearched) // 2]

    # the eight levels with a tenth +inf; the twins share one offset each
    offsets = draw_offsets(n + k, n, twins=w["twins"])
    for a, c in w["twins"][:3]:
        offsets[a] = offsets[c] = np.float32(0.3)
    want = reference(g, dist, offsets, k, ex)
    if w["twins"] and k >= 10:                           # equal keys inside a group, inside the answer
        assert (want[1][0, :-1] == want[1][0, 1:]).any()
    got = index.batch_query_offset_raw(k, Q, offsets, ex)
    same(got, want)
    assert padded(got)
    if b > 1:
        assert ex[1] >= 0 and ex[1] not in got[0][1]
    if len(unsearched):
        same(index.batch_query_offset_raw(k, Q[:1], offsets, None), tuple(a[:1] for a in want))

    # signed levels: negative keys, and the step to positive ones inside the first k
    signed = plant_nearest(draw_offsets(n + 2 * k, n, levels=SIGNED_LEVELS), dist, np.arange(n), ex, -1.5)
    want = reference(g, dist, signed, k, ex)
    negative = want[1][:, 0] < 0                         # (a query that excludes its own row may start above zero)
    assert negative.any()
    if k >= 10:
        assert (want[1][negative & (want[2] == k), -1] > 0).any()
    same(index.batch_query_offset_raw(k, Q, signed, ex), want)

    # every finite distance + 3e38 rounds to one key: ties run across groups and the row id decides across the lists
    huge = huge_offsets(n + 3 * k, n, np.arange(5, n, 97))
    want = reference(g, dist, huge, k, ex)
    if k == 63 and per_query.min() > 1:
        q = int(np.argmax(per_query))
        assert want[2][q] == k and want[1][q, -1] == want[1][q, -2]
        with np.errstate(over="ignore"):
            tied = np.flatnonzero(((dist[q] + huge).astype(np.float32) == want[1][q, -1]) & (np.arange(n) != ex[q]))
        assert len(np.unique(group[tied])) > 1           # the tie spans groups, so the lists of several slots hold it
        if shape == "many-groups":                       # and here, with groups under 64 rows, so does the answer
            assert len(np.unique(group[want[0][q][want[1][q] == want[1][q, -1]]])) > 1
    same(index.batch_query_offset_raw(k, Q, huge, ex), want)

    # all but five rows of the first query's searched groups +inf: count 5 at the most, and padding
    live = np.flatnonzero(searched[0])
    keep = live[:: max(1, len(live) // 5)][:5]
    few = draw_offsets(n + 4 * k, n, keep=keep)
    want = reference(g, dist, few, k, None)
    assert want[2][0] == min(k, 5) and (want[2] <= 5).all()
    got = index.batch_query_offset_raw(k, Q, few, None)
    same(got, want)
    assert padded(got)

    # all rows of one searched group +inf
    masked = draw_offsets(n + 5 * k, n, inf_share=0.0)
    masked[group == group[live[0]]] = np.inf
    want = reference(g, dist, masked, k, ex)
    assert not np.isin(want[0][0], np.flatnonzero(group == group[live[0]])).any()
    same(index.batch_query_offset_raw(k, Q, masked, ex), want)


def test_nan_and_inf_queries_beside_ordinary_ones(g, oracle):
    """Five queries of LimitGroups(3): slots 0 .. 3 of the first workgroup belong to queries 0 and 1."""
    shape, strategy, limit, k = "two-words-padded", "groups", 3, 10
    w = world(g, shape)
    index, Q, ex, dist = asked(g, oracle, shape, strategy, limit, 5)
    bad = Q.copy()
    bad[1, 2] = np.nan
    bad[3, 0] = np.inf
    offsets = draw_offsets(11, w["n"])
    want = reference(g, dist, offsets, k, ex)
    got = index.batch_query_offset_raw(k, bad, offsets, ex)
    assert got[2][1] == 0 and got[2][3] == 0 and padded(got) and (want[2][[0, 2, 4]] == k).all()
    same(tuple(a[[0, 2, 4]] for a in got), tuple(a[[0, 2, 4]] for a in want))


def test_cosine_index_normalises_the_queries(g):
    shape, k = "two-words-padded", 10
    w = world(g, shape)
    index = index_of(g, shape, "groups", 3, "cosine")
    Q, ex = queries_from(3, w["Xg"], 5)
    Q = Q * np.float32(7.5)
    dist = scattered_distances(index, Q)
    plain = scattered_distances(index_of(g, shape, "groups", 3), Q)
    assert not np.array_equal(bits(dist), bits(plain))          # the normalisation matters
    offsets = draw_offsets(12, w["n"])
    same(index.batch_query_offset_raw(k, Q, offsets, ex), reference(g, dist, offsets, k, ex))
    results = index.batch_query_offset(k, Q, offsets, ex)
    assert [len(r.rows) for r in results] == [k] * 5 and results[0].flags == 0


def test_a_batch_of_one_pass_and_four(g):
    shape, k = "many-groups", 10
    w = world(g, shape)
    index = index_of(g, shape, "groups", 70)
    Q, ex = queries_from(5, w["Xg"], PASS + 4)
    dist = scattered_distances(index, Q)
    offsets = draw_offsets(13, w["n"])
    want = reference(g, dist, offsets, k, ex)
    assert (want[2] == k).all()
    same(index.batch_query_offset_raw(k, Q, offsets, ex), want)


@pytest.mark.parametrize("literal", (False, True))
def test_a_used_handle_answers_the_ordinary_query_as_before(g, monkeypatch, literal):
    if literal:
        monkeypatch.setenv("GULON_GROUPED_LITERAL", "1")
    shape = "many-groups"
    w = world(g, shape)
    strat = g.LimitGroups(70)
    fresh, used = (g.Index.grouped(w["gv"], w["pq"], strat) for _ in range(2))
    try:
        Q, ex = queries_from(9, w["Xg"], 17)
        before = used.batch_query_raw(10, Q)
        for k in (63, 1):
            used.batch_query_offset_raw(k, Q, draw_offsets(k, w["n"]), ex)
        after, other = used.batch_query_raw(10, Q), fresh.batch_query_raw(10, Q)
        for a, b in ((before, after), (before, other)):
            assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
    finally:
        fresh.close()
        used.close()


def test_host_checks(g):
    shape = "two-words-padded"
    w = world(g, shape)
    n = w["n"]
    index = index_of(g, shape, "groups", 3)
    Q, ex = queries_from(1, w["Xg"], 5)
    offsets = draw_offsets(14, n)
    for value in (np.nan, -np.inf):
        bad = offsets.copy()
        bad[n - 1] = value
        with pytest.raises(ValueError):
            index.batch_query_offset_raw(5, Q, bad)
    for row in (n, -2):
        bad = ex.copy()
        bad[2] = row
        with pytest.raises(ValueError):
            index.batch_query_offset_raw(5, Q, offsets, bad)
    for k in (0, 64):
        with pytest.raises(NotImplementedError):
            index.batch_query_offset_raw(k, Q, offsets)
    with pytest.raises(ValueError):
        index.batch_query_offset_raw(5, Q, offsets[:-1])
    with pytest.raises(ValueError):
        index.batch_query_offset_raw(5, Q, offsets, ex[:-1])
    dev = g.DeviceOffsets.from_host(offsets[:-1])
    try:
        with pytest.raises(ValueError):
            index.batch_query_offset_raw(5, Q, dev)
    finally:
        dev.free()
    dev = g.DeviceOffsets.from_host(offsets)
    try:
        same(index.batch_query_offset_raw(5, Q, dev, ex), index.batch_query_offset_raw(5, Q, offsets, ex))
    finally:
        dev.free()
    got = index.batch_query_offset_raw(5, Q[:0], offsets)
    assert got[0].shape == (0, 5) and got[2].shape == (0,)


def test_wide_codes_are_refused(g):
    w = build(g, 1200, 8, 4, 2, 512, seed=3, iters=1)
    index = g.Index.grouped(w["gv"], w["pq"], g.LimitGroups(2))
    try:
        with pytest.raises(NotImplementedError, match="byte codes"):
            index.batch_query_offset_raw(5, w["Xg"][:3], np.zeros(1200, np.float32))
    finally:
        index.close()


@pytest.mark.parametrize("strategy,limit", [(0, 1), (1, 10)])
def test_index_without_rows_answers_nothing(g, strategy, limit):
    from gulon_amd import native as N
    d, m, k, B, K = 8, 4, 16, 3, 5
    h = C.c_void_p()
    cents = np.random.default_rng(0).standard_normal(k * d).astype(np.float32)
    assert N.lib().gulon_grouped_index_create(np.zeros(1, np.uint8), 0, d, m, k, cents, np.zeros(d, np.float32),
                                              np.zeros(1, np.int32), 1, C.byref(h)) == 0
    Q = np.random.default_rng(1).standard_normal(B * d).astype(np.float32)
    oi, ok, oc = np.zeros(B * K, np.int32), np.zeros(B * K, np.float32), np.full(B, -1, np.int32)
    assert N.lib().gulon_grouped_index_query_offset(h, Q, B, K, strategy, limit, np.zeros(1, np.float32), None, oi, ok,
                                                    oc) == 0
    assert oc.tolist() == [0] * B and (oi == -1).all() and np.isposinf(ok).all()
    assert N.lib().gulon_grouped_index_destroy(h) == 0
