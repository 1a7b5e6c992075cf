"""Rank queries on the exact index (csrc/rank.hip, gulon_exact_index_query_rank): rank, row, key BITS and
total against ranks.rank_query_reference over the handle's own distances -- its ordinary query at k = the rows of its
range.  The gold lists are planted from the reference's full order (rank_ref.py): positions 0, 1, 62, 63, 64 and last, a
list of rows that cannot be ranked, an empty list, three rows whose best is not the first, and a pair of equal rows from
either side; the reference is asserted to show each case before the device is asked.

Shapes: 700 rows of 40 dimensions over [37, 695) with 37 queries -- ragged row steps, a second staging step of 8
dimensions, a query tile of 5; one query; 4 100 queries over 4 400 rows of 8 dimensions -- two passes, and row chunks of
3 groups; a batch with NaN, infinite and overflowing queries."""
import numpy as np
import pytest

import rank_ref
from cosmul_ref import exact_distances as numpy_distances
from cosmul_ref import unit_rows
from offset_ref import (distances_by_row, draw_offsets, huge_offsets, noisy_queries, nonfinite_queries, own_or_nan)

pytestmark = pytest.mark.gpu

TWINS = [(100 + i, 400 + i) for i in range(20)]


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


_WORLDS = {}


def world(g, n, d, frm, until, b):
    """The rows (twenty of them copies of others), the handle over [frm, until), b noisy copies of rows of the range --
    the odd ones exclude the row they were made from -- and the distances [b][until - frm] by the handle itself."""
    key = (n, d, frm, until, b)
    if key not in _WORLDS:
        X = unit_rows(n + d, n, d)
        for a, c in TWINS:
            X[c] = X[a]
        Q, exclude = noisy_queries(b + d, X, b, frm, until)
        dm = g.DeviceMatrix.from_host(X)
        ix = g.ExactIndex(dm, "l2", frm, until)
        ids = np.arange(frm, until)
        dist = distances_by_row(ix.batch_query_raw(until - frm, Q), ids)
        offsets = draw_offsets(n + b, n, TWINS)
        twin = rank_ref.pick_twins(TWINS, exclude)
        offsets[list(twin)] = 0.25
        _WORLDS[key] = {"ix": ix, "dm": dm, "X": X, "Q": Q, "exclude": exclude, "dist": dist, "ids": ids,
                        "offsets": offsets, "twin": twin, "outside": 0 if frm > 0 else None}
    return _WORLDS[key]


def planted(g, w):
    """kind -> (gold lists, the reference's answer), each asserted to show its case."""
    if "planted" not in w:
        order = rank_ref.full_order(g, w, w["offsets"])
        w["planted"] = {}
        for kind in rank_ref.KINDS:
            gold = rank_ref.plant(kind, order, w, w["offsets"], w["twin"], w["outside"])
            want = rank_ref.reference(g, w, w["offsets"], gold)
            assert rank_ref.shows(kind, want, order, w["twin"]), kind
            w["planted"][kind] = (gold, want)
    return w["planted"]


@pytest.mark.parametrize("b", (37, 1))
def test_every_planted_case_matches_the_reference(g, b):
    w = world(g, 700, 40, 37, 695, b)
    lists = w["ix"].batch_query_offset_raw(63, w["Q"], w["offsets"], w["exclude"])[0]
    checked = 0
    for kind, (gold, want) in planted(g, w).items():
        got = w["ix"].batch_query_rank_raw(w["Q"], gold, w["offsets"], w["exclude"])
        rank_ref.same(got, want)
        checked += rank_ref.agrees_with_the_offset_query(got, lists)
    assert checked >= 4 * b                                      # positions 0, 1, 62 and the three at the least


def test_no_offsets_and_no_excluded_rows(g):
    w = world(g, 700, 40, 37, 695, 37)
    plain = dict(w, exclude=np.full(37, -1, np.int32))
    zeros = np.zeros(700, np.float32)
    order = rank_ref.full_order(g, plain, zeros)
    gold = [[o[63], o[3]] for o in order]
    want = rank_ref.reference(g, plain, zeros, gold)
    assert (want[0] == 3).all() and (want[3] == 658).all()
    rank_ref.same(w["ix"].batch_query_rank_raw(w["Q"], gold), want)
    rank_ref.same(w["ix"].batch_query_rank_raw(w["Q"], gold, zeros, plain["exclude"]), want)
    dev = g.DeviceOffsets.from_host(w["offsets"])                # downloaded: the entry point takes host pointers
    try:
        gold, want = planted(g, w)["three"]
        rank_ref.same(w["ix"].batch_query_rank_raw(w["Q"], gold, dev, w["exclude"]), want)
    finally:
        dev.free()


def test_two_passes_and_chunks_of_three_row_groups(g):
    """4 096 queries are one pass: 4 100 take two, the second with its own gold lists and excluded rows.  256 query tiles
    leave 8 workgroups per tile: 18 row groups go into 6 chunks of 3."""
    n, b, base = 4400, 4100, 37
    groups = -(-n // 256)
    want_chunks = -(-2048 // (4096 // 16))
    per_chunk = -(-groups // min(want_chunks, groups))
    assert (groups, per_chunk, -(-groups // per_chunk)) == (18, 3, 6)            # knn_row_chunks, restated
    w = world(g, n, 8, 0, n, base)
    cases = planted(g, w)
    pick, kind_of = np.arange(b) % base, (np.arange(b) // base) % len(rank_ref.KINDS)
    gold = [cases[rank_ref.KINDS[kind_of[i]]][0][pick[i]] for i in range(b)]
    want = tuple(np.array([cases[rank_ref.KINDS[kind_of[i]]][1][part][pick[i]] for i in range(b)]) for part in range(4))
    got = w["ix"].batch_query_rank_raw(w["Q"][pick], gold, w["offsets"], w["exclude"][pick])
    rank_ref.same(got, want)
    lists = w["ix"].batch_query_offset_raw(63, w["Q"], w["offsets"], w["exclude"])[0]
    assert rank_ref.agrees_with_the_offset_query(got, lists[pick]) >= 4 * (b // len(rank_ref.KINDS))


def test_non_finite_queries(g):
    """The first query tile holds a NaN query, a +inf query, one whose distances overflow and one whose keys overflow at
    the offsets of 3e38: the first three have no candidate at all, the fourth only the rows with small offsets."""
    n, d, frm, until, b = 700, 33, 37, 695, 17
    w = world(g, n, d, frm, until, b)
    at = (3, 5, 7, 9)
    Q = nonfinite_queries(w["Q"], at)
    dist = own_or_nan(w["ix"].batch_query_raw(until - frm, Q), w["ids"], numpy_distances(w["X"][frm:until], Q))
    keepers = np.arange(frm + 3, until, 16)
    offsets = huge_offsets(800, n, keepers)
    nf = dict(w, dist=dist)
    order = rank_ref.full_order(g, nf, offsets)
    assert [len(order[q]) for q in at[:3]] == [0, 0, 0] and 0 < len(order[at[3]]) <= len(keepers)
    gold = [[int(o[len(o) // 2]), int(keepers[0])] if len(o) else [int(keepers[1]), int(keepers[2])] for o in order]
    want = rank_ref.reference(g, nf, offsets, gold)
    assert (want[0][list(at[:3])] == -1).all() and (want[3][list(at[:3])] == 0).all()
    assert (np.delete(want[0], at[:3]) >= 0).all()
    rank_ref.same(w["ix"].batch_query_rank_raw(Q, gold, offsets, w["exclude"]), want)


def test_a_used_handle_answers_the_same(g):
    w = world(g, 700, 40, 37, 695, 37)
    gold, want = planted(g, w)["at64"]
    first = w["ix"].batch_query_rank_raw(w["Q"], gold, w["offsets"], w["exclude"])
    w["ix"].batch_query_raw(5, w["Q"])
    w["ix"].batch_query_offset_raw(10, w["Q"][:3], w["offsets"])
    rank_ref.same(w["ix"].batch_query_rank_raw(w["Q"], gold, w["offsets"], w["exclude"]), first)
    rank_ref.same(first, want)


def test_host_checks(g):
    w = world(g, 700, 40, 37, 695, 37)
    ix, Q, b = w["ix"], w["Q"], 37
    gold = [[100]] * b
    off = np.zeros(700, np.float32)
    off[123] = np.nan
    with pytest.raises(ValueError, match=r"row_offsets\[123\]"):
        ix.batch_query_rank_raw(Q, gold, off)
    for bad in (700, -1):
        lists = [[100]] * 5 + [[200, bad]] + [[100]] * (b - 6)
        with pytest.raises(ValueError, match=r"gold_rows\[6\] = %d" % bad):
            ix.batch_query_rank_raw(Q, lists)
    exclude = np.full(b, -1, np.int32)
    exclude[3] = 700
    with pytest.raises(ValueError, match=r"exclude\[3\]"):
        ix.batch_query_rank_raw(Q, gold, None, exclude)
    with pytest.raises(ValueError):
        ix.batch_query_rank_raw(Q, gold[:-1])
    with pytest.raises(ValueError):
        ix.batch_query_rank_raw(Q, gold, np.zeros(699, np.float32))
    N, L = g.native, g.native.lib()
    out_i, out_f = np.zeros(b, np.int32), np.zeros(b, np.float32)
    goff = np.arange(b + 1, dtype=np.int32)
    goff[9] = 7                                                  # descends after entry 8
    with pytest.raises(ValueError, match=r"gold_offsets\[9\] = 7 < gold_offsets\[8\] = 8"):
        N.check(L.gulon_exact_index_query_rank(ix._h, Q.reshape(-1), b, None, None, goff, np.full(b, 100, np.int32),
                                               out_i, out_i.copy(), out_f, None))
    goff = np.arange(1, b + 2, dtype=np.int32)
    with pytest.raises(ValueError, match=r"gold_offsets\[0\] = 1"):
        N.check(L.gulon_exact_index_query_rank(ix._h, Q.reshape(-1), b, None, None, goff, np.full(b + 1, 100, np.int32),
                                               out_i, out_i.copy(), out_f, None))
    empty = ix.batch_query_rank_raw(np.zeros((0, 40), np.float32), [])
    assert [len(a) for a in empty] == [0, 0, 0, 0]
