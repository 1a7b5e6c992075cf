"""Rank queries on the flat byte-code index (csrc/rank.hip, gulon_index_query_rank): rank, row, key BITS
and total against ranks.rank_query_reference over the handle's own distances -- its ordinary query at k = the rows of the
range.  The gold lists are planted from the reference's full order (rank_ref.py) and the reference is asserted to show
each case before the device is asked.

Shapes: 4 300 rows, the range [70, n - 33) -- neither end on a 64-row code block, 66 blocks in two row chunks; 256
centroids at (m, d) = (16, 32), (25, 50) and (64, 64): one 16-byte code word, seven 4-byte words and four 16-byte words,
with eight, four and two query slots to a workgroup; batches of 19 (a last workgroup with idle slots) and 1 (one slot).
Twenty rows are copies of others with the same offset; a tenth of the offsets are +inf; every other query excludes the row
it was made from.  The launcher's second pass has a case of its own: 4 100 queries at m = 64 on 327 rows."""
import numpy as np
import pytest

import rank_ref
from cosmul_ref import unit_rows
from offset_ref import distances_by_row, draw_offsets, flat_chunks, flat_slots, noisy_queries

pytestmark = pytest.mark.gpu

N, FROM, K, ITERS = 4300, 70, 256, 1
UNTIL = N - 33
DIMENSIONS = {16: 32, 25: 50, 64: 64}
SLOTS = {16: 8, 25: 4, 64: 2}
TWINS = [(200 + i, 3000 + i) for i in range(20)]


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


_INDEXES, _WORLDS = {}, {}


def index(g, m):
    if m not in _INDEXES:
        X = unit_rows(5 * m + N, N, DIMENSIONS[m])
        for a, c in TWINS:
            X[c] = X[a]
        dm = g.DeviceMatrix.from_host(X)
        pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(K, m, ITERS))
        _INDEXES[m] = (X, g.Index.sorted(dm, pq, "l2").vector_index)
    return _INDEXES[m]


def world(g, m, b):
    """A trained PQIndex over N unit rows, b noisy copies of rows of [70, N - 33) -- the odd ones exclude the row they
    were made from -- and the distances [b][N - 103] of the handle's ordinary query over that range."""
    if (m, b) not in _WORLDS:
        X, vi = index(g, m)
        Q, exclude = noisy_queries(m + b, X, b, FROM, UNTIL)
        ids = np.arange(FROM, UNTIL)
        dist = distances_by_row(vi.batch_query_raw(len(ids), Q, FROM, UNTIL), ids)
        offsets = draw_offsets(m + 7 * b, N, TWINS)
        twin = rank_ref.pick_twins(TWINS, exclude)
        offsets[list(twin)] = 0.25
        offsets[[3, N - 5]] = 0.0                                # finite, but outside the range
        _WORLDS[(m, b)] = {"vi": vi, "Q": Q, "exclude": exclude, "dist": dist, "ids": ids, "offsets": offsets,
                           "twin": twin, "outside": N - 5}
    return _WORLDS[(m, b)]


def ask(w, gold, offsets="own", exclude="own"):
    return w["vi"].batch_query_rank_raw(w["Q"], gold, w["offsets"] if isinstance(offsets, str) else offsets,
                                        w["exclude"] if isinstance(exclude, str) else exclude, FROM, UNTIL)


@pytest.mark.parametrize("b", (19, 1))
@pytest.mark.parametrize("m", (16, 25, 64))
def test_every_planted_case_matches_the_reference(g, m, b):
    assert flat_slots(m, 19)[3] == SLOTS[m] and flat_slots(m, b)[4] == (SLOTS[m] if b == 19 else 1)
    assert flat_chunks(FROM, UNTIL, b, m)[1] >= 2
    w = world(g, m, b)
    order = rank_ref.full_order(g, w, w["offsets"])
    lists = w["vi"].batch_query_offset_raw(63, w["Q"], w["offsets"], w["exclude"], FROM, UNTIL)[0]
    checked = 0
    for kind in rank_ref.KINDS:
        gold = rank_ref.plant(kind, order, w, w["offsets"], w["twin"], w["outside"])
        want = rank_ref.reference(g, w, w["offsets"], gold)
        assert rank_ref.shows(kind, want, order, w["twin"]), kind
        got = ask(w, gold)
        rank_ref.same(got, want)
        checked += rank_ref.agrees_with_the_offset_query(got, lists)
    assert checked >= 4 * b                                      # positions 0, 1, 62 and the three at the least


def test_no_offsets_no_excluded_rows_and_the_sorted_index_prepares(g):
    w = world(g, 16, 19)
    plain = dict(w, exclude=np.full(19, -1, np.int32))
    zeros = np.zeros(N, np.float32)
    order = rank_ref.full_order(g, plain, zeros)
    gold = [[o[63], o[3]] for o in order]
    want = rank_ref.reference(g, plain, zeros, gold)
    assert (want[0] == 3).all() and (want[3] == UNTIL - FROM).all()
    rank_ref.same(ask(w, gold, None, None), want)
    rank_ref.same(ask(w, gold, zeros, plain["exclude"]), want)
    # over all rows, through a cosine SortedIndex: the queries are normalised first, as its offset query normalises them
    cosine = g.SortedIndex(w["vi"], "cosine")
    scaled = w["Q"] * np.float32(3)
    lists, keys, _ = cosine.batch_query_offset_raw(63, scaled, w["offsets"])
    gold = [[int(lists[q, 50]), int(lists[q, 9])] for q in range(19)]
    rank, row, key, total = cosine.batch_query_rank_raw(scaled, gold, w["offsets"])
    assert (rank == 9).all() and np.array_equal(row, lists[:, 9]) and np.array_equal(key.view(np.uint32),
                                                                                     keys[:, 9].view(np.uint32))
    assert (total == np.isfinite(w["offsets"]).sum()).all()
    dev = g.DeviceOffsets.from_host(w["offsets"])                # downloaded: the entry point takes host pointers
    try:
        rank_ref.same(cosine.batch_query_rank_raw(scaled, gold, dev), (rank, row, key, total))
    finally:
        dev.free()


def test_a_used_handle_answers_the_same(g):
    w = world(g, 25, 19)
    order = rank_ref.full_order(g, w, w["offsets"])
    gold = rank_ref.plant("at64", order, w, w["offsets"], w["twin"], w["outside"])
    first = ask(w, gold)
    w["vi"].batch_query_raw(5, w["Q"])
    w["vi"].batch_query_offset_raw(10, w["Q"][:3], w["offsets"])
    rank_ref.same(ask(w, gold), first)
    rank_ref.same(first, rank_ref.reference(g, w, w["offsets"], gold))


def test_more_queries_than_one_pass_holds(g):
    """The rank twin of test_gpu_offset_paths.test_flat_more_queries_than_one_pass_holds, on its index: 327 rows, the
    range [5, n - 3), m = 64 -- 256 MiB of tables are 4 096 queries, so 4 100 take two passes and the second reads its
    gold lists, excluded rows and outputs from query 4 096 on.  The queries are 41 noisy copies of rows, repeated: the
    second pass holds copies 37 .. 40 where the first begins with 0 .. 3.  Every one of those four has a planted rank of 1
    or more, two of them exclude a row, and the reference itself answers each of them differently once it is given the
    gold lists, or the excluded rows, of queries 0 .. 3 instead."""
    n, base = 64 * 5 + 7, 41
    frm, until = 5, n - 3
    assert flat_chunks(frm, until, 4100, 64)[0] == 4096
    X = unit_rows(7 * 64 + n, n, 64)
    dm = g.DeviceMatrix.from_host(X)
    try:
        pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(K, 64, ITERS))
        enc = pq.encode(dm)
    finally:
        dm.close()
    vi = g.PQIndex(pq, enc)
    try:
        Q, exclude = noisy_queries(64 + base, X, base, frm, until)
        ids = np.arange(frm, until)
        w = {"dist": distances_by_row(vi.batch_query_raw(len(ids), Q, frm, until), ids), "ids": ids, "exclude": exclude}
        offsets = draw_offsets(301, n)
        offsets[exclude[exclude >= 0]] = 0.0                     # an excluded row would be a candidate otherwise
        order = rank_ref.full_order(g, w, offsets)
        kinds = ("three", "at1", "at64", "at-1")
        planted = {kind: rank_ref.plant(kind, order, w, offsets, None, None) for kind in kinds}
        gold = [planted[kinds[q % 4]][q] for q in range(base)]
        want = rank_ref.reference(g, w, offsets, gold)
        rank_ref.same(vi.batch_query_rank_raw(Q, gold, offsets, exclude, frm, until), want)      # one pass

        pick = np.arange(4100) % base
        head, tail = pick[:4], pick[4096:]
        assert (want[0][tail] >= 1).all() and (exclude[tail] >= 0).sum() == 2
        there = dict(w, dist=w["dist"][tail], exclude=exclude[tail])
        other_gold = rank_ref.reference(g, there, offsets, [gold[q] for q in head])
        other_rows = rank_ref.reference(g, dict(there, exclude=exclude[head]), offsets, [gold[q] for q in tail])
        assert (other_gold[1] != want[1][tail]).all() and (other_rows[3] != want[3][tail]).all()

        got = vi.batch_query_rank_raw(Q[pick], [gold[q] for q in pick], offsets, exclude[pick], frm, until)
        rank_ref.same(got, tuple(a[pick] for a in want))
    finally:
        vi.close()


def test_wide_index_view_and_tables_past_the_lds_budget_are_refused(g):
    X = unit_rows(59, 1500, 32)
    dm = g.DeviceMatrix.from_host(X)
    wide = g.Index.sorted(dm, g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(1024, 4, 1)), "l2")
    try:
        with pytest.raises(NotImplementedError, match="byte codes"):
            wide.batch_query_rank_raw(X[:2], [[1], [2]])
    finally:
        wide.vector_index.close()
        dm.close()
    w = world(g, 16, 19)
    view = w["vi"].select(rows=np.arange(0, N, 2))
    try:
        with pytest.raises(NotImplementedError, match="view"):
            view.batch_query_rank_raw(w["Q"], [[0]] * 19)
    finally:
        view.close()
    # m = 148 is m_pad = 148: the tables of one query are 148 KiB, more than the 144 a workgroup may take, so no slot fits.
    # No byte-code handle is made for such an m (gulon_index_create refuses with the same words), so there is none to ask.
    assert flat_slots(148, 19)[2:4] == (148, 0)
    X = unit_rows(61, 600, 148)
    dm = g.DeviceMatrix.from_host(X)
    try:
        pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(K, 148, 1))
        enc = pq.encode(dm)
    finally:
        dm.close()
    with pytest.raises(NotImplementedError, match=r"m = 148 .* LDS"):
        g.PQIndex(pq, enc)


def test_host_checks(g):
    w = world(g, 16, 19)
    vi, Q, b = w["vi"], w["Q"], 19
    gold = [[100]] * b
    for bad in (np.nan, -np.inf):
        off = np.zeros(N, np.float32)
        off[77] = bad
        with pytest.raises(ValueError, match=r"row_offsets\[77\]"):
            vi.batch_query_rank_raw(Q, gold, off)
    for bad in (N, -1):
        lists = [[100]] * 5 + [[200, bad]] + [[100]] * (b - 6)
        with pytest.raises(ValueError, match=r"gold_rows\[6\] = %d" % bad):
            vi.batch_query_rank_raw(Q, lists)
    exclude = np.full(b, -1, np.int32)
    exclude[2] = N
    with pytest.raises(ValueError, match=r"exclude\[2\]"):
        vi.batch_query_rank_raw(Q, gold, None, exclude)
    for frm, until in ((-1, N), (0, N + 1), (9, 8)):
        with pytest.raises(ValueError):
            vi.batch_query_rank_raw(Q, gold, None, None, frm, until)
    NAT, L = g.native, g.native.lib()
    out_i, out_f = np.zeros(b, np.int32), np.zeros(b, np.float32)
    goff = np.arange(b + 1, dtype=np.int32)
    goff[9] = 7                                                  # descends after entry 8
    with pytest.raises(ValueError, match=r"gold_offsets\[9\] = 7 < gold_offsets\[8\] = 8"):
        NAT.check(L.gulon_index_query_rank(vi._h, Q.reshape(-1), b, 0, N, None, None, goff, np.full(b, 100, np.int32),
                                           out_i, out_i.copy(), out_f, None))
    rank, row, key, total = vi.batch_query_rank_raw(Q, gold, None, None, 64, 64)        # an empty range
    assert (rank == -1).all() and (row == -1).all() and np.isposinf(key).all() and (total == 0).all()
    assert [len(a) for a in vi.batch_query_rank_raw(np.zeros((0, 32), np.float32), [])] == [0, 0, 0, 0]
