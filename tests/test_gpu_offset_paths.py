"""The offset scans (csrc/offset.hip) on the paths test_gpu_offset_flat.py and test_gpu_offset_exact.py do
not reach: rows of several code words, slot counts E that the LDS budget forces (4, 2, 1, and the refusal past 144 KiB),
a second pass of the flat form, three ragged row chunks, tie groups larger than a list, negative keys, non-finite keys
that come from the arithmetic, and a flat handle with a row base and its context.

The reference is the one of those two files: the handle's own ordinary query at k = the rows of its range, scattered
back by row id, through csls.offset_query_reference; rows, key BITS and counts (offset_ref.same), no tolerance.  The
distances of the multi-word worlds are themselves checked bit for bit against the oracle.  Every test first asserts, from
the reference side alone, that the case it names occurs in its inputs; the launch geometry is not observable, so it is
derived by offset_ref.flat_slots / flat_chunks, which restate the launcher's arithmetic.

Flat worlds: 256 centroids, one training iteration, unit rows, 64 * 5 + 7 rows and the range [5, n - 3) unless a case
says otherwise.  Exact worlds: 700 rows, d = 33, the handle over [37, 695), 17 queries."""
import numpy as np
import pytest

from conftest import bits
from cosmul_ref import exact_distances as numpy_distances
from cosmul_ref import unit_rows
from offset_ref import (HUGE, LEVELS, SIGNED_LEVELS, ceil_div, distances_by_row, distances_in_steps, draw_offsets,
                        flat_chunks, flat_slots, huge_offsets, noisy_queries, nonfinite_queries, own_or_nan, padded,
                        plant_nearest, run_dev, same, sign_change_inside)

pytestmark = pytest.mark.gpu

N = 64 * 5 + 7
N_CHUNKED = 64 * 100 + 7                     # the range's 101 code blocks: three chunks of 34, 34 and 33
K, ITERS = 256, 1
DIMENSIONS = {3: 32, 16: 32, 25: 50, 32: 64, 64: 64, 80: 80, 144: 144, 148: 148}
# m -> (vec, ng, m_pad, E): what the launcher derives for a batch of 5
SLOTS = {25: (4, 7, 28, 4), 32: (16, 2, 32, 4), 64: (16, 4, 64, 2), 80: (16, 5, 80, 1), 144: (16, 9, 144, 1)}
BASE = 1000


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


# ---------------------------------------------------------------- flat index
_WORLDS = {}


def finish(g, key, vi, X, Q, exclude, extra):
    n = vi.length
    ids = np.arange(5, n - 3)
    dist = distances_by_row(vi.batch_query_raw(len(ids), Q, 5, n - 3), ids)
    _WORLDS[key] = dict({"vi": vi, "X": X, "Q": Q, "exclude": exclude, "dist": dist, "ids": ids, "n": n}, **extra)
    return _WORLDS[key]


def world(g, m, b=5):
    """A PQIndex trained on N unit rows of DIMENSIONS[m] dimensions, b noisy copies of rows of [5, N - 3) as queries, the
    rows they exclude, and the distances [b][N - 8] of the handle's ordinary query over that range."""
    key = (m, b)
    if key not in _WORLDS:
        X = unit_rows(7 * m + N, N, DIMENSIONS[m])
        dm = g.DeviceMatrix.from_host(X)
        try:
            pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(K, m, ITERS))
            enc = pq.encode(dm)
        finally:
            dm.close()
        Q, exclude = noisy_queries(m + b, X, b, 5, N - 3)
        finish(g, key, g.PQIndex(pq, enc), X, Q, exclude, {"pq": pq, "enc": enc, "m": m})
    return _WORLDS[key]


def tie_world(g):
    """N_CHUNKED rows, row r = base[r % 8], encoded by the m = 16 world's quantizer: eight classes of equal rows."""
    if "ties" not in _WORLDS:
        pq = world(g, 16)["pq"]
        base = unit_rows(61, 8, DIMENSIONS[16])
        X = base[np.arange(N_CHUNKED) % 8]
        dm = g.DeviceMatrix.from_host(X)
        try:
            enc = pq.encode(dm)
        finally:
            dm.close()
        Q, _ = noisy_queries(62, base, 5, 0, 8)
        finish(g, "ties", g.PQIndex(pq, enc), X, Q, None, {"m": 16})
    return _WORLDS["ties"]


@pytest.fixture(scope="module", autouse=True)
def close_worlds():
    yield
    for w in _WORLDS.values():
        w["vi"].close()
    _WORLDS.clear()
    for w in _EXACT.values():
        w["ix"].close()
        w["dm"].close()
    _EXACT.clear()


def reference(g, w, offsets, k, exclude, base=0):
    return g.offset_query_reference(w["dist"], offsets[5:w["n"] - 3], k, exclude, rows=w["ids"] + base)


def ask(w, k, offsets, exclude, Q=None):
    return w["vi"].batch_query_offset_raw(k, w["Q"] if Q is None else Q, offsets, exclude, 5, w["n"] - 3)


def lds_bound(m, b=5):
    """The geometry a case at m quantizers names, from the launcher's arithmetic alone: several code words per row, E
    lowered by the LDS budget and not by the batch, two workgroups or more, idle slots in the last where E > 1."""
    vec, ng, m_pad, e_lds, e = flat_slots(m, b)
    assert (vec, ng, m_pad, e) == SLOTS[m] and ng >= 2
    assert e == e_lds < 8 and e * m_pad <= 144 < 2 * e * m_pad
    assert ceil_div(b, e) >= 2 and (e == 1 or b % e != 0)
    return e


@pytest.mark.parametrize("m,k", [(25, 1), (25, 10), (25, 63), (32, 10), (64, 1), (64, 10), (64, 63), (80, 10), (144, 10)])
def test_flat_multi_word_rows_at_every_lds_bound_slot_count(g, m, k):
    """m = 25: seven 4-byte words, 28 KiB a slot, E = 4; m = 32, 64, 80, 144: two, four, five and nine 16-byte words, E =
    4, 2, 1, 1 -- at m = 144 one slot is the whole budget.  E = the largest of 8, 4, 2, 1 that is <= 144 KiB // max(m_pad
    KiB, 8 KiB), halved while E > 1 and E / 2 >= b; five queries leave the last workgroup of E = 4 and of E = 2 with idle
    zero-table slots."""
    lds_bound(m)
    w = world(g, m)
    offsets = draw_offsets(100 + m + k, N)
    want = reference(g, w, offsets, k, w["exclude"])
    assert (want[2] == k).all()
    got = ask(w, k, offsets, w["exclude"])
    same(got, want)
    assert padded(got)
    same(ask(w, k, offsets, None), reference(g, w, offsets, k, None))


@pytest.mark.parametrize("m", (25, 64))
def test_flat_multi_word_distances_match_the_oracle(g, oracle, m):
    """The reference's distances are the handle's own: here they are the oracle's, bit for bit, at K = the rows of the
    index -- an error in a table of the second or a later code word could not hide in them."""
    w = world(g, m)
    assert flat_slots(m, 5)[1] >= 2
    oi, od, oc = oracle.pq_batch_query(w["vi"].indices(), DIMENSIONS[m], K, w["pq"].flat_centroids(), w["Q"], N)
    full = distances_by_row((oi, od, oc), np.arange(N))
    assert np.array_equal(bits(full[:, 5:N - 3]), bits(w["dist"]))


@pytest.mark.parametrize("k", (1, 10, 63))
def test_flat_multi_word_dev_form(g, k):
    lds_bound(25)
    w = world(g, 25)
    offsets = draw_offsets(200 + k, N)
    L = g.native.lib()

    def call(d_q, b, kk, d_off, d_ex, d_oi, d_ok, d_oc):
        return L.gulon_index_query_offset_dev(w["vi"]._h, d_q, b, kk, 5, N - 3, d_off, d_ex, d_oi, d_ok, d_oc, None)
    same(run_dev(g, call, w["Q"], k, offsets, w["exclude"]), reference(g, w, offsets, k, w["exclude"]))
    same(run_dev(g, call, w["Q"], k, offsets, None), reference(g, w, offsets, k, None))


def test_flat_tables_past_the_lds_budget_are_refused(g):
    """m = 148 is m_pad = 148: one query's tables are 148 KiB, more than the 144 there are, and no slot fits.  The
    refusal comes before any offset query can be asked: gulon_index_create makes no byte-code handle whose table is past
    the same 144 KiB (NotImplementedError naming m and the LDS), so check_flat's own test of offset_flat_max_e guards a
    state no handle is in, and m = 144 -- answered above -- is the largest there is.  After the refusals the m = 144
    handle answers an offset query and its ordinary query as before."""
    assert flat_slots(148, 5)[2:4] == (148, 0) and flat_slots(144, 5)[2:4] == (144, 1)
    X = unit_rows(7 * 148 + N, N, DIMENSIONS[148])
    dm = g.DeviceMatrix.from_host(X)
    try:
        pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(K, 148, ITERS))
        enc = pq.encode(dm)
    finally:
        dm.close()
    for _ in range(2):
        with pytest.raises(NotImplementedError, match=r"m = 148 .* LDS"):
            g.PQIndex(pq, enc)
    w = world(g, 144)
    offsets = draw_offsets(148, N)
    same(ask(w, 10, offsets, w["exclude"]), reference(g, w, offsets, 10, w["exclude"]))
    again = distances_by_row(w["vi"].batch_query_raw(len(w["ids"]), w["Q"], 5, N - 3), w["ids"])
    assert np.array_equal(bits(again), bits(w["dist"]))


def test_flat_more_queries_than_one_pass_holds(g):
    """m = 64: 256 MiB of tables are 4 096 queries, so 4 100 take two passes; the second starts at a query whose
    excluded row differs from the first pass's first, and whose answer holds that row once it is not excluded."""
    w = world(g, 64)
    assert flat_chunks(5, N - 3, 4100, 64)[0] == 4096 and flat_slots(64, 4100)[4] == 2
    ex = w["exclude"]
    offsets = draw_offsets(300, N)
    offsets[ex[ex >= 0]] = 0.0
    pick = np.arange(4100) % 5
    exclude = ex[pick]
    assert (exclude[4096:] != exclude[:4]).all()
    want = reference(g, w, offsets, 10, ex)
    unexcluded = reference(g, w, offsets, 10, None)
    for q in np.flatnonzero(ex >= 0):
        assert ex[q] in unexcluded[0][q].tolist() and ex[q] not in want[0][q].tolist()
    same(ask(w, 10, offsets, ex), want)
    same(ask(w, 10, offsets, exclude, Q=w["Q"][pick]), tuple(a[pick] for a in want))


@pytest.mark.parametrize("excluding", (False, True))
@pytest.mark.parametrize("k", (10, 63))
def test_flat_tie_groups_larger_than_a_list_across_three_chunks(g, k, excluding):
    """Eight classes of about 700 equal rows with one offset each, a tenth of the rows masked: a query's answer is the
    first k candidates of one class, which has more than 64 members in each of the three row chunks -- every wave list
    and every chunk list is full of one key, and the row id alone decides what the merges keep."""
    w = tie_world(g)
    n, ids = N_CHUNKED, w["ids"]
    assert flat_chunks(5, n - 3, 5, 16)[1:] == (3, 34) and ceil_div(n - 3, 64) - 2 * 34 == 33
    rng = np.random.default_rng(63)
    offsets = LEVELS[rng.permutation(8)][np.arange(n) % 8]
    offsets[rng.random(n) < 0.1] = np.inf
    first = reference(g, w, offsets, 1, None)[0][:, 0]
    exclude = first.astype(np.int32) if excluding else None         # the winning class's smallest candidate
    want = reference(g, w, offsets, k + 1, exclude)
    for q in range(5):
        assert want[2][q] == k + 1 and want[1][q, k - 1] == want[1][q, k]
        members = ids[(ids % 8 == first[q] % 8) & np.isfinite(offsets[ids])]
        assert (w["dist"][q][members - 5] == w["dist"][q][first[q] - 5]).all()
        for chunk in range(3):
            assert np.sum(members // (34 * 64) == chunk) > 64
        if excluding:
            assert members[0] == first[q]
            members = members[1:]
        assert want[0][q].tolist() == members[:k + 1].tolist()
    want = tuple(a[:, :k] if a.ndim == 2 else np.minimum(a, k) for a in want)
    got = ask(w, k, offsets, exclude)
    same(got, want)
    assert padded(got)


@pytest.mark.parametrize("k", (10, 63))
@pytest.mark.parametrize("m", (3, 25))
def test_flat_negative_keys(g, m, k):
    """Offsets from SIGNED_LEVELS (r_S of CSLS is negative for isolated rows), -1.5 at every query's nearest candidate:
    every answer starts with negative keys and turns positive inside the first k."""
    w = world(g, m)
    offsets = plant_nearest(draw_offsets(400 + m, N, levels=SIGNED_LEVELS), w["dist"], w["ids"], w["exclude"], -1.5)
    assert (offsets[np.isfinite(offsets)] < 0).any() and np.signbit(offsets[offsets == 0]).any()
    want = reference(g, w, offsets, k, w["exclude"])
    assert sign_change_inside(want)
    got = ask(w, k, offsets, w["exclude"])
    same(got, want)
    assert padded(got)


def check_nonfinite(want, dist, offsets, ids, exclude, at, k):
    """From the reference alone: the NaN, +inf and far queries have no finite distance and no answer; the edge query's
    distances and the offsets are all finite (or +inf masks), its keys overflow exactly at the HUGE offsets, and it
    answers with the other rows only, fewer than k; every other query's list is full."""
    nan, inf, far, edge = at
    assert np.isnan(dist[nan]).all() and np.isposinf(dist[inf]).all() and np.isposinf(dist[far]).all()
    assert want[2][[nan, inf, far]].tolist() == [0, 0, 0]
    off = offsets[ids]
    assert np.isfinite(dist[edge]).all() and (np.isfinite(off) | np.isposinf(off)).all()
    with np.errstate(over="ignore"):
        keys = (dist[edge] + off).astype(np.float32)
    assert np.array_equal(np.isposinf(keys) & np.isfinite(off), off == HUGE) and (off == HUGE).sum() > len(ids) // 2
    left = ids[np.isfinite(keys) & (ids != exclude[edge])]
    assert 0 < len(left) < k and want[2][edge] == len(left)
    assert sorted(want[0][edge, :len(left)].tolist()) == left.tolist()
    ordinary = np.setdiff1d(np.arange(len(dist)), at)
    assert np.isfinite(dist[ordinary]).all() and (want[2][ordinary] == k).all()
    return ordinary


def test_flat_non_finite_keys(g):
    """One workgroup of six queries: a NaN component, a +inf component, components of 1e19 (every distance overflows),
    components of 3e18 against offsets of 3e38 (finite + finite overflows), two ordinary ones."""
    w = world(g, 16, b=6)
    assert flat_slots(16, 6)[4] == 8
    at, k = (0, 1, 2, 3), 63
    Q = nonfinite_queries(w["Q"], at)
    dist = distances_in_steps(lambda kk, f, u: w["vi"].batch_query_raw(kk, Q, f, u), 5, N - 3,
                              w["vi"].batch_query_raw(N - 8, Q, 5, N - 3))
    offsets = huge_offsets(500, N, np.arange(8, N - 3, 8))
    v = dict(w, dist=dist)
    want = reference(g, v, offsets, k, w["exclude"])
    ordinary = check_nonfinite(want, dist, offsets, w["ids"], w["exclude"], at, k)
    got = ask(w, k, offsets, w["exclude"], Q=Q)
    same(got, want)
    assert padded(got)
    alone = ask(w, k, offsets, w["exclude"][ordinary], Q=Q[ordinary])
    same(alone, tuple(a[ordinary] for a in got))
    same(ask(w, 10, offsets, w["exclude"], Q=Q), reference(g, v, offsets, 10, w["exclude"]))


def test_flat_row_base_and_context(g):
    """A handle at row base 1000 over the m = 16 world's codes: offsets are indexed by local row, exclude and the answers
    are global ids, the host checks move with the base; its context() answers identically."""
    w = world(g, 16)
    ex = w["exclude"]
    exclude = np.where(ex >= 0, ex + BASE, -1).astype(np.int32)
    offsets = draw_offsets(600, N)
    offsets[ex[ex >= 0]] = 0.0
    based = g.PQIndex(w["pq"], w["enc"], row_base=BASE)
    ctx = None
    try:
        dist = distances_by_row(based.batch_query_raw(len(w["ids"]), w["Q"], 5, N - 3), w["ids"] + BASE)
        assert np.array_equal(bits(dist), bits(w["dist"]))
        for k in (10, 63):
            want = reference(g, w, offsets, k, exclude, base=BASE)
            unexcluded = reference(g, w, offsets, k, None, base=BASE)
            for q in np.flatnonzero(ex >= 0):      # the excluded row would be there; as a local row it names nothing
                assert exclude[q] in unexcluded[0][q].tolist() and exclude[q] not in want[0][q].tolist()
                assert exclude[q] >= N
            got = based.batch_query_offset_raw(k, w["Q"], offsets, exclude, 5, N - 3)
            same(got, want)
            assert padded(got) and got[0][got[0] >= 0].min() >= BASE + 5
            plain = ask(w, k, offsets, ex)
            same(got, (np.where(plain[0] >= 0, plain[0] + BASE, -1), plain[1], plain[2]))
        for bad in (BASE - 1, BASE + N):
            wrong = exclude.copy()
            wrong[1] = bad
            with pytest.raises(ValueError, match=r"exclude\[1\]"):
                based.batch_query_offset_raw(10, w["Q"], offsets, wrong, 5, N - 3)
        edge = exclude.copy()
        edge[1] = BASE                                               # row 0: accepted, and outside the range
        same(based.batch_query_offset_raw(10, w["Q"], offsets, edge, 5, N - 3),
             reference(g, w, offsets, 10, edge, base=BASE))
        ctx = based.context()
        same(ctx.batch_query_offset_raw(63, w["Q"], offsets, exclude, 5, N - 3), got)
        dev = g.DeviceOffsets.from_host(offsets)
        try:
            same(ctx.batch_query_offset_raw(63, w["Q"], dev, exclude, 5, N - 3), got)
        finally:
            dev.free()
        same(based.batch_query_offset_raw(63, w["Q"], offsets, exclude, 5, N - 3), got)
    finally:
        if ctx is not None:
            ctx.close()
        based.close()


# ---------------------------------------------------------------- exact index
EN, ED, FROM, UNTIL, EB = 700, 33, 37, 695, 17
_EXACT = {}


def exact_world(g, name):
    """(handle over [37, 695), X, queries, excluded rows, the handle's distances [17][658]): "unit" -- unit rows, the
    queries noisy copies of rows of the range; "ties" -- row r = base[r % 4], the queries noisy copies of base rows."""
    if name not in _EXACT:
        if name == "unit":
            X = unit_rows(71, EN, ED)
            Q, exclude = noisy_queries(72, X, EB, FROM, UNTIL)
        else:
            base = unit_rows(73, 4, ED)
            X = base[np.arange(EN) % 4]
            Q, exclude = noisy_queries(74, base, EB, 0, 4)[0], None
        dm = g.DeviceMatrix.from_host(X)
        ix = g.ExactIndex(dm, "l2", FROM, UNTIL)
        _EXACT[name] = {"ix": ix, "dm": dm, "X": X, "Q": Q, "exclude": exclude, "ids": np.arange(FROM, UNTIL),
                        "dist": exact_distances(ix, Q)}
    return _EXACT[name]


def exact_distances(ix, Q):
    ids = np.arange(FROM, UNTIL)
    return distances_by_row(ix.batch_query_raw(len(ids), Q), ids)


def exact_reference(g, w, offsets, k, exclude, dist=None):
    return g.offset_query_reference(w["dist"] if dist is None else dist, offsets[FROM:UNTIL], k, exclude, rows=w["ids"])


@pytest.mark.parametrize("k", (10, 63))
def test_exact_negative_keys(g, k):
    """As test_flat_negative_keys.  (On unit rows of 33 dimensions about fifty rows are nearer than 1.5 to a query, so
    a draw can put ten negative keys into a list: this one puts six at the most, which the assertion checks.)"""
    w = exact_world(g, "unit")
    offsets = plant_nearest(draw_offsets(719, EN, levels=SIGNED_LEVELS), w["dist"], w["ids"], w["exclude"], -1.5)
    assert (offsets[np.isfinite(offsets)] < 0).any() and np.signbit(offsets[offsets == 0]).any()
    want = exact_reference(g, w, offsets, k, w["exclude"])
    assert sign_change_inside(want)
    got = w["ix"].batch_query_offset_raw(k, w["Q"], offsets, w["exclude"])
    same(got, want)
    assert padded(got)


@pytest.mark.parametrize("k", (10, 63))
def test_exact_tie_groups_larger_than_a_list(g, k):
    """Four classes of equal rows, one offset each, a tenth of the rows masked: the answer is the winning class's first
    k candidates after the excluded one, its smallest.  The class has more than 64 candidates and some in every 256-row
    group, so equal keys meet inside a wave's list, between the waves of a workgroup and between row chunks."""
    w = exact_world(g, "ties")
    ids = w["ids"]
    rng = np.random.default_rng(75)
    offsets = LEVELS[rng.permutation(8)[:4]][np.arange(EN) % 4]
    offsets[rng.random(EN) < 0.1] = np.inf
    first = exact_reference(g, w, offsets, 1, None)[0][:, 0]
    exclude = first.astype(np.int32)
    want = exact_reference(g, w, offsets, k + 1, exclude)
    for q in range(EB):
        assert want[2][q] == k + 1 and want[1][q, k - 1] == want[1][q, k]
        members = ids[(ids % 4 == first[q] % 4) & np.isfinite(offsets[ids])]
        assert (w["dist"][q][members - FROM] == w["dist"][q][first[q] - FROM]).all()
        assert len(members) > 64 and set((members // 256).tolist()) == {0, 1, 2} and members[0] == first[q]
        assert want[0][q].tolist() == members[1:k + 2].tolist()
    want = tuple(a[:, :k] if a.ndim == 2 else np.minimum(a, k) for a in want)
    got = w["ix"].batch_query_offset_raw(k, w["Q"], offsets, exclude)
    same(got, want)
    assert padded(got)
    same(w["ix"].batch_query_offset_raw(k, w["Q"], offsets), tuple(
        a[:, :k] if a.ndim == 2 else np.minimum(a, k) for a in exact_reference(g, w, offsets, k + 1, None)))


def test_exact_non_finite_keys(g):
    """The first query tile holds a NaN query, a +inf query, one whose distances overflow, one whose keys overflow at
    the offsets of 3e38, and twelve ordinary ones; the second tile holds the seventeenth."""
    w = exact_world(g, "unit")
    at, k = (3, 5, 7, 9), 63
    Q = nonfinite_queries(w["Q"], at)
    dist = own_or_nan(w["ix"].batch_query_raw(UNTIL - FROM, Q), w["ids"], numpy_distances(w["X"][FROM:UNTIL], Q))
    assert np.flatnonzero(np.isnan(dist).all(axis=1)).tolist() == [at[0]]
    offsets = huge_offsets(800, EN, np.arange(FROM + 3, UNTIL, 16))
    want = exact_reference(g, w, offsets, k, w["exclude"], dist)
    ordinary = check_nonfinite(want, dist, offsets, w["ids"], w["exclude"], at, k)
    assert (ordinary < 16).sum() == 12 and ordinary[-1] == 16
    got = w["ix"].batch_query_offset_raw(k, Q, offsets, w["exclude"])
    same(got, want)
    assert padded(got)
    alone = w["ix"].batch_query_offset_raw(k, Q[ordinary], offsets, w["exclude"][ordinary])
    same(alone, tuple(a[ordinary] for a in got))
    same(w["ix"].batch_query_offset_raw(10, Q, offsets, w["exclude"]),
         exact_reference(g, w, offsets, 10, w["exclude"], dist))
