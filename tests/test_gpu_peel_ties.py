"""The large-K peel (PeelRounds, peel_update, peel_finalize, peel_export and the eligibility test of the scan kernels)
on indexes where most of the nearest rows tie: K > 63 gets no tie replay, so the answer is the plain (distance, row id)
order, and it is compared in full -- rows, distance bits, count and flags of every query; nothing "up to ties".

Indexes come from explicit code matrices.  A few base code rows are copied to groups of rows that a permutation
scatters over the whole row range, so tie-mates sit in different row blocks, waves and chunks.  Groups A, B and C
differ in quantizer 0 only (B and C hold the two codes nearest to A's), so for the query "decoded A" they fill entries
0..69, 70..139 and 140..239: a group across entries 63/64, one across 127/128, and one across every K cut used here.
Group D is 300 copies of an unrelated row.

The expected answer comes from the oracle only: the distance of every row (oracle.pq_batch_query at K = n), ordered
by np.lexsort((row, distance)); tests/merge_ref.py turns that into output slots, count and flags, and restates the
peel for the shards' partial lists."""
import numpy as np
import pytest

import merge_ref as mr
from batch_seams_ref import wide_sub_batch
from conftest import bits
from test_gpu_merge import Dev, merge_dev

pytestmark = pytest.mark.gpu

N_ROWS = 20000
GROUPS = (("A", 70), ("B", 70), ("C", 100), ("D", 300))
FORMS = {
    "byte16": dict(d=32, m=16, k=256),      # one code word per row (a default build scans its plain codes: DESIGN 9ae)
    "byte8": dict(d=16, m=8, k=256),
    "byte40": dict(d=40, m=40, k=256),      # ten 4-byte code words per row, two queries per table entry
    "wide": dict(d=32, m=16, k=1024),       # wide.hip
}
B_TILE = 37                                 # more than the 16 queries of the largest query tile (m = 8)


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


# ---- the launch shapes, restated ------------------------------------------------------------------------------------------

def ceil_div(a, b):
    return -(-a // b)


def scan_chunks(row_blocks, want, waves):
    """scan.hpp: about `want` chunks, at least two row blocks per wave."""
    nchunks = max(1, min(want, row_blocks // (2 * waves)))
    per_chunk = ceil_div(row_blocks, nchunks)
    return ceil_div(row_blocks, per_chunk)


def byte_query_tile(m):
    """gulon_index_create: W queries interleaved per table entry, NSUB sub-tables, within 144 KiB of LDS."""
    m_pad = m if m % 16 == 0 else ceil_div(m, 4) * 4
    w = 4
    while w > 1 and m_pad * 256 * w * 4 > 144 * 1024:
        w //= 2
    per_sub = m_pad * 256 * w * 4
    nsub = 1 if w < 4 else 4 if 4 * per_sub <= 144 * 1024 else 2 if 2 * per_sub <= 144 * 1024 else 1
    return w * nsub


def nchunks_of(form, B, frm, until):
    f = FORMS[form]
    rb = ceil_div(until, 64) - frm // 64
    if form == "wide":
        return scan_chunks(rb, ceil_div(2048, wide_sub_batch(B, f["m"], f["k"], rb * 64)), 8)
    return scan_chunks(rb, ceil_div(4096, ceil_div(B, byte_query_tile(f["m"]))), 16)


def test_launch_shapes_restated():
    assert [byte_query_tile(m) for m in (8, 16, 40)] == [16, 8, 2]
    for form in FORMS:
        assert nchunks_of(form, B_TILE, 0, N_ROWS) >= 2 and nchunks_of(form, 1, 0, N_ROWS) >= 2
        assert nchunks_of(form, 5, 0, 500) == 1
        assert form == "wide" or B_TILE > 2 * byte_query_tile(FORMS[form]["m"])
    # the wide sub-batch: a table is m * k * 4 = 64 KiB here, so 1 GiB holds 16 384 queries' -- 37 are ONE sub-batch.  A
    # sub-batch below 37 needs > 27 MiB of tables per query (m * k > 7 M), which no index of this file's size has
    # (tests/test_gpu_batch_seams.py crosses that seam).
    f = FORMS["wide"]
    assert wide_sub_batch(B_TILE, f["m"], f["k"], ceil_div(N_ROWS, 64) * 64) == B_TILE
    assert wide_sub_batch(B_TILE, 112, 65536, 64) == 36


# ---- the worlds -------------------------------------------------------------------------------------------------------------

class World:
    pass


def _index(g, w, idx, lo=0, hi=None):
    hi = idx.shape[1] if hi is None else hi
    pq = g.ProductQuantizer.from_flat(w.k, w.d, w.m, w.cents)
    coder = pq.coder_factory(hi - lo)
    enc = g.EncodedMatrix(coder, [coder.build_code(np.ascontiguousarray(idx[j, lo:hi])) for j in range(idx.shape[0])])
    return g.PQIndex(pq, enc, row_base=lo)


def _all_distances(oracle, w, idx, Q):
    """[B][n] distance of every row, from the oracle alone (a heap of n entries evicts nothing)."""
    n = idx.shape[1]
    oi, od, oc = oracle.pq_batch_query(idx, w.d, w.k, w.cents, Q, n, 0, n)
    assert (oc == n).all()
    D = np.zeros((len(Q), n), np.float32)
    for q in range(len(Q)):
        assert np.array_equal(np.sort(oi[q]), np.arange(n))
        D[q, oi[q]] = od[q]
    return D


@pytest.fixture(scope="module")
def worlds(oracle, g):
    """One world per index form, built when first asked for: codes, queries, the oracle's distance of every row, and
    the handle every whole-index case shares."""
    made = {}

    def get(form):
        if form not in made:
            made[form] = build_world(oracle, form)
            made[form].ix = _index(g, made[form], made[form].idx)
        return made[form]

    yield get
    for w in made.values():
        w.ix.close()


def build_world(oracle, form):
    """Oracle and numpy only."""
    w = World()
    w.form, w.n = form, N_ROWS
    w.d, w.m, w.k = (FORMS[form][x] for x in "dmk")
    rng = np.random.default_rng(sorted(FORMS).index(form) + 40)
    w.cents = rng.standard_normal(w.k * w.d).astype(np.float32)
    idx = rng.integers(0, w.k, (w.m, w.n)).astype(np.int32)
    # base rows: A random; B, C = A with the two codes of quantizer 0 nearest to A's; D unrelated
    base = {"A": rng.integers(0, w.k, w.m).astype(np.int32), "D": rng.integers(0, w.k, w.m).astype(np.int32)}
    probe = idx[:, :1].copy()
    probe[:, 0] = base["A"]
    qa = oracle.pq_decode(probe, w.d, w.k, w.cents)[:1]
    near = np.argsort(oracle.prepare_query(w.cents, w.d, w.m, w.k, qa)[0, 0], kind="stable")
    assert near[0] == base["A"][0]
    for name, c in (("B", near[1]), ("C", near[2])):
        base[name] = base["A"].copy()
        base[name][0] = c
    perm = rng.permutation(w.n)
    w.members, at = {}, 0
    for name, size in GROUPS:
        w.members[name] = np.sort(perm[at:at + size])
        idx[:, w.members[name]] = base[name][:, None]
        at += size
    w.idx = idx
    # B_TILE queries, tied and untied mixed: the four decoded base rows, noisy copies of them, decoded ordinary rows,
    # random vectors
    X = oracle.pq_decode(idx, w.d, w.k, w.cents)
    dec = {name: X[w.members[name][0]] for name, _ in GROUPS}
    Q = rng.standard_normal((B_TILE, w.d)).astype(np.float32)
    for slot, name in ((0, "A"), (2, "B"), (3, "C"), (5, "D"), (20, "A"), (36, "D")):
        Q[slot] = dec[name]
    for slot, name in ((7, "A"), (8, "D"), (30, "C")):
        Q[slot] = dec[name] + (rng.standard_normal(w.d) * 1e-3).astype(np.float32)
    for slot in (10, 11, 25):
        Q[slot] = X[perm[-slot]]
    w.Q = Q
    w.D = _all_distances(oracle, w, idx, Q)
    return w


def expected(D, rows, K):
    """The (distance, row id) answer over `rows` (global ids, columns of D): idx, dist bits, count, flags."""
    B = D.shape[0]
    ei, ed = np.zeros((B, K), np.int32), np.zeros((B, K), np.float32)
    ec, ef = np.zeros(B, np.int32), np.zeros(B, np.int32)
    order = []
    for q in range(B):
        d = D[q, rows]
        o = np.lexsort((rows, d))[:max(K + 2, 302)]
        ei[q], ed[q], ec[q], ef[q] = mr.finalize(rows[o][:K + 1], d[o][:K + 1], K)
        order.append(d[o])
    return ei, bits(ed), ec, ef, order


def check(ix, Q, K, exp, frm=0, until=None):
    ei, ed, ec, ef, _ = exp
    oi, od, oc, of = ix.batch_query_raw(K, Q, frm, until)
    assert np.array_equal(oc, ec)
    assert np.array_equal(bits(od), ed)
    assert np.array_equal(oi, ei), np.flatnonzero((oi != ei).any(axis=1))
    assert np.array_equal(of, ef), (of, ef)
    assert ((of & 4) == 0).all()


# ---- the cases --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [64, 100, 128, 200])
@pytest.mark.parametrize("form", list(FORMS))
def test_tie_groups_across_round_boundaries_and_the_cut(oracle, g, worlds, form, K):
    w = worlds(form)
    sel = [0, 1, 2, 3, 7]                                  # decoded A, B, C with a random and a noisy query between
    exp = expected(w.D[sel], np.arange(w.n), K)
    sd = exp[4][0]
    assert sd[63] == sd[64] and sd[127] == sd[128] and sd[K - 1] == sd[K]     # query "A": groups across 63/64, 127/128, the cut
    assert sd[69] != sd[70] and sd[139] != sd[140]
    assert exp[3][0] == 3 and (exp[3] == 0).any()
    check(w.ix, w.Q[sel], K, exp)


@pytest.mark.parametrize("form", list(FORMS))
def test_tie_group_longer_than_a_round(oracle, g, worlds, form):
    """300 identical rows at K = 250: rounds 2 to 4 start inside the group, where only the id half of the bound moves."""
    w = worlds(form)
    sel = [5, 6]
    exp = expected(w.D[sel], np.arange(w.n), 250)
    sd = exp[4][0]
    assert sd[0] == sd[299] != sd[300] and exp[0][0].tolist() == w.members["D"][:250].tolist() and exp[3].tolist()[0] == 3
    check(w.ix, w.Q[sel], 250, exp)


@pytest.mark.parametrize("K", [200, 700])
@pytest.mark.parametrize("form", list(FORMS))
def test_every_row_identical(oracle, g, worlds, form, K):
    """500 copies of one code row: every query ties on every row; K = 700 > n leaves count = 500 and (-1, +inf) slots,
    and the rounds after the list is exhausted add nothing."""
    w = worlds(form)
    n = 500
    idx = np.repeat(w.idx[:, w.members["D"][:1]], n, axis=1)
    ix = _index(g, w, idx)
    Q = w.Q[[5, 1]]
    D = _all_distances(oracle, w, idx, Q)
    assert (D == D[:, :1]).all() and nchunks_of(form, 2, 0, n) == 1
    exp = expected(D, np.arange(n), K)
    assert exp[0][:, :min(K, n)].tolist() == [list(range(min(K, n)))] * 2
    assert exp[2].tolist() == [min(K, n)] * 2 and exp[3].tolist() == [3 if K < n else 2] * 2
    check(ix, Q, K, exp)
    ix.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_sub_range_of_a_shard_cuts_a_tie_group(oracle, g, worlds, form):
    w = worlds(form)
    lo, hi, frm, until, K = 4993, 15017, 1003, 8891, 100
    assert frm % 64 and until % 64 and nchunks_of(form, 5, frm, until) >= 2
    rows = np.arange(lo + frm, lo + until)
    for name in "AB":                                       # the range cuts through both groups
        inside = np.isin(w.members[name], rows).sum()
        assert 0 < inside < len(w.members[name])
    sel = [0, 1, 2, 5, 8]
    exp = expected(w.D[sel], rows, K)
    assert (exp[3] & 3 != 0).any() and (exp[2] == K).all()
    shard = _index(g, w, w.idx, lo, hi)
    check(shard, w.Q[sel], K, exp, frm, until)
    shard.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_batch_larger_than_a_query_tile(oracle, g, worlds, form):
    w = worlds(form)
    K = 100
    exp = expected(w.D, np.arange(w.n), K)
    assert (exp[3] != 0).sum() >= 6 and (exp[3] == 0).sum() >= 6          # flagged and unflagged queries mixed
    check(w.ix, w.Q, K, exp)


@pytest.mark.parametrize("form", list(FORMS))
def test_every_distance_infinite(oracle, g, worlds, form):
    """A query component of 3e19: every distance is +inf, so the (distance, row id) rule returns the first K rows by
    id, flagged as the ties they are, without a replay bit."""
    w = worlds(form)
    K = 100
    Q = w.Q[[1, 1]].copy()
    Q[0, 5] = np.float32(3e19)
    D = _all_distances(oracle, w, w.idx, Q)
    assert np.isposinf(D[0]).all() and np.isfinite(D[1]).all()
    exp = expected(D, np.arange(w.n), K)
    assert exp[0][0].tolist() == list(range(K)) and exp[3][0] == 3 and exp[2][0] == K
    check(w.ix, Q, K, exp)


@pytest.mark.parametrize("form", list(FORMS))
def test_used_handle_answers_like_a_fresh_one(oracle, g, worlds, form):
    """K = 200, then 64, then 200 on one handle: the peel buffers are sized per call."""
    w = worlds(form)
    sel = [0, 5, 1, 2]
    for K in (200, 64, 200):
        check(w.ix, w.Q[sel], K, expected(w.D[sel], np.arange(w.n), K))


@pytest.mark.parametrize("form", ["byte16", "wide"])
def test_shards_partial_lists_and_their_merge(oracle, g, worlds, form):
    """Four row shards at K = 200 through gulon_index_scan_partial_dev (peel_export): every partial list is the peel
    of its range cut to K + 1, and gulon_topk_merge_dev of the four is the unsharded answer, ties and flags included."""
    N = g.native
    w = worlds(form)
    K, sel = 200, [0, 1, 2, 5, 7]
    B, bounds = len(sel), [0, 7000, 7001, 19999, w.n]
    Q = np.ascontiguousarray(w.Q[sel])
    dq = Dev(N, Q)
    pv = np.zeros((4, B, K + 1), np.float32)
    pi = np.zeros((4, B, K + 1), np.int32)
    for s, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        dv, di = Dev(N, np.full(B * (K + 1) + 8, 0x5A5A5A5A, np.uint32)), Dev(N, np.full(B * (K + 1) + 8, 0x5A5A5A5A, np.uint32))
        shard = _index(g, w, w.idx, lo, hi)
        N.check(N.lib().gulon_index_scan_partial_dev(shard._h, dq.p, B, K, 0, hi - lo, dv.p, di.p, None))
        N.check(N.lib().gulon_device_synchronize())
        shard.close()
        rv, ri = dv.read(np.uint32), di.read(np.uint32)
        dv.free()
        di.free()
        assert (rv[B * (K + 1):] == 0x5A5A5A5A).all() and (ri[B * (K + 1):] == 0x5A5A5A5A).all()
        pv[s] = rv[:B * (K + 1)].view(np.float32).reshape(B, K + 1)
        pi[s] = ri[:B * (K + 1)].view(np.int32).reshape(B, K + 1)
        rows = np.arange(lo, hi)
        for q in range(B):
            ev, ei = mr.peel_partial(*mr.peeled_rounds(w.D[sel[q], lo:hi], rows, K), K)
            assert np.array_equal(pi[s, q], ei), (s, q)
            assert np.array_equal(bits(pv[s, q]), bits(ev)), (s, q)
    dq.free()
    mr.check_precondition(pv, pi)
    ei, ed, ec, ef, _ = expected(w.D[sel], np.arange(w.n), K)
    assert ef[0] == 3 and mr.cross_list_ties(pv, pi, K).max() >= 1           # a tie group spread over the shards
    rc, oi, od, oc, of = merge_dev(N, pv, pi, K, "exact")
    assert rc == 0, N.last_error()
    assert np.array_equal(oi, ei) and np.array_equal(od, ed) and np.array_equal(oc, ec) and np.array_equal(of, ef)
