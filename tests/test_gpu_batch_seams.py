"""What only a large batch reaches: the host loops that cut a batch into sub-batches (wide.hip, exact.hip, grouped.hip),
the batch sizes at which the wide filter hands over to the plain scan or its fallback changes form (wide_filter.hip),
and batches of more than 65 535 queries, whose number no longer fits the y extent of a grid.

Every case first asserts from batch_seams_ref.py (checked by hand in test_batch_seams_ref_host.py) that it crosses the
seam it is named after: two or more sub-batches, a ragged last one, the expected branch.  Then every answer is compared
bit for bit with the CPU oracle -- rows where no tie flag is set or the tie was replayed, by the suite's rule for
unreplayed ties otherwise.  Where the oracle over the whole batch would cost more than ORACLE_LOOK_UPS table look-ups
it answers the queries within 3 of a seam, the first and last one and 32 spread evenly; the others must equal, bit for
bit, what the same handle answers when asked in batches of at most one sub-batch (the count is printed).

The indexes are the smallest that cross each seam, which the sub-batch formulas make a matter of the code book (a
query's table is m * k * 4 bytes), not of the rows; scratch of 1 to 2 GiB per case follows from the seams themselves."""
import ctypes as C

import numpy as np
import pytest

import batch_seams_ref as S
from conftest import bits
from test_gpu_filter import tune          # noqa: F401  (the flat filter's small stage settings)
from test_gpu_grouped import _build, _oracle_side
from test_gpu_query import _same_up_to_ties

pytestmark = pytest.mark.gpu

ORACLE_LOOK_UPS = 10 ** 9
REPLAYED = 4                      # GULON_FLAG_REPLAYED
TIES = 3


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


# ---- comparing -----------------------------------------------------------------------------------------------------------

def _live(oc, K):
    return np.arange(K)[None, :] < oc[:, None]


def compare_flat(got, want):
    """A flat index's (rows, distances, counts, flags) against the oracle's (rows, distances, counts)."""
    oi, od, oc, of = got
    ei, ed, ec = want
    assert np.array_equal(oc, ec)
    live = _live(oc, oi.shape[1])
    assert np.array_equal(bits(od)[live], bits(ed)[:, :oi.shape[1]][live])
    settled = (of == 0) | ((of & REPLAYED) != 0)      # no tie, or the reference heap's order replayed
    assert np.array_equal(oi[settled][live[settled]], ei[:, :oi.shape[1]][settled][live[settled]])
    for q in np.flatnonzero(~settled):
        _same_up_to_ties(oi[q, :oc[q]], od[q, :oc[q]], ei[q, :ec[q]])


def compare_exact(got, want):
    """The exact index: every distance and count; every row of a query without a tie flag, and of a flagged one every
    row whose distance differs from both of its neighbours' (tests/test_gpu_exact.py)."""
    oi, od, oc, of = got
    ei, ed, ec = want
    K = oi.shape[1]
    ei, ed = ei[:, :K], ed[:, :K]
    assert np.array_equal(oc, ec)
    live = _live(oc, K)
    assert np.array_equal(bits(od)[live], bits(ed)[live])
    eq = (ed[:, 1:] == ed[:, :-1]) & live[:, 1:]
    apart = live.copy()
    apart[:, 1:] &= ~eq
    apart[:, :-1] &= ~eq
    need = np.where(((of & TIES) != 0)[:, None], apart, live)
    assert np.array_equal(oi[need], ei[need])
    assert (oi[~live] == -1).all() and np.isposinf(od[~live]).all()


def compare_grouped(got, want):
    """The grouped index runs the reference's heaps: rows, order, distances and counts."""
    oi, od, oc = got
    ei, ed, ec = want
    K = oi.shape[1]
    assert np.array_equal(oc, ec)
    live = _live(oc, K)
    assert np.array_equal(bits(od)[live], bits(ed[:, :K])[live])
    assert np.array_equal(oi[live], ei[:, :K][live])


def same_answers(a, b, rows):
    for x, y in zip(a, b):
        x, y = x[rows], y[rows]
        if x.dtype == np.float32:
            x, y = bits(x), bits(y)
        assert np.array_equal(x, y)


def seam_sample(B, sub, extra=()):
    """The queries the oracle answers when it cannot answer all: within 3 of a seam, the first and the last, 32 spread
    evenly, and the ones the case names."""
    sel = {0, B - 1, *extra, *np.linspace(0, B - 1, 32).astype(int).tolist()}
    for s in S.seams(B, sub):
        sel.update(q for q in range(s - 3, s + 4) if 0 <= q < B)
    return np.array(sorted(sel))


def verify(ask, oracle_ask, compare, Q, sub, look_ups_per_query, extra=(), skip_oracle=(), got=None):
    """ask(Q) -> the handle's raw answer; oracle_ask(Q) -> the oracle's.  Returns the handle's answer for the batch
    (`got`: the caller has it already)."""
    B = len(Q)
    got = ask(Q) if got is None else got
    whole = B * look_ups_per_query <= ORACLE_LOOK_UPS
    sel = np.arange(B) if whole else seam_sample(B, sub, extra)
    sel = np.setdiff1d(sel, np.asarray(skip_oracle, int))
    compare(tuple(a[sel] for a in got), oracle_ask(Q[sel]))
    rest = np.setdiff1d(np.arange(B), sel)
    if len(rest):
        print(f"{len(rest)} of {B} queries compared with the same handle asked in batches of {sub}, not with the oracle")
        parts = [ask(Q[a:a + sub]) for a in range(0, B, sub)]
        again = tuple(np.concatenate([p[j] for p in parts]) for j in range(len(got)))
        same_answers(got, again, rest)
    return got


# ---- flat indexes from explicit codes ---------------------------------------------------------------------------------------

class World:
    pass


def _world(seed, n, d, m, k):
    w = World()
    w.n, w.d, w.m, w.k = n, d, m, k
    w.rng = np.random.default_rng(seed)
    w.cents = w.rng.standard_normal(k * d).astype(np.float32)
    w.idx = w.rng.integers(0, k, (m, n)).astype(np.int32)
    return w


def _decode(w, code):
    from gulon_amd.vectors import subvector_bounds
    fr, un = subvector_bounds(w.d, w.m)
    out = np.zeros(w.d, np.float32)
    for j in range(w.m):
        s = un[j] - fr[j]
        out[fr[j]:un[j]] = w.cents[w.k * fr[j] + code[j] * s: w.k * fr[j] + (code[j] + 1) * s]
    return out


def _index(g, w):
    pq = g.ProductQuantizer.from_flat(w.k, w.d, w.m, w.cents)
    coder = pq.coder_factory(w.n)
    enc = g.EncodedMatrix(coder, [coder.build_code(np.ascontiguousarray(w.idx[j])) for j in range(w.m)])
    return g.PQIndex(pq, enc)


def _set(ix, **knobs):
    from gulon_amd import native as N
    for key, v in knobs.items():
        N.check(N.lib().gulon_index_tuning(ix._h, key.encode(), int(v)))


def _filter_stats(ix):
    from gulon_amd import native as N
    t, r = C.c_int32(-1), C.c_int32(-1)
    N.check(N.lib().gulon_index_filter_stats(ix._h, C.byref(t), C.byref(r)))
    return t.value, r.value


def _flat_look_ups(w):
    """Per query: its table (m * k entries, built from d coordinates) and one look-up per row and quantizer."""
    return w.m * w.k + w.n * w.m


def _verify_flat(oracle, ix, w, Q, K, sub, extra=()):
    return verify(lambda q: ix.batch_query_raw(K, q), lambda q: oracle.pq_batch_query(w.idx, w.d, w.k, w.cents, q, K),
                  compare_flat, Q, sub, _flat_look_ups(w), extra)


# ---- 1. run_wide_query's sub-batch loops -------------------------------------------------------------------------------------

WIDE = {            # form: (k, n, B) at m = 2, d = 4
    "lds": (16384, 200, 8192 + 5),
    "gathered": (65536, 200, 2048 + 5),
    "sliced": (32768, 262144 - 64, 1024 + 5),     # (one row block short of what the wide filter takes by default)
}
N_TIED = 600


@pytest.fixture(scope="module")
def wide_worlds(g):
    made = {}

    def get(form):
        if form not in made:
            k, n, B = WIDE[form]
            w = _world(sorted(WIDE).index(form) + 900, n, 4, 2, k)
            w.B = B
            w.sub = S.wide_sub_batch(B, w.m, k, S.ceil_div(n, 64) * 64)
            w.Q = w.rng.standard_normal((B, w.d)).astype(np.float32)
            w.tied = np.zeros(0, int)
            if form == "gathered":
                # rows 100..149 repeat rows 0..49; 600 queries sit on those rows, on both sides of the seam
                w.idx[:, 100:150] = w.idx[:, :50]
                w.tied = np.r_[np.arange(0, 3 * (N_TIED - 5), 3), np.arange(w.sub, w.sub + 5)]
                for t, q in enumerate(w.tied):
                    w.Q[q] = _decode(w, w.idx[:, t % 50])
            if form == "sliced":
                # the neighbours of the queries around the seam sit in the last row block, three rows each
                w.planted = np.arange(w.sub - 2, w.sub + 3)
                for t, q in enumerate(w.planted):
                    code = w.rng.integers(0, k, w.m)
                    w.Q[q] = _decode(w, code)
                    rows = n - 64 + 12 * t + np.arange(3)
                    w.idx[:, rows] = code[:, None]
                    w.idx[1, rows[1:]] = (code[1] + np.arange(1, 3)) % k
            w.ix = _index(g, w)
            made[form] = w
        return made[form]

    yield get
    for w in made.values():
        w.ix.close()


@pytest.mark.parametrize("K", [10, 70])
@pytest.mark.parametrize("form", list(WIDE))
def test_wide_scan_in_sub_batches(oracle, g, wide_worlds, form, K):
    """run_wide_query cuts the batch where its fp32 tables (sliced: its parked sums) pass 1 GiB: the q0 offsets of the
    tables, of the merge's outputs (K = 10) and of the peel's bounds and lists (K = 70), the parked sums reused per
    sub-batch, and one tie replay over the whole batch afterwards -- in two rounds for the gathered form, whose 600 tied
    queries are more than the 512 tables of 512 KiB a round holds."""
    w = wide_worlds(form)
    k, n, B = WIDE[form]
    assert S.wide_form(w.m, k) == form
    cuts = S.sub_batches(B, w.sub)
    assert len(cuts) == 2 and cuts[1] == (w.sub, 5) and w.sub == {"lds": 8192, "gathered": 2048, "sliced": 1024}[form]
    assert not S.wide_filter_eligible(B, K, w.m, k, S.ceil_div(n, 64))        # the plain scan, not the filter
    oi, od, oc, of = _verify_flat(oracle, w.ix, w, w.Q, K, w.sub, extra=tuple(w.tied))
    assert _filter_stats(w.ix)[0] == 0
    assert (oc == K).all()
    if form == "gathered":
        per_round = S.wide_replay_round(B, w.m, k)
        assert per_round == 512 < N_TIED == len(w.tied) and (w.tied < w.sub).sum() > per_round > (w.tied >= w.sub).sum() > 0
        assert ((of[w.tied] & TIES) != 0).all()
        # K <= 63: every tied query of both rounds was replayed; K > 63 has no replay
        assert ((of[w.tied] & REPLAYED) != 0).all() == (K <= S.MAX_K) and ((of & REPLAYED) != 0).any() == (K <= S.MAX_K)
    if form == "sliced":
        assert (oi[w.planted, 0] >= n - 64).all() and (od[w.planted, 0] == 0).all()


# ---- 2. where the wide filter hands over -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def handover(oracle, g):
    w = _world(77, 2048, 4, 2, 16384)
    w.Q = w.rng.standard_normal((8193, w.d)).astype(np.float32)
    w.K = 10
    w.want = oracle.pq_batch_query(w.idx, w.d, w.k, w.cents, w.Q, w.K)
    w.ix = _index(g, w)
    _set(w.ix, GULON_FILTER_MIN_RB=4, GULON_FILTER_CAP=1024)
    yield w
    w.ix.close()


@pytest.mark.parametrize("B,filtered", [(8192, True), (8193, False)])
def test_wide_filter_hands_over_at_one_gib_of_tables(oracle, g, handover, B, filtered):
    """B * m * k * 4 = 2^30 at B = 8192: the last batch the wide filter takes, and the first it leaves to
    run_wide_query (there a second sub-batch of one query)."""
    w = handover
    assert S.wide_filter_eligible(B, w.K, w.m, w.k, w.n // 64, min_rb=4) == filtered
    assert S.wide_sub_batch(B, w.m, w.k, w.n) == 8192 and S.wide_range_form(B, w.m, w.k, w.n // 64) == "lds"
    got = w.ix.batch_query_raw(w.K, w.Q[:B])
    assert _filter_stats(w.ix)[0] == (B if filtered else 0)
    compare_flat(got, tuple(a[:B] for a in w.want))


def test_wide_filter_fallback_gathers_above_256_mib_of_parked_sums(oracle, g):
    """70 queries over 2^20 rows of a sliced index: the filter's sample scan parks its sums (sliced), its fallback over
    every row would park 280 MiB and gathers through L2 instead.  Four queries sit on 3000 copies of their own code row
    each, scattered over the index: all of them pass any bound, the survivor queues (16 of 64 entries per query at the
    smallest GULON_FILTER_CAP) overflow, and those queries fall back."""
    w = _world(78, 1 << 20, 4, 2, 32768)
    B, K, rb = 70, 10, (1 << 20) // 64
    assert S.wide_filter_eligible(B, K, w.m, w.k, rb) and S.wf_slice(w.m, w.k) < w.m
    assert S.wide_range_form(B, w.m, w.k, S.wide_filter_sample_blocks(rb)) == "sliced"
    assert S.wide_range_form(B, w.m, w.k, rb) == "gathered" and S.wide_range_form(64, w.m, w.k, rb) == "sliced"
    Q = w.rng.standard_normal((B, w.d)).astype(np.float32)
    crowded = [0, 33, 68, 69]
    spots = w.rng.permutation(w.n)[:3000 * len(crowded)].reshape(len(crowded), 3000)
    for q, rows in zip(crowded, spots):
        code = w.rng.integers(0, w.k, w.m)
        w.idx[:, rows] = code[:, None]
        Q[q] = _decode(w, code)
    ix = _index(g, w)
    _set(ix, GULON_FILTER_CAP=64)
    oi, od, oc, of = _verify_flat(oracle, ix, w, Q, K, B)
    tiles, redone = _filter_stats(ix)
    print(f"wide filter: {tiles} query tiles, {redone} redone by the gathered scan")
    assert tiles == B and redone >= len(crowded)
    assert (od[crowded] == 0).all() and ((of[crowded] & TIES) != 0).all()
    ix.close()


# ---- 3. the exact index's one-pass path --------------------------------------------------------------------------------------

def _exact_ask(ix, K):
    return lambda q: ix.batch_query_raw(K, q)


@pytest.mark.parametrize("K", [64, 1000])
def test_exact_one_pass_unsampled_in_sub_batches(oracle, g, K):
    """Queues of 2^22 entries: 32 queries fill the 1 GiB of scratch, the 40-query batch takes two sub-batches."""
    n, d, cap = 300, 8, 1 << 22
    rng = np.random.default_rng(31)
    X = rng.standard_normal((n, d)).astype(np.float32)
    sub = S.exact_sub_batch(40, K, n, cap)
    B = sub + 8
    assert sub == 32 and S.exact_sample(K, n, cap) == 0 and S.sub_batches(B, S.exact_sub_batch(B, K, n, cap)) == [(0, 32), (32, 8)]
    Q = rng.standard_normal((B, d)).astype(np.float32)
    ix = g.ExactIndex(g.DeviceMatrix.from_host(X))
    ix.tune(GULON_EXACT_QUEUE_CAP=cap)
    got = verify(_exact_ask(ix, K), lambda q: oracle.exact_knn(X, q, K), compare_exact, Q, sub, n * d)
    s = ix.stats()
    assert (s["one_pass"], s["fallback"], s["nonfinite"], s["sample"], s["capacity"]) == (B, 0, 0, 0, cap)
    assert (got[2] == min(K, n)).all()
    ix.close()


@pytest.mark.parametrize("K", [64, 1000])
def test_exact_one_pass_sampled_in_sub_batches(oracle, g, K):
    """Every row sampled (GULON_EXACT_SAMPLE) and queues of 2048 entries: 176 384 bytes of scratch per query, 6080 queries
    per sub-batch.  On each side of the seam one query sits on 2100 identical rows -- all at its bound, so its queue
    overflows and the peeled fallback answers it -- one holds a NaN and the rest are ordinary: the per-query counters
    at q0, the queue and sample buffers reused, and the fallback's answers scattered across the seam.  The NaN queries'
    answers are held against the handle asked for each alone (the contract of test_non_finite_queries_are_answered_alone);
    the oracle answers the others, under the cost cap."""
    n, d, cap, dups = 40000, 4, 2048, 2100
    rng = np.random.default_rng(32)
    X = rng.standard_normal((n, d)).astype(np.float32)
    far = np.full(d, 10.0, np.float32)                     # far outside the cloud: no other query's bound reaches it
    X[1000:1000 + dups] = far
    sub = S.exact_sub_batch(1 << 20, K, n, cap, knob_sample=n)
    B = sub + 8
    assert sub == 6080 and S.exact_sample(K, n, cap, n) == n > cap
    assert S.sub_batches(B, S.exact_sub_batch(B, K, n, cap, n)) == [(0, 6080), (6080, 8)]
    Q = rng.standard_normal((B, d)).astype(np.float32)
    overflowing, nan, ordinary = [5, sub + 3], [7, sub + 5], [6, sub + 4]
    Q[overflowing] = far
    Q[nan, 2] = np.nan
    ix = g.ExactIndex(g.DeviceMatrix.from_host(X))
    ix.tune(GULON_EXACT_QUEUE_CAP=cap, GULON_EXACT_SAMPLE=n)
    got = ix.batch_query_raw(K, Q)
    s = ix.stats()                                        # (of the last batch: before verify asks again)
    verify(_exact_ask(ix, K), lambda q: oracle.exact_knn(X, q, K), compare_exact, Q, sub, n * d,
           extra=overflowing + ordinary, skip_oracle=nan, got=got)
    assert (s["fallback"], s["nonfinite"], s["one_pass"]) == (2, 2, B - 4) and (s["sample"], s["capacity"]) == (n, cap)
    assert s["max_fill"] >= dups
    assert ((got[3][overflowing] & TIES) != 0).all() and (got[1][overflowing, 0] == 0).all()
    for q in nan:
        same_answers(tuple(a[q:q + 1] for a in got), ix.batch_query_raw(K, Q[q:q + 1]), slice(None))
    ix.close()


# ---- 4. the grouped index at k_nn > 63 -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,groups,strategy,limit,K", [(3000, 64, 1, 1500, 2048), (8000, 2048, 0, 2048, 1024)])
def test_grouped_big_k_in_sub_batches(oracle, g, n, groups, strategy, limit, K):
    """run_grouped_query calls itself on sub-batches that keep the per-group heaps under 2^28 entries: the offsets of
    the queries, of every output and of the counts, which come back for every query."""
    d, m, k = 8, 2, 16
    X, dm, coarse, gv, pq = _build(oracle, g, n, d, groups, m, k, seed=n + K, iters=2)
    R, cents, offsets = _oracle_side(oracle, X, coarse, gv, pq, n)
    ng = len(cents)
    sub = S.grouped_big_k_sub(1 << 20, K, ng, strategy, limit)
    B = sub + 3
    assert S.sub_batches(B, S.grouped_big_k_sub(B, K, ng, strategy, limit)) == [(0, sub), (sub, 3)]
    assert sub == (1 << 28) // (ng * K) and ng > groups // 2
    index = g.Index.grouped(gv, pq, g.LimitVectors(limit) if strategy else g.LimitGroups(limit))
    codes = index.data.indices()
    rng = np.random.default_rng(4)
    Q = (X[rng.integers(0, n, B)] + 0.1 * rng.standard_normal((B, d))).astype(np.float32)
    oi, od, oc = verify(lambda q: index.batch_query_raw(K, q),
                        lambda q: oracle.grouped_query(codes, d, k, pq.flat_centroids(), cents, offsets, q, K, strategy, limit),
                        compare_grouped, Q, sub, n * m + ng * d)
    assert len(oc) == B and (oc >= min(K, limit if strategy else K)).all() and (oc <= K).all()
    index.close()


# ---- 5. more queries than a grid's y extent ---------------------------------------------------------------------------------

B_BIG = 65537
STEP = 4096                       # "one sub-batch" where the path itself has none


def _queries(rng, X, B):
    return (X[rng.integers(0, len(X), B)] + 0.05 * rng.standard_normal((B, X.shape[1]))).astype(np.float32)


@pytest.mark.parametrize("filt", [1, 0])
def test_65537_queries_flat_byte_codes(oracle, g, tune, filt):
    w = _world(61, 8192, 8, 4, 16)
    assert B_BIG > S.GRID_Y_MAX
    Q = w.rng.standard_normal((B_BIG, w.d)).astype(np.float32)
    ix = _index(g, w)
    _set(ix, GULON_SCAN_FILTER=filt)
    _verify_flat(oracle, ix, w, Q, 10, STEP)
    assert (_filter_stats(ix)[0] > 0) == bool(filt)
    ix.close()


def test_65537_queries_wide_filter(oracle, g):
    """wf_table_mins takes the query from the y extent of its grid."""
    w = _world(62, 2048, 4, 2, 1024)
    K = 10
    assert S.wide_filter_eligible(B_BIG, K, w.m, w.k, w.n // 64, min_rb=4) and B_BIG > S.GRID_Y_MAX
    Q = w.rng.standard_normal((B_BIG, w.d)).astype(np.float32)
    ix = _index(g, w)
    _set(ix, GULON_FILTER_MIN_RB=4, GULON_FILTER_CAP=1024)
    _verify_flat(oracle, ix, w, Q, K, STEP)
    ix.close()
    # (the handle's last batch was one of verify's or the whole one: both are filtered batches)


def test_65537_queries_grouped(oracle, g):
    """by_group_applies refuses the batch; the pre-selection taken instead builds its tables on a (m_pad, B) grid."""
    n, d, groups, m, k, K = 400, 8, 8, 2, 16, 3
    X, dm, coarse, gv, pq = _build(oracle, g, n, d, groups, m, k, seed=63)
    R, cents, offsets = _oracle_side(oracle, X, coarse, gv, pq, n)
    assert not S.by_group_takes_batch(B_BIG, 8, len(cents))
    index = g.Index.grouped(gv, pq, g.LimitGroups(2))
    codes = index.data.indices()
    Q = _queries(np.random.default_rng(5), X, B_BIG)
    oi, od, oc = verify(lambda q: index.batch_query_raw(K, q),
                        lambda q: oracle.grouped_query(codes, d, k, pq.flat_centroids(), cents, offsets, q, K, 0, 2),
                        compare_grouped, Q, STEP, n * m + len(cents) * d)
    assert len(oc) == B_BIG
    index.close()


@pytest.mark.parametrize("K", [3, 64])
def test_65537_queries_exact(oracle, g, K):
    """K = 64: 17 sub-batches of 4096 at the default capacity, the last of one query."""
    n, d = 300, 8
    rng = np.random.default_rng(64)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = _queries(rng, X, B_BIG)
    sub = S.exact_sub_batch(B_BIG, K, n)
    assert sub == 4096 and S.sub_batches(B_BIG, sub)[-1] == (65536, 1)
    ix = g.ExactIndex(g.DeviceMatrix.from_host(X))
    verify(_exact_ask(ix, K), lambda q: oracle.exact_knn(X, q, K), compare_exact, Q, sub, n * d)
    s = ix.stats()
    assert s["one_pass"] + s["fallback"] == B_BIG and s["nonfinite"] == 0
    ix.close()
