"""The tie replay (replay.hip) at its limits: rows that insert late into the reference's TopKHeap, the keep list of
2 048 insertions, candidate pools that overflow (8 192 per query, 2 048 per shard), more flagged queries than one
round, the road through the quantized filter -- on the inputs of replay_adversary.py (their CPU predicates:
test_replay_adversary.py).  The reference is the C oracle's literal heap, bit for bit (TopKHeap.scala:57-79).

The contract, for every query of every batch (_contract): count and distance bits are the oracle's, and then
  (a) no tie flag, or GULON_FLAG_EXACT_REPLAY: the rows are the oracle's, as a list;
  (b) tie flags without GULON_FLAG_EXACT_REPLAY: the rows are the fast path's -- the (distance, row id) order of the
      oracle's distances over the range, cut by row id -- untouched.
Every batch is mixed: the target query at both ends and in the middle, ordinary tied queries (a decoded row that has
one duplicate) between its copies; those must come back replayed whatever happens to the target next to them."""
import re

import numpy as np
import pytest

import replay_adversary as ra
from conftest import bits

pytestmark = pytest.mark.gpu

TIE, REPLAYED = 3, 4


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def _index_parts(g, c):
    pq = g.ProductQuantizer.from_flat(c.k, c.d, c.m, c.cents)
    coder = pq.coder_factory(c.n)
    return pq, g.EncodedMatrix(coder, [coder.build_code(c.idx[j]) for j in range(c.m)])


def _index(g, c):
    return g.PQIndex(*_index_parts(g, c))


def _contract(oracle, c, Q, res, exp, expect):
    """expect[q]: 'replayed' (tie flags and EXACT_REPLAY), 'untouched' (tie flags, branch (b)) or None (either form)"""
    ri, rd, rc, rf = res
    oi, od, oc = exp
    assert np.array_equal(rc, oc)
    assert np.array_equal(bits(rd), bits(od))
    for q in range(len(Q)):
        if rf[q] == 0 or rf[q] & REPLAYED:
            branch = "replayed" if rf[q] & TIE else "unflagged"
            assert ri[q, :oc[q]].tolist() == oi[q, :oc[q]].tolist(), (q, rf[q])
        else:
            branch = "untouched"
            assert rf[q] & TIE, (q, rf[q])
            dist = ra.distances(oracle, c.cents, c.idx, c.d, c.m, c.k, Q[q])[c.frm:c.until]
            fast = c.frm + ra.fast_path_rows(dist, c.K)
            assert np.array_equal(bits(dist[fast - c.frm]), bits(od[q]))
            assert ri[q].tolist() == fast.tolist(), q
        if expect[q] is not None:
            assert branch == expect[q], (q, int(rf[q]), branch, expect[q])


def _run(oracle, g, c, B, target, runs=1, later=None, ix=None):
    """the mixed batch `runs` times on one handle; the targets must take branch `target` in the first run and `later`
    in the following ones, the ordinary tied queries are replayed every time"""
    Q, targets, others = ra.batch(c, B)
    exp = oracle.pq_batch_query(c.idx, c.d, c.k, c.cents, Q, c.K, c.frm, c.until)
    own = ix is None
    ix = _index(g, c) if own else ix
    out = []
    for run in range(runs):
        res = ix.batch_query_raw(c.K, Q, c.frm, c.until)
        expect = ["replayed"] * B
        for t in targets:
            expect[t] = target if run == 0 else later
        _contract(oracle, c, Q, res, exp, expect)
        out.append(res)
    if own:
        ix.close()
    return out


@pytest.mark.parametrize("name", ra.LATE_CASES)
def test_late_insertions_are_replayed(oracle, g, name):
    """1 500 staircase rows over the three levels: 1 500 to 1 800 insertions, most of them in rows that a segment
    seeded from an earlier level has to let through.  4-byte, 16-byte and two-word codes, K = 2, 10, 63, a sub-range."""
    _run(oracle, g, ra.case(oracle, name), 8, "replayed")


@pytest.mark.parametrize("name", ["late-m16-K10", "late-m8-K63", "late-m32-K2", "late-m8range-K10"])
def test_late_insertions_on_the_filtered_road(oracle, g, name):
    """40 flagged queries, twice on one handle: the second batch has a level 0 four times as long and levels 1 and 2
    behind the quantized filter (rp_prefix_pool gives the long level's bound).  Same answers, all replayed."""
    a, b = _run(oracle, g, ra.case(oracle, name), 40, "replayed", runs=2, later="replayed")
    assert ((a[3] & TIE) != 0).sum() >= 32
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("name,target", [("keep-l0-2048", "replayed"), ("keep-l0-2049", "untouched"),
                                         ("keep-3l-2048", "replayed"), ("keep-3l-2049", "untouched")])
def test_both_sides_of_the_keep_limit(oracle, g, name, target):
    """rp_heap keeps 2 048 inserting rows: exactly that many are replayed, one more leaves the result untouched --
    in level 0 alone (n = 4 096) and across the levels."""
    c = ra.case(oracle, name)
    assert c.insertions == (ra.KEEP if target == "replayed" else ra.KEEP + 1)
    _run(oracle, g, c, 8, target)


@pytest.mark.parametrize("name", ["overflow-m16", "overflow-w1024"])
def test_pool_overflow_by_insertions(oracle, g, name):
    """9 000 inserting rows: the target's pool overflows, its result stays the fast path's; the queries next to it in
    the pack are replayed.  A second batch on the handle: each answer is one of the two forms."""
    c = ra.case(oracle, name)
    assert c.insertions > ra.POOL
    _run(oracle, g, c, 8, "untouched", runs=2, later=None)


def test_pool_overflow_with_few_insertions(oracle, g, monkeypatch, capfd):
    """32 level-1 segments with a staircase of 300 rows each, all below level 0's bound, only the first below the
    reference's: 400 insertions, 9 600 candidates on a handle that has not seen many flagged queries."""
    c = ra.case(oracle, "segments-m8")
    assert c.insertions <= 600
    monkeypatch.setenv("GULON_REPLAY_STATS", "1")
    ix = _index(g, c)
    capfd.readouterr()
    _, targets, _ = ra.batch(c, 8)
    failure = None
    try:
        _run(oracle, g, c, 8, "untouched", ix=ix)
    except AssertionError as e:
        failure = e
    err = capfd.readouterr().err
    lines = re.findall(r"\[replay\] (\d+) flagged queries;[^\n]*candidates:((?: \d+)+)", err)
    assert lines, err
    flagged, counts = int(lines[0][0]), [int(x) for x in lines[0][1].split()]
    assert flagged == 8 and len(counts) == 8, lines            # every query of the batch is flagged: list order = batch order
    print("candidates per flagged query:", counts)
    assert all(counts[t] > ra.POOL for t in targets), (
        f"the target has {[counts[t] for t in targets]} candidates, not more than {ra.POOL}: the level geometry of "
        "the replay changed and replay_adversary.segment_stairs has to follow it")
    if failure is not None:
        raise failure
    monkeypatch.delenv("GULON_REPLAY_STATS")
    _run(oracle, g, c, 8, None, ix=ix)
    ix.close()


def test_late_insertions_wide_codes(oracle, g):
    """case 1 over 10-bit codes (k = 1 024): rp_scan_wide, no shortcut, no filter"""
    _run(oracle, g, ra.case(oracle, "late-w1024"), 8, "replayed")


def test_second_round_byte_codes(oracle, g):
    """B = 1 100 tied queries: the replay's rounds hold 1 024, the second one has 76 queries to do"""
    n, d, m, k, K, B = 6000, 16, 4, 4, 10, 1100
    rng = np.random.default_rng(99)
    cents = rng.standard_normal(k * d).astype(np.float32)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    Q = np.random.default_rng(3).standard_normal((B, d)).astype(np.float32)
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    coder = pq.coder_factory(n)
    ix = g.PQIndex(pq, g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(m)]))
    oi, od, oc = oracle.pq_batch_query(idx, d, k, cents, Q, K)
    for _ in range(2):                                           # (the second batch: the handle has seen many flagged queries)
        ri, rd, rc, rf = ix.batch_query_raw(K, Q)
        assert ((rf & TIE) != 0).all() and ((rf & REPLAYED) != 0).all()
        assert np.array_equal(rc, oc) and np.array_equal(bits(rd), bits(od)) and np.array_equal(ri, oi)
    ix.close()


def test_second_round_wide_codes(oracle, g):
    """k = 65 536, m = 16: a flagged query's table is 4 MiB, a round holds 64 of them; 70 tied queries"""
    n, d, m, k, K, B, dup = 3000, 16, 16, 65536, 10, 70, 1500
    rng = np.random.default_rng(7)
    cents = rng.standard_normal(k * d).astype(np.float32)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    idx[:, -dup:] = idx[:, :dup]
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    coder = pq.coder_factory(n)
    ix = g.PQIndex(pq, g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(m)]))
    Q = np.stack([ix.decode(r) for r in range(0, dup, dup // B)][:B]).astype(np.float32)
    oi, od, oc = oracle.pq_batch_query(idx, d, k, cents, Q, K)
    ri, rd, rc, rf = ix.batch_query_raw(K, Q)
    assert ((rf & TIE) != 0).all() and ((rf & REPLAYED) != 0).all()
    assert np.array_equal(rc, oc) and np.array_equal(bits(rd), bits(od)) and np.array_equal(ri, oi)
    ix.close()


def _sharded(oracle, g, c, B, target):
    from gulon_amd.sharded import NodeShardedIndex
    Q, targets, others = ra.batch(c, B)
    exp = oracle.pq_batch_query(c.idx, c.d, c.k, c.cents, Q, c.K)
    sx = NodeShardedIndex(*_index_parts(g, c), [0, 0, 0])
    res = sx.batch_query_raw(c.K, Q)
    info = sx.info()
    sx.close()
    expect = ["replayed"] * B
    for t in targets:
        expect[t] = target
    _contract(oracle, c, Q, res, exp, expect)
    return Q, res, info


def test_sharded_late_insertions_equal_unsharded(oracle, g):
    """three shards of one device: each starts cold at its first row, the candidates of all three are replayed together"""
    c = ra.case(oracle, "late-m16-K10")
    Q, res, info = _sharded(oracle, g, c, 8, "replayed")
    ix = _index(g, c)
    full = ix.batch_query_raw(c.K, Q)
    ix.close()
    assert np.array_equal(res[0], full[0]) and np.array_equal(bits(res[1]), bits(full[1]))
    assert np.array_equal(res[2], full[2]) and np.array_equal(res[3], full[3])


def test_sharded_pool_overflow_in_one_shard(oracle, g):
    """113 insertions over the whole index, 2 134 for a heap that starts cold at the last shard's first row: that
    shard's pool of 2 048 overflows, the target stays untouched, the queries next to it are replayed"""
    c = ra.case(oracle, "shard-local-m16")
    assert c.insertions <= 600 and c.extra["last_shard_insertions"] > ra.POOL_SHARD
    _sharded(oracle, g, c, 8, "untouched")


def test_sharded_more_flagged_queries_than_the_first_round(oracle, g):
    """40 flagged queries: the first exchange holds 16, the next one the other 24"""
    Q, res, info = _sharded(oracle, g, ra.case(oracle, "late-m16-K10"), 40, "replayed")
    assert info["last_flagged_queries"] == 40 and info["last_replay_rounds"] == 2
