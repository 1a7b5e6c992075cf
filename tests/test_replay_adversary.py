"""The inputs of test_gpu_replay_limits.py exhibit what they are built for -- checked on the CPU, against the
reference alone (the oracle's tables and answers, a heap walk over its distances), at every shape the GPU tests use."""
import numpy as np
import pytest

import replay_adversary as ra
from conftest import bits


def _target(oracle, c):
    dist = ra.distances(oracle, c.cents, c.idx, c.d, c.m, c.k, c.q)
    oi, od, oc = oracle.pq_batch_query(c.idx, c.d, c.k, c.cents, c.q.reshape(1, -1), c.K, c.frm, c.until)
    return dist, oi[0], od[0], oc[0]


def _smallest_distinct(stair, other):
    """the staircase holds the smallest pairwise-distinct distances: a row outside it that is not above all of them
    repeats one of its distances (and is counted by the heap walk like any row)"""
    assert len(np.unique(stair)) == len(stair)
    assert np.isin(other[other <= stair.max()], stair).all()
    assert (other <= stair.max()).sum() < len(stair) // 100


@pytest.mark.parametrize("name", list(ra.CASES))
def test_case_predicates(oracle, name):
    c = ra.case(oracle, name)
    dist, oi, od, oc = _target(oracle, c)
    rng_d = dist[c.frm:c.until]
    # the numpy distances are the oracle's, so the fast-path restatement of the GPU test stands on them
    assert oc == c.K
    assert np.array_equal(bits(np.sort(rng_d)[:c.K]), bits(np.sort(od)))
    # the input alone forces a tie: two bit-equal distances in the reference's answer
    assert len(np.unique(bits(od))) < c.K
    assert c.insertions == ra.insertions(rng_d, c.K)
    # the ordinary tied queries: every pair is two equal code rows inside the range, outside every staircase
    taken = set(c.positions.tolist()) | {c.until - 1}
    assert len(c.pairs) == ra.PAIRS
    for a, b in c.pairs:
        assert c.frm <= a < c.until and c.frm <= b < c.until and a != b and a not in taken and b not in taken
        assert np.array_equal(c.idx[:, a], c.idx[:, b])
    stair = dist[c.positions]
    other = np.ones(c.n, bool)
    other[c.positions] = False
    other[c.until - 1] = False
    if c.kind in ("stairs", "exact"):
        assert np.all(np.diff(stair) < 0)                            # strictly descending: every one of them inserts
        _smallest_distinct(stair, dist[other])
        assert c.insertions >= len(c.positions) + 1
    if name.startswith("late-"):
        assert 1200 < c.insertions <= ra.KEEP
        # rows that insert in each of the three levels of a handle that has not seen many flagged queries
        rel = c.positions - (c.frm // 64) * 64
        l01 = ra.L0_ROWS + 2048 * 64
        assert (rel < ra.L0_ROWS).sum() >= 20 and (rel >= l01).sum() >= 20
        assert ((rel >= ra.L0_ROWS) & (rel < l01)).sum() >= 1000
    if c.kind == "exact":
        assert c.insertions == ra.CASES[name][6]
    if name.startswith("overflow-"):
        assert c.insertions > ra.POOL
    if c.kind == "segments":
        per = ra.CASES[name][6]
        assert c.insertions <= 600
        half = np.sort(dist)[c.n // 2]
        assert dist[:ra.L0_ROWS].min() >= half                       # level 0's bound is loose
        assert len(c.positions) == 32 * per and 32 * per > ra.POOL
        for w in range(32):
            pos = c.positions[w * per:(w + 1) * per]
            lo = ra.L0_ROWS + w * ra.L1_SEG_ROWS
            assert lo <= pos[0] and pos[-1] < lo + ra.L1_SEG_ROWS
            assert np.all(np.diff(dist[pos]) < 0)
        first_kth = np.sort(stair[:per])[c.K - 1]
        assert stair[per:].min() > first_kth                         # no later staircase row inserts
        _smallest_distinct(stair, dist[other])                       # ... yet all lie below level 0's bound
    if c.kind == "shards":
        rg = ra.shard_ranges(c.n, 3)
        assert c.insertions <= 600
        assert c.extra["last_shard_insertions"] == ra.insertions(dist[rg[2][0]:], c.K)
        assert c.extra["last_shard_insertions"] > ra.POOL_SHARD
        assert c.positions[0] >= rg[2][0] and np.all(np.diff(stair) < 0)
        assert np.sort(dist[:rg[0][1]])[c.K - 1] < stair.min()       # shard 0 holds the smallest distances


@pytest.mark.parametrize("name,B", [("late-m16-K10", 8), ("late-m8-K63", 40), ("keep-l0-2048", 8)])
def test_batches_are_mixed_and_every_query_ties(oracle, name, B):
    c = ra.case(oracle, name)
    Q, targets, others = ra.batch(c, B)
    assert targets[0] == 0 and targets[-1] == B - 1 and 0 < targets[1] < B - 1 and len(others) == B - 3
    oi, od, oc = oracle.pq_batch_query(c.idx, c.d, c.k, c.cents, Q, c.K, c.frm, c.until)
    for p in others:                                                 # the decoded row and its duplicate: distance 0 twice
        a, b = c.pairs[others.index(p)]
        assert od[p, 0] == 0 and od[p, 1] == 0 and {a, b} <= set(oi[p].tolist())
    for p in targets:
        assert np.array_equal(bits(od[p]), bits(od[0])) and np.array_equal(oi[p], oi[0])


def test_insertions_is_the_literal_heap(oracle):
    """the heap walk counts what the oracle's TopKHeap does: an update that changes the heap"""
    rng = np.random.default_rng(5)
    dist = rng.integers(0, 50, 3000).astype(np.float32)              # many ties: equal to the root must not insert
    for K in (1, 2, 10, 63):
        h, count = oracle.TopKHeap(K), 0
        for r, v in enumerate(dist):
            h.update(r, float(v))
            count += r in h.raw()[0]
        assert ra.insertions(dist, K) == count
