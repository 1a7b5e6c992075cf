"""tests/merge_ref.py against plain Python: merge_final equals sorted() over tuples, peeled_rounds equals the plain sort
on the tie shapes the GPU tests use (in miniature), and make_lists returns what the merge kernels assume.  No GPU."""
import numpy as np
import pytest

import merge_ref as mr
from conftest import bits

INT_MAX = mr.INT_MAX


def _sorted_reference(pv, pi, K):
    """Per query: sorted() over (distance value, id, bit pattern) tuples of the non-padding entries."""
    lists, B, keff = pv.shape
    out = []
    for q in range(B):
        ent = []
        for l in range(lists):
            for e in range(keff):
                if int(pi[l, q, e]) != INT_MAX:
                    ent.append((float(pv[l, q, e]) + 0.0, int(pi[l, q, e]), int(bits(pv[l, q, e:e + 1])[0])))
        ent = sorted(ent)
        idx = [e[1] for e in ent[:K]] + [-1] * (K - min(K, len(ent)))
        dbits = [e[2] for e in ent[:K]] + [0x7F800000] * (K - min(K, len(ent)))
        flags = 0
        for e in range(K):
            if e + 1 < len(ent) and ent[e][0] == ent[e + 1][0]:
                flags |= 1 if e == K - 1 else 2
        out.append((idx, dbits, min(K, len(ent)), flags))
    return out


@pytest.mark.parametrize("regime", mr.REGIMES)
@pytest.mark.parametrize("lists,B,K", [(1, 3, 1), (3, 6, 2), (2, 7, 5), (5, 6, 9)])
def test_merge_final_equals_python_sorted(regime, lists, B, K):
    pv, pi = mr.make_lists(np.random.default_rng(lists * 100 + K), lists, B, K, regime)
    oi, od, oc, of = mr.merge_final(pv, pi, K)
    assert oi.shape == od.shape == (B, K) and oi.dtype == np.int32 and od.dtype == np.float32
    for q, (idx, dbits, count, flags) in enumerate(_sorted_reference(pv, pi, K)):
        assert oi[q].tolist() == idx and bits(od[q]).tolist() == dbits
        assert oc[q] == count and of[q] == flags and of[q] & 4 == 0


def test_merge_final_keeps_bit_patterns_and_breaks_zero_ties_by_id():
    pv = np.array([[[-0.0, 0.0, np.inf]], [[0.0, -0.0, np.inf]]], np.float32)
    pi = np.array([[[4, 9, INT_MAX]], [[2, 6, INT_MAX]]], np.int32)
    oi, od, oc, of = mr.merge_final(pv, pi, 2)
    assert oi.tolist() == [[2, 4]] and bits(od).tolist() == [[0x00000000, 0x80000000]]
    assert oc.tolist() == [2] and of.tolist() == [3]


def test_real_inf_entry_sorts_before_padding_and_padding_is_dropped():
    pv = np.array([[[1.0, np.inf, np.inf]], [[np.inf, np.inf, np.inf]]], np.float32)
    pi = np.array([[[8, 3, INT_MAX]], [[1, INT_MAX, INT_MAX]]], np.int32)
    oi, od, oc, of = mr.merge_final(pv, pi, 2)
    assert oi.tolist() == [[8, 1]] and np.isposinf(od[0, 1]) and oc.tolist() == [2]
    assert of.tolist() == [1]                                   # (inf, 1) and (inf, 3): the boundary pair
    oi, od, oc, of = mr.merge_final(np.full((2, 1, 4), np.inf, np.float32), np.full((2, 1, 4), INT_MAX, np.int32), 3)
    assert oi.tolist() == [[-1, -1, -1]] and np.isposinf(od).all() and oc.tolist() == [0] and of.tolist() == [0]


# ---- the peel -----------------------------------------------------------------------------------------------------------

def _plain(dist, rows, K):
    o = np.lexsort((rows, dist))
    return mr.finalize(rows[o][:K + 1], dist[o][:K + 1], K), (rows[o], dist[o])


def _peel_case(name):
    rng = np.random.default_rng(5)
    if name == "group across a round boundary":           # 40 untied rows, then 50 equal ones over entries 63/64
        n, K = 300, 100
        dist = (1000 + rng.permutation(n)).astype(np.float32)
        dist[rng.permutation(n)[:40]] = np.arange(40, dtype=np.float32)
        far = np.flatnonzero(dist >= 1000)
        dist[far[rng.permutation(len(far))[:50]]] = 500.0
    elif name == "group longer than a round":              # 150 equal rows first: rounds 2 and 3 start inside it
        n, K = 400, 130
        dist = (1000 + rng.permutation(n)).astype(np.float32)
        dist[rng.permutation(n)[:150]] = 7.0
    elif name == "fewer rows than K":
        n, K = 100, 200
        dist = rng.choice(np.asarray([1.0, 2.0, 3.0], np.float32), n)
    else:                                                   # every distance equal, K on both sides of n
        n, K = 150, {"all equal": 100, "all equal, K > n": 190}[name]
        dist = np.full(n, 2.5, np.float32)
    rows = rng.permutation(n).astype(np.int64) + 1000      # not in id order: only the comparison orders them
    return dist, rows, K


@pytest.mark.parametrize("name", ["group across a round boundary", "group longer than a round", "fewer rows than K",
                                  "all equal", "all equal, K > n"])
def test_peeled_rounds_equal_the_plain_sort(name):
    dist, rows, K = _peel_case(name)
    (ei, ed, ec, ef), (srows, sdist) = _plain(dist, rows, K)
    if name == "group across a round boundary":
        assert sdist[63] == sdist[64] and sdist[62] == sdist[65] and ef & 2
    if name == "group longer than a round":
        assert sdist[0] == sdist[63] == sdist[64] == sdist[128] and len(set(sdist[:131].tolist())) == 1
    ids, pd = mr.peeled_rounds(dist, rows, K)
    rounds = -(-(K + 1) // 64)
    assert len(ids) == len(pd) == rounds * 64
    live = min(len(rows), rounds * 64)
    assert ids[:live].tolist() == srows[:live].tolist() and bits(pd[:live]).tolist() == bits(sdist[:live]).tolist()
    assert (ids[live:] == INT_MAX).all() and np.isposinf(pd[live:]).all()
    oi, od, oc, of = mr.peel_final(ids, pd, K)
    assert oi.tolist() == ei.tolist() and bits(od).tolist() == bits(ed).tolist() and (oc, of) == (ec, ef)
    if len(rows) < K:
        assert oc == len(rows) and (oi[oc:] == -1).all() and np.isposinf(od[oc:]).all()
    pv, pi = mr.peel_partial(ids, pd, K)
    assert len(pv) == len(pi) == K + 1
    assert pi[:min(K + 1, len(rows))].tolist() == srows[:K + 1].tolist()
    assert (pi[len(rows):] == INT_MAX).all()


def test_peeled_rounds_on_inf_distances_go_by_row_id():
    rows = np.random.default_rng(2).permutation(200).astype(np.int64)
    ids, pd = mr.peeled_rounds(np.full(200, np.inf, np.float32), rows, 100)
    assert ids.tolist() == list(range(128)) and np.isposinf(pd).all()
    assert mr.peel_final(ids, pd, 100)[2:] == (100, 3)


# ---- the generator --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("regime", mr.REGIMES)
@pytest.mark.parametrize("lists,B,K", [(1, 4, 1), (3, 6, 2), (4, 9, 7), (2, 3, 64), (5, 6, 70)])
def test_make_lists_meet_the_precondition(regime, lists, B, K):
    pv, pi = mr.make_lists(np.random.default_rng(K), lists, B, K, regime)
    assert pv.shape == pi.shape == (lists, B, K + 1) and pv.dtype == np.float32 and pi.dtype == np.int32
    mr.check_precondition(pv, pi)
    live = (pi != INT_MAX).sum(axis=(0, 2))
    if regime == "ties" and lists > 1 and K >= 2:
        assert mr.cross_list_ties(pv, pi, K).max() >= 1            # some tie is decided between two lists
        of = mr.merge_final(pv, pi, K)[3]
        assert (of & 1).any() and (of & 2).any() and (of == 0).any()
    if regime == "short":
        assert (live < K).any()                                    # a query with fewer than K entries in total
        assert ((pi != INT_MAX).sum(axis=2) == 0).any()            # a list that is all padding
    if regime == "inf":
        assert (np.isposinf(pv) & (pi != INT_MAX)).any()           # real ids at +inf
        oi, od, oc, of = mr.merge_final(pv, pi, K)
        assert (np.isposinf(od) & (oi >= 0)).any()                 # ... that reach an output
    if regime == "zeros":
        z = bits(pv[pi != INT_MAX])
        assert (z == 0x80000000).any() and (z == 0).any()


def test_check_precondition_rejects_bad_lists():
    pv, pi = mr.make_lists(np.random.default_rng(0), 2, 1, 4, "distinct")
    for spoil in ("order", "dup", "padding"):
        v, i = pv.copy(), pi.copy()
        if spoil == "order":
            v[0, 0, [0, 1]] = v[0, 0, [1, 0]]
        elif spoil == "dup":
            i[1, 0, 0] = i[0, 0, 0]
        else:
            i[0, 0, 1] = INT_MAX
        with pytest.raises(AssertionError):
            mr.check_precondition(v, i)
