"""Reference of the merge of sorted (distance, row id) lists and of the large-K peel, in numpy and plain Python.

The operation is a pure function: the union of the lists, ordered by (distance as a float VALUE, row id), cut to K.
`-0.0` and `+0.0` are one value (the id decides between them) and every entry keeps its own bit pattern.  An entry
with id INT_MAX is padding whatever its distance; a real id at `+inf` is an entry like any other and sorts before the
padding.  NaN is out of scope: a scan never emits one (`acc <= tau` rejects it), so no list here holds one and nothing
below says where one would go.

merge_final    what gulon_topk_merge / gulon_topk_merge_dev must return for [lists][B][K+1] partial lists
finalize       one query's sorted entries -> K output slots, count and tie flags (also the tail of a peeled query)
peeled_rounds  the peel restated: round r = the 64 smallest pairs strictly after round r-1's last one
make_lists     constructed inputs that meet the kernels' precondition, in five regimes
"""
import numpy as np

INT_MAX = int(np.iinfo(np.int32).max)
FLAG_BOUNDARY_TIE = 1
FLAG_INTERIOR_TIE = 2
ROUND = 64
REGIMES = ("distinct", "ties", "short", "inf", "zeros")
TIE_VALUES = (0.5, 1.0, 2.0)


def order(dist, ids):
    """Positions of the entries in ascending (distance value, id) order; -0.0 == +0.0."""
    dist = np.asarray(dist, np.float32)
    return np.lexsort((np.asarray(ids, np.int64), dist + np.float32(0.0)))       # -0.0 + 0.0 = +0.0


def finalize(ids, dist, K):
    """ids / dist: one query's live entries in (distance, id) order (K+1 of them are enough).
    -> (idx[K], dist[K], count, flags): unfilled slots (-1, +inf); flags from entries e, e+1 of the first K+1."""
    ids = np.asarray(ids, np.int32)
    dist = np.asarray(dist, np.float32)
    assert not (ids == INT_MAX).any()
    count = min(K, len(ids))
    oi = np.full(K, -1, np.int32)
    od = np.full(K, np.inf, np.float32)
    oi[:count] = ids[:count]
    od[:count] = dist[:count]
    flags = 0
    for e in range(min(K, len(ids) - 1)):
        if dist[e] == dist[e + 1]:
            flags |= FLAG_BOUNDARY_TIE if e == K - 1 else FLAG_INTERIOR_TIE
    return oi, od, count, flags


def merged_entries(pv, pi, q):
    """Query q's live entries of every list in (distance, id) order: (ids, dist, source list)."""
    pv, pi = np.asarray(pv, np.float32), np.asarray(pi, np.int32)
    v, i = pv[:, q, :].reshape(-1), pi[:, q, :].reshape(-1)
    src = np.repeat(np.arange(pv.shape[0]), pv.shape[2])
    live = i != INT_MAX
    v, i, src = v[live], i[live], src[live]
    o = order(v, i)
    return i[o], v[o], src[o]


def merge_final(pv, pi, K):
    """[lists][B][K+1] -> (idx[B][K], dist[B][K], count[B], flags[B])."""
    pv, pi = np.asarray(pv, np.float32), np.asarray(pi, np.int32)
    lists, B, keff = pv.shape
    assert keff == K + 1 and pi.shape == pv.shape
    oi = np.zeros((B, K), np.int32)
    od = np.zeros((B, K), np.float32)
    oc = np.zeros(B, np.int32)
    of = np.zeros(B, np.int32)
    for q in range(B):
        ids, dist, _ = merged_entries(pv, pi, q)
        oi[q], od[q], oc[q], of[q] = finalize(ids[:K + 1], dist[:K + 1], K)
    return oi, od, oc, of


def cross_list_ties(pv, pi, K):
    """Per query: neighbouring entries of the merged K+1 that are equal in distance and come from different lists --
    the places where only the id orders two lists' entries."""
    B = np.asarray(pv).shape[1]
    out = np.zeros(B, np.int64)
    for q in range(B):
        ids, dist, src = merged_entries(pv, pi, q)
        ids, dist, src = ids[:K + 1], dist[:K + 1], src[:K + 1]
        out[q] = int(((dist[1:] == dist[:-1]) & (src[1:] != src[:-1])).sum())
    return out


def peeled_rounds(dist_all, rows_all, K):
    """The peel of one query over the rows (rows_all[i], dist_all[i]): ceil((K+1)/64) rounds, round r the 64 smallest
    (distance, id) pairs STRICTLY after the bound, which starts at (-1.0, -1) and becomes the round's last pair, or
    (+inf, INT_MAX) once a round comes back short (nothing is eligible after that).
    -> (ids, dist) of rounds * 64 entries, padded with (INT_MAX, +inf).  Cut it to K for the final output (finalize on
    the live part) or to K + 1 for a shard's partial list (peel_partial)."""
    dist_all = np.asarray(dist_all, np.float32)
    rows_all = np.asarray(rows_all, np.int64)
    rounds = -(-(K + 1) // ROUND)
    ids = np.full(rounds * ROUND, INT_MAX, np.int32)
    dist = np.full(rounds * ROUND, np.inf, np.float32)
    lbv, lbi = np.float32(-1.0), -1
    for r in range(rounds):
        eligible = (dist_all > lbv) | ((dist_all == lbv) & (rows_all > lbi))
        if lbi == INT_MAX:
            eligible[:] = False
        v, i = dist_all[eligible], rows_all[eligible]
        o = order(v, i)[:ROUND]
        ids[r * ROUND:r * ROUND + len(o)] = i[o]
        dist[r * ROUND:r * ROUND + len(o)] = v[o]
        if len(o) == ROUND:
            lbv, lbi = v[o[-1]], int(i[o[-1]])
        else:
            lbv, lbi = np.float32(np.inf), INT_MAX
    return ids, dist


def peel_final(ids, dist, K):
    """peeled_rounds' lists cut to the final output: (idx[K], dist[K], count, flags)."""
    live = ids != INT_MAX
    return finalize(ids[live][:K + 1], dist[live][:K + 1], K)


def peel_partial(ids, dist, K):
    """peeled_rounds' lists cut to a shard's partial (K+1)-list: (dist[K+1], ids[K+1]), padding included."""
    return dist[:K + 1].copy(), ids[:K + 1].copy()


# ---- constructed inputs ---------------------------------------------------------------------------------------------

def _pack(per_list, K):
    """per_list: [(dist, ids)] of one query, any order, at most K+1 each -> sorted, padded [lists][K+1] arrays."""
    pv = np.full((len(per_list), K + 1), np.inf, np.float32)
    pi = np.full((len(per_list), K + 1), INT_MAX, np.int32)
    for l, (v, i) in enumerate(per_list):
        v, i = np.asarray(v, np.float32), np.asarray(i, np.int32)
        assert len(v) == len(i) <= K + 1
        o = order(v, i)
        pv[l, :len(o)] = v[o]
        pi[l, :len(o)] = i[o]
    return pv, pi


def _ids(rng, total):
    """`total` distinct row ids, ascending, with gaps; the largest legal id (INT_MAX - 1) among them now and then."""
    ids = np.sort(rng.choice(max(4 * total, 8), size=total, replace=False)).astype(np.int64)
    if total and rng.integers(0, 2):
        ids[-1] = INT_MAX - 1
    return ids


def _deal(ids, dist, counts, interleave, rng):
    """Split the entries over the lists: list l gets counts[l] of them -- round-robin in id order (interleave: ids of
    neighbouring rank sit in different lists) or at random."""
    lists = len(counts)
    where = np.full(len(ids), -1)
    if interleave:
        left = list(counts)
        l = 0
        for e in range(len(ids)):
            while left[l] == 0:
                l = (l + 1) % lists
            where[e] = l
            left[l] -= 1
            l = (l + 1) % lists
    else:
        where = rng.permutation(np.repeat(np.arange(lists), counts))
    return [(dist[where == l], ids[where == l]) for l in range(lists)]


def make_lists(rng, lists, B, K, regime):
    """[lists][B][K+1] (pv float32, pi int32): every list ascending in (distance, id), padded with (+inf, INT_MAX);
    ids distinct within a query across its lists; no NaN.

    distinct  full lists, every distance of a query different
    ties      full lists, ids dealt round-robin so that the id decides between lists; query q draws its distances from
              TIE_VALUES, exactly K of them the smallest (q % 3 == 0: the cut falls where the value changes, so ties
              inside and none at the boundary), has none equal (q % 3 == 1: a batch keeps unflagged queries), or has
              all equal (q % 3 == 2: interior and boundary)
    short     0 .. K+1 live entries per list; q % 3 == 0: fewer than K in total; q % 3 <= 1: one list wholly padding
    inf       real ids at +inf behind the finite entries, lists not full: +inf entries next to padding, and few enough
              finite ones (q % 2 == 0) that the +inf entries reach the output
    zeros     -0.0 and +0.0 mixed (one value: the id decides), some 1.0 behind them
    """
    assert regime in REGIMES
    keff = K + 1
    pv = np.zeros((lists, B, keff), np.float32)
    pi = np.zeros((lists, B, keff), np.int32)
    for q in range(B):
        counts = [keff] * lists
        interleave = False
        if regime == "short":
            if q % 3 == 0:
                share = np.ones(lists)
                if lists > 1:
                    share[int(rng.integers(0, lists))] = 0.0                  # ... with one list wholly padding
                counts = [int(c) for c in rng.multinomial(int(rng.integers(0, K)), share / share.sum())]
            else:
                counts = [int(c) for c in rng.integers(0, keff + 1, lists)]
                if q % 3 == 1:
                    counts[int(rng.integers(0, lists))] = 0
        elif regime == "inf":
            counts = [int(c) for c in rng.integers(1, keff, lists)]           # 1 .. K: never full
        total = sum(counts)
        ids = _ids(rng, total)
        if regime in ("distinct", "short"):
            dist = (rng.permutation(total) * 0.25).astype(np.float32)
        elif regime == "ties":
            interleave = True
            if q % 3 == 0:
                dist = rng.choice(np.asarray(TIE_VALUES[1:], np.float32), total)
                dist[rng.permutation(total)[:K]] = TIE_VALUES[0]
            elif q % 3 == 1:
                dist = (rng.permutation(total) * 0.25).astype(np.float32)
            else:
                dist = np.full(total, TIE_VALUES[(q // 3) % 3], np.float32)
        elif regime == "inf":
            dist = (rng.permutation(total) * 0.25).astype(np.float32)
            finite = int(rng.integers(0, max(K // 2, 1))) if q % 2 == 0 else total // 2
            dist[rng.permutation(total)[finite:]] = np.inf
        else:
            interleave = True
            dist = rng.choice(np.asarray([-0.0, 0.0, 0.0, -0.0, 1.0], np.float32), total)
        v, i = _pack(_deal(ids, dist, counts, interleave, rng), K)
        pv[:, q, :], pi[:, q, :] = v, i
    return pv, pi


def check_precondition(pv, pi):
    """What the merge kernels assume of their input; raises AssertionError naming the list."""
    pv, pi = np.asarray(pv, np.float32), np.asarray(pi, np.int32)
    lists, B, keff = pv.shape
    assert not np.isnan(pv).any()
    for q in range(B):
        seen = set()
        for l in range(lists):
            v, i = pv[l, q], pi[l, q]
            live = int((i != INT_MAX).sum())
            assert (i[:live] != INT_MAX).all() and (i[live:] == INT_MAX).all(), (q, l)      # padding is a suffix
            assert np.isposinf(v[live:]).all(), (q, l)
            assert (i[:live] >= 0).all(), (q, l)
            key = [(float(a) + 0.0, int(b)) for a, b in zip(v[:live], i[:live])]
            assert all(x < y for x, y in zip(key, key[1:])), (q, l)                         # strictly ascending
            ids = set(i[:live].tolist())
            assert len(ids) == live and not (ids & seen), (q, l)
            seen |= ids
