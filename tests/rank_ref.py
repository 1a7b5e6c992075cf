"""What the rank-query tests share: gold lists PLANTED from the reference's full order of every query, so
that each case a rank query has to get right is present by construction -- and asserted on the reference before the
device is asked -- and the comparison of all four outputs with ranks.rank_query_reference, keys by bits."""
import numpy as np

from conftest import bits

POSITIONS = (0, 1, 62, 63, 64, -1)               # the list boundary of the offset query (63) from both sides, and last
KINDS = tuple(f"at{p}" for p in POSITIONS) + ("unrankable", "empty", "three", "twin_low", "twin_high")


def pick_twins(twins, exclude):
    """The first (row, copy) pair none of whose rows a query excludes: both are candidates of every query."""
    banned = set(np.asarray(exclude).tolist())
    return next((a, c) for a, c in twins if a not in banned and c not in banned)


def full_order(g, w, offsets):
    """Per query the candidates in order: the offset reference at k = the columns.  w: dist [b][n], ids [n], exclude [b];
    offsets: per row id.  -> list of b int arrays."""
    ids = w["ids"]
    oi, _, oc = g.offset_query_reference(w["dist"], offsets[ids], len(ids), w["exclude"], rows=ids)
    return [oi[q, :oc[q]] for q in range(len(oc))]


def plant(kind, order, w, offsets, twin, outside):
    """The gold list of every query for one kind.  order: full_order; twin: (row, copy) with equal rows and offsets,
    row < copy, candidates of every query; outside: a valid row id that lies outside the handle's range, or None."""
    ids = w["ids"]
    masked = ids[np.isposinf(offsets[ids])]
    gold = []
    for q, o in enumerate(order):
        assert len(o) > 65, len(o)
        if kind.startswith("at"):
            gold.append([o[int(kind[2:])]])
        elif kind == "unrankable":                       # masked by +inf, the excluded row, outside the range
            gold.append([masked[q % len(masked)]] + ([] if outside is None else [outside])
                        + ([w["exclude"][q]] if w["exclude"][q] >= 0 else []))
        elif kind == "empty":
            gold.append([])
        elif kind == "three":                            # the best of the three is the second entry
            gold.append([o[40], o[7], o[20]])
        elif kind == "twin_low":                         # the gold row's twin has the lower id: it is ahead
            gold.append([twin[1]])
        else:                                            # ... the higher id: it is not
            gold.append([twin[0]])
    return gold


def reference(g, w, offsets, gold):
    ids = w["ids"]
    return g.rank_query_reference(w["dist"], offsets[ids], gold, w["exclude"], rows=ids)


def shows(kind, want, order, twin):
    """Does the reference itself show the case the kind was planted for?"""
    rank, row, key, total = want
    b = len(rank)
    if not all(total[q] == len(order[q]) for q in range(b)):
        return False
    if kind.startswith("at"):
        p = int(kind[2:])
        return all(rank[q] == (p if p >= 0 else len(order[q]) - 1) and row[q] == order[q][p] for q in range(b))
    if kind in ("unrankable", "empty"):
        return bool((rank == -1).all() and (row == -1).all() and np.isposinf(key).all() and (total > 0).all())
    if kind == "three":
        return all(rank[q] == 7 and row[q] == order[q][7] for q in range(b))
    a, c = twin
    at = [order[q].tolist().index(a) for q in range(b)]
    if not all(order[q][at[q] + 1] == c for q in range(b)):      # equal keys: the twins are neighbours, the lower id first
        return False
    if kind == "twin_low":
        return all(rank[q] == at[q] + 1 and row[q] == c for q in range(b))
    return all(rank[q] == at[q] and row[q] == a for q in range(b))


def same(got, want):
    for name, a, c in zip(("rank", "row", "key", "total"), got, want):
        a, c = (bits(a), bits(c)) if name == "key" else (np.asarray(a), np.asarray(c))
        assert np.array_equal(a, c), (name, np.flatnonzero(a != c)[:8], a[a != c][:8], c[a != c][:8])


def agrees_with_the_offset_query(got, lists):
    """Every rank below 63 is the position of the row in the offset query's answer at 63; -> how many were checked."""
    rank, row = got[0], got[1]
    near = np.flatnonzero((rank >= 0) & (rank < 63))
    assert np.array_equal(lists[near, rank[near]], row[near])
    return len(near)
