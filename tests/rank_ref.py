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


def unranked(want, q):
    """Does the reference give query q no best gold row?"""
    rank, row, key, _ = want
    return bool(rank[q] == -1 and row[q] == -1 and np.isposinf(key[q]))


# ---- what test_gpu_rank_paths.py adds: gold lists of up to 300 rows, and the exact launcher's row chunks --------------

LONG_LENGTHS = (0, 1, 2, 63, 64, 65, 129, 300)   # per query in turn: a wave's 64 lanes from both sides, 3 and 5 trips
SLOTS = ("last", 64, 130, 63, "first")           # where the best row sits in its list, clipped to the list's last index


def slot_index(slot, length):
    return min({"first": 0, "last": length - 1}.get(slot, slot), length - 1)


def plant_long(order, w, offsets, outside, positions, lengths=LONG_LENGTHS, turn=0, twin=None, seed=0):
    """Per query a gold list of lengths[q % len(lengths)] rows whose best row is the one at a chosen position p of the
    query's full order: p = positions[(q + turn) % len(positions)] (negative: from the end), or with `twin` = (row, copy)
    the position of `row`.  The best row sits at SLOTS[...] of its list -- the lists of 65 rows and more and the shorter
    ones take the SLOTS in turn, each kind from `turn` on -- and the other entries are the query's excluded row,
    `outside`, three rows masked by +inf and rows drawn from those strictly behind position p (masked rows again where
    there are too few), shuffled, with one repeat of the best row somewhere behind it where the list has room.  With
    `twin` the copy -- an equal key, the higher id -- is the list's first entry and the best row comes after it.
    -> (gold: b lists, at [b]: the index of the best row in its list, -1 for an empty list, expect: per query
    (p, row), None for an empty list)."""
    ids = w["ids"]
    masked = ids[np.isposinf(offsets[ids])]
    rng = np.random.default_rng(seed)
    gold, at, expect = [], [], []
    seen = {True: 0, False: 0}
    for q, o in enumerate(order):
        length = lengths[q % len(lengths)]
        if twin is None:
            p = positions[(q + turn) % len(positions)]
            p = p if p >= 0 else len(o) + p
        else:
            p = o.tolist().index(twin[0])
        assert 0 <= p < len(o), (p, len(o))
        if length == 0:
            gold.append([]), at.append(-1), expect.append(None)
            continue
        i = slot_index(SLOTS[(seen[length >= 65] + turn) % len(SLOTS)], length)
        seen[length >= 65] += 1
        best = int(o[p])
        others = [int(twin[1])] if twin is not None and length >= 2 else []
        i = max(i, len(others))
        rest = ([int(w["exclude"][q])] if w["exclude"][q] >= 0 else []) + ([] if outside is None else [int(outside)])
        rest += [int(masked[(q + j) % len(masked)]) for j in range(3)]
        behind = o[p + 1:]
        want = max(0, length - 1 - len(others) - len(rest))
        rest += rng.choice(behind, min(want, len(behind)), replace=False).tolist()
        rest += [int(masked[(q + j) % len(masked)]) for j in range(length)]      # where too few rows are behind
        rest = rest[:length - 1 - len(others)]
        others += [rest[j] for j in rng.permutation(len(rest))]
        mine = others[:i] + [best] + others[i:]
        if length >= 3 and i < length - 1:
            mine[int(rng.integers(i + 1, length))] = best                        # a repeat of the best row, behind it
        assert len(mine) == length and mine[i] == best and best not in mine[:i]
        gold.append(mine), at.append(i), expect.append((p, best))
    return gold, np.array(at), expect


def shows_long(want, order, expect):
    """The reference ranks every query's best row at its chosen position, and no query with an empty list."""
    rank, row, key, total = want
    for q, e in enumerate(expect):
        if total[q] != len(order[q]):
            return False
        if e is None:
            if not unranked(want, q):
                return False
        elif not (rank[q] == e[0] and row[q] == e[1] == order[q][e[0]] and np.isfinite(key[q])):
            return False
    return True


def knn_row_chunks(frm, until, tiles):
    """exact.hpp's knn_row_chunks restated: the 256-row groups that cover [frm, until), frm rounded down to a group, in
    chunks for about 2048 workgroups over `tiles` query tiles of 16.  -> (row chunks, groups per chunk)."""
    groups = max(1, -(-(until - frm // 256 * 256) // 256))
    per = -(-groups // min(max(-(-2048 // tiles), 1), groups))
    return -(-groups // per), per


def agrees_with_the_offset_query(got, lists):
    """Every rank below 63 is the position of the row in the offset query's answer at 63; -> how many were checked."""
    rank, row = got[0], got[1]
    near = np.flatnonzero((rank >= 0) & (rank < 63))
    assert np.array_equal(lists[near, rank[near]], row[near])
    return len(near)
