"""Adversarial inputs for the tie replay (replay.hip): data on which rows insert LATE into the reference's TopKHeap.

On random codes a query's running K-th distance is final after a few thousand rows, a flagged query has a few hundred
replay candidates and none of the replay's limits is near.  A *staircase* is a set of rows at chosen positions whose
distances to one target query fall strictly from row to row: every one of them inserts into the reference heap, however
late it comes.  That drives, exactly, the number of successful insertions (the keep list of rp_heap, 2 048), the number
of candidates (the pool, 8 192; 2 048 per shard) and which level of the replay meets an inserting row.

Everything here is seeded, runs on the CPU and looks at the reference alone: distances are the numpy restatement of
the oracle's j-ordered binary32 sums over oracle.prepare_query's table, the insertion count is a heap walk over them.
test_replay_adversary.py asserts every predicate for every case below; test_gpu_replay_limits.py runs the cases.

    case(oracle, name) -> Case        (cached: the CPU and GPU tests of one process share the arrays)
    batch(case, B)     -> Q [B][d], target positions, neighbour positions
"""
import collections
import heapq

import numpy as np

from value_regimes import decode

N3 = 147968                 # (64 + 2048 + 200) * 64 rows: the replay's three levels, 200 row blocks in the long one
L0_ROWS = 64 * 64           # level 0 of a handle that has not seen many flagged queries
L1_SEG_ROWS = 64 * 64       # one level-1 segment
KEEP = 2048                 # successful insertions rp_heap keeps per query
POOL = 8192                 # candidates per query; POOL_SHARD per shard of a sharded index
POOL_SHARD = 2048
PAIRS = 37                  # duplicated rows for the ordinary tied queries of a batch (B = 40: 3 targets + 37)

FORMS = {                   # d, m, k
    "m8": (32, 8, 256),         # 4-byte code words
    "m16": (64, 16, 256),       # 16-byte code words
    "m32": (64, 32, 256),       # two 16-byte words per row (ng > 1)
    "w1024": (32, 8, 1024),     # wide codes: rp_scan_wide
}

Case = collections.namedtuple("Case", "name kind n d m k K frm until cents idx q positions insertions pairs extra")

# name: (kind, form, n, K, frm, until, S or the exact insertion count, seed)
CASES = {}
for _form in ("m8", "m16", "m32"):
    for _K in (2, 10, 63):
        CASES[f"late-{_form}-K{_K}"] = ("stairs", _form, N3, _K, 0, N3, 1500, 11)
for _K in (2, 10, 63):      # a sub-range whose first row cuts a row block, the last one too
    CASES[f"late-m8range-K{_K}"] = ("stairs", "m8", N3, _K, 64 * 64 + 37, N3 - 75, 1500, 12)
CASES.update({
    "keep-l0-2048": ("exact", "m8", 4096, 10, 0, 4096, KEEP, 13),
    "keep-l0-2049": ("exact", "m8", 4096, 10, 0, 4096, KEEP + 1, 13),
    "keep-3l-2048": ("exact", "m16", N3, 10, 0, N3, KEEP, 14),
    "keep-3l-2049": ("exact", "m16", N3, 10, 0, N3, KEEP + 1, 14),
    "overflow-m16": ("stairs", "m16", N3, 10, 0, N3, 9000, 15),
    "segments-m8": ("segments", "m8", N3, 10, 0, N3, 300, 16),
    "late-w1024": ("stairs", "w1024", N3, 10, 0, N3, 1500, 17),
    "overflow-w1024": ("stairs", "w1024", N3, 10, 0, N3, 9000, 18),
    "shard-local-m16": ("shards", "m16", N3, 10, 0, N3, 2100, 19),
})
LATE_CASES = [c for c in CASES if c.startswith("late-m")]


def distances(oracle, cents, idx, d, m, k, q):
    """[n] float32: the reference's distance of every row to q (Index.scala sums the quantizers in order, in binary32)"""
    T = oracle.prepare_query(cents, d, m, k, np.ascontiguousarray(q, np.float32).reshape(1, d))[0]
    acc = np.zeros(idx.shape[1], np.float32)
    for j in range(m):
        acc = (acc + T[j, idx[j]]).astype(np.float32)
    return acc


def insertions(dist, K):
    """Successful TopKHeap.update calls over the rows in order: a row inserts if fewer than K came before or its distance
    is strictly below the K-th smallest so far (TopKHeap.scala:57-67)."""
    heap, count = [], 0          # max-heap of the K smallest, negated
    for c0 in range(0, len(dist), 4096):
        chunk = dist[c0:c0 + 4096]
        cand = range(len(chunk)) if len(heap) < K else np.flatnonzero(chunk < -heap[0])
        for i in cand:
            v = float(chunk[i])
            if len(heap) < K:
                heapq.heappush(heap, -v)
                count += 1
            elif v < -heap[0]:
                heapq.heapreplace(heap, -v)
                count += 1
    return count


def fast_path_rows(dist, K):
    """the (distance, row id) rule of the fast path: the K smallest distances, the cut and the order by row id"""
    return np.lexsort((np.arange(len(dist)), dist))[:K]


def spread(S, lo, hi):
    """S distinct ascending rows of [lo, hi - 1), evenly spaced (hi - 1 is kept for the copy of the best row)"""
    assert hi - 1 - lo >= S
    return lo + (np.arange(S, dtype=np.int64) * (hi - 1 - lo)) // S


def _distinct_smallest(dist, S):
    """the rows of the S smallest pairwise-distinct distances (first row of each value), ascending by distance"""
    _, first = np.unique(dist, return_index=True)
    assert len(first) >= S
    return first[:S]


def _draw(oracle, n, d, m, k, seed):
    rng = np.random.default_rng(seed)
    cents = rng.standard_normal(k * d).astype(np.float32)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    q = rng.standard_normal(d).astype(np.float32)
    return rng, cents, idx, q, distances(oracle, cents, idx, d, m, k, q)


def _place(idx, placed, rng, first_rows=None):
    """idx with source row placed[p] at position p and every other row at a shuffled free position; first_rows: the
    source rows that the free positions of [0, L0_ROWS) are filled from"""
    n = idx.shape[1]
    perm = np.full(n, -1, np.int64)
    pos = np.fromiter(placed.keys(), np.int64, len(placed))
    src = np.fromiter(placed.values(), np.int64, len(placed))
    assert len(np.unique(src)) == len(src)
    perm[pos] = src
    used = np.zeros(n, bool)
    used[src] = True
    if first_rows is not None:
        free0 = np.flatnonzero(perm[:L0_ROWS] < 0)
        pick = rng.permutation(first_rows[~used[first_rows]])[:len(free0)]
        perm[free0] = pick
        used[pick] = True
    free = np.flatnonzero(perm < 0)
    perm[free] = rng.permutation(np.flatnonzero(~used))
    assert np.array_equal(np.sort(perm), np.arange(n))
    return np.ascontiguousarray(idx[:, perm])


def _finish(idx, best_pos, taken, frm, until, rng):
    """the copy of the best row at the range's last row (an interior tie for K >= 2: the target is flagged) and PAIRS
    rows with one duplicate each, outside every staircase: the ordinary tied queries of a batch decode those"""
    n = idx.shape[1]
    idx[:, until - 1] = idx[:, best_pos]
    free = np.ones(n, bool)
    free[taken] = False
    free[until - 1:] = False
    free[:max(frm, L0_ROWS if until - frm > 2 * L0_ROWS else frm)] = False
    rows = rng.permutation(np.flatnonzero(free))[:2 * PAIRS]
    a, b = np.sort(rows[:PAIRS]), rows[PAIRS:]
    idx[:, b] = idx[:, a]
    return [(int(x), int(y)) for x, y in zip(a, b)]


def staircase(oracle, n, d, m, k, K, positions, seed, frm=0, until=None):
    """Random centroids, codes and one target query; the S = len(positions) rows with the smallest pairwise-distinct
    distances sit at `positions` (ascending) in strictly descending distance, every other row at a shuffled position;
    the last row of the range is a copy of the best row.  -> cents, idx [m][n], q, reference insertions, pairs"""
    until = n if until is None else until
    positions = np.asarray(positions, np.int64)
    assert np.all(np.diff(positions) > 0) and positions[0] >= frm and positions[-1] < until - 1
    rng, cents, idx, q, dist = _draw(oracle, n, d, m, k, seed)
    rows = _distinct_smallest(dist, len(positions))[::-1]               # descending distance
    idx = _place(idx, dict(zip(positions.tolist(), rows.tolist())), rng)
    pairs = _finish(idx, int(positions[-1]), positions, frm, until, rng)
    final = distances(oracle, cents, idx, d, m, k, q)
    return cents, idx, q, insertions(final[frm:until], K), pairs


def staircase_with_insertions(oracle, n, d, m, k, K, target, seed):
    """staircase() over evenly spread positions whose reference insertion count is exactly `target`: one more staircase
    row is one more insertion, so S is corrected by the difference (the caller asserts the count)."""
    S, seen = target - 4 * K, {}
    while True:
        positions = spread(S, 0, n)
        out = staircase(oracle, n, d, m, k, K, positions, seed)
        seen[S] = out[3]
        if out[3] == target or len(seen) == 24:
            return out + (positions,)
        S += target - out[3]
        if S in seen:        # the spacing moved with S and the correction came back: walk the neighbourhood instead
            S = min(seen) - 1 if len(seen) % 2 else max(seen) + 1


def segment_stairs(oracle, n, d, m, k, K, seed, windows=32, per_window=300):
    """Many candidates, few insertions.  Rows [0, L0_ROWS) come from the large-distance half; each of the `windows`
    following level-1 segments holds a descending staircase of `per_window` rows: the first from the smallest
    distances, every later one from ranks above the first window's K-th smallest and below every other row.  The
    reference inserts the first staircase and nothing after it; a segment scan that starts from level 0's loose bound
    emits all of them."""
    assert n >= L0_ROWS + windows * L1_SEG_ROWS + 1
    rng, cents, idx, q, dist = _draw(oracle, n, d, m, k, seed)
    ranked = _distinct_smallest(dist, windows * per_window)
    placed, positions = {}, []
    for w in range(windows):
        pos = spread(per_window, L0_ROWS + w * L1_SEG_ROWS, L0_ROWS + (w + 1) * L1_SEG_ROWS + 1)
        src = ranked[w * per_window:(w + 1) * per_window][::-1]
        placed.update(zip(pos.tolist(), src.tolist()))
        positions.append(pos)
    positions = np.concatenate(positions)
    far_half = np.argsort(dist, kind="stable")[n // 2:]
    idx = _place(idx, placed, rng, first_rows=far_half)
    pairs = _finish(idx, int(positions[per_window - 1]), positions, 0, n, rng)
    final = distances(oracle, cents, idx, d, m, k, q)
    return cents, idx, q, insertions(final, K), pairs, positions


def shard_ranges(n, shards):
    return [(n * s // shards, n * (s + 1) // shards) for s in range(shards)]


def shard_local_stairs(oracle, n, d, m, k, K, seed, shards=3, first=300, S=2100):
    """Shard 0's rows hold the `first` smallest distances (shuffled), so the reference's bound is final before shard
    0 ends; the last shard holds a descending staircase of the next S ranks: none of them inserts into the
    reference's heap, all of them into a heap that starts cold at the shard's first row."""
    rng, cents, idx, q, dist = _draw(oracle, n, d, m, k, seed)
    ranked = _distinct_smallest(dist, first + S)
    rg = shard_ranges(n, shards)
    placed = dict(zip(rng.permutation(np.arange(L0_ROWS, rg[0][1]))[:first].tolist(), ranked[:first].tolist()))
    positions = spread(S, rg[-1][0], n)
    placed.update(zip(positions.tolist(), ranked[first:][::-1].tolist()))
    best_pos = [p for p, r in placed.items() if r == ranked[0]][0]
    idx = _place(idx, placed, rng)
    taken = np.fromiter(placed.keys(), np.int64, len(placed))
    pairs = _finish(idx, best_pos, taken, 0, n, rng)
    final = distances(oracle, cents, idx, d, m, k, q)
    local = insertions(final[rg[-1][0]:], K)
    return cents, idx, q, insertions(final, K), pairs, positions, local


_cache = collections.OrderedDict()


def case(oracle, name):
    if name in _cache:
        _cache.move_to_end(name)
        return _cache[name]
    kind, form, n, K, frm, until, S, seed = CASES[name]
    d, m, k = FORMS[form]
    extra = {}
    if kind == "stairs":
        positions = spread(S, frm, until)
        cents, idx, q, ins, pairs = staircase(oracle, n, d, m, k, K, positions, seed, frm, until)
    elif kind == "exact":
        cents, idx, q, ins, pairs, positions = staircase_with_insertions(oracle, n, d, m, k, K, S, seed)
    elif kind == "segments":
        cents, idx, q, ins, pairs, positions = segment_stairs(oracle, n, d, m, k, K, seed, per_window=S)
    else:
        cents, idx, q, ins, pairs, positions, local = shard_local_stairs(oracle, n, d, m, k, K, seed, S=S)
        extra["last_shard_insertions"] = local
    c = Case(name, kind, n, d, m, k, K, frm, until, cents, idx, q, positions, ins, pairs, extra)
    _cache[name] = c
    while len(_cache) > 3:
        _cache.popitem(last=False)
    return c


def batch(c, B):
    """A mixed batch: the target query at 0, B // 2 and B - 1, ordinary tied queries -- the decoded rows that have one
    duplicate each -- everywhere between.  -> Q [B][d], target positions, neighbour positions"""
    assert 4 <= B <= PAIRS + 3
    targets = [0, B // 2, B - 1]
    others = [p for p in range(B) if p not in targets]
    Q = np.empty((B, c.d), np.float32)
    Q[targets] = c.q
    rows = np.array([a for a, _ in c.pairs[:len(others)]])
    Q[others] = decode(c.cents, c.idx[:, rows], c.d, c.m, c.k)
    return Q, targets, others
