"""The rank queries (csrc/rank.hip) on the paths test_gpu_rank_flat.py and test_gpu_rank_exact.py do not
reach: gold lists longer than a wave (second and later trips of rank_flat_gold's lane loop, several 256-slot steps of
rank_exact_gold, lists that straddle a step, empty lists between long ones), classes of hundreds of equal keys in the gold
reduction and in the counting scans, the slot counts E the LDS budget or a small batch forces, non-finite queries on the
flat form, negative and signed-zero offsets, a flat handle with a row base and its context, and a handle's history.

The reference is the one of those two files: ranks.rank_query_reference over the handle's own distances -- its ordinary
query at k = the rows of the range, scattered back by row id -- and all four outputs are compared with rank_ref.same,
keys by bits, no tolerance.  Where a world has a quantizer count no other file checks against the oracle (m = 3, 32, 80,
144) the handle's distances are themselves compared with the oracle's, bit for bit.  Every test first asserts, from the
reference side alone, that the case it names occurs in its inputs; the launch geometry is not observable, so it is
derived by offset_ref.flat_slots / flat_chunks and rank_ref.knn_row_chunks, which restate the launchers' arithmetic.

Flat worlds: 256 centroids, one training iteration, unit rows.  "big": the worlds of test_gpu_rank_flat.py, 4 300 rows
over [70, n - 33), 19 queries; "small": those of test_gpu_offset_paths.py, 327 rows over [5, n - 3), with eight twin
pairs; "ties": 6 407 rows, row r = base[r % 8], encoded by the small m = 16 quantizer.  Exact worlds: those of
test_gpu_rank_exact.py, and the "ties" world of test_gpu_offset_paths.py (700 rows, d = 33, row r = base[r % 4])."""
import numpy as np
import pytest

import rank_ref
from conftest import bits
from cosmul_ref import unit_rows
from offset_ref import (LEVELS, SIGNED_LEVELS, ceil_div, distances_by_row, distances_in_steps, draw_offsets, flat_chunks,
                        flat_slots, huge_offsets, noisy_queries, nonfinite_queries, plant_nearest)

pytestmark = pytest.mark.gpu

K, ITERS = 256, 1
DIMENSIONS = {3: 32, 16: 32, 25: 50, 32: 64, 80: 80, 144: 144}
N, FROM = 4300, 70                                   # the big worlds
UNTIL = N - 33
TWINS = [(200 + i, 3000 + i) for i in range(20)]
SMALL_N = 64 * 5 + 7                                 # the small worlds
SMALL_TWINS = [(20 + i, 200 + i) for i in range(8)]
TIE_N = 64 * 100 + 7                                 # the range's 101 code blocks: three chunks of 34, 34 and 33
EXACT_TWINS = [(100 + i, 400 + i) for i in range(20)]
BASE = 1000
POSITIONS = (0, 64, 1000, -1, 7)                     # of the full order (about 3 700 candidates): the best gold row
# m -> (vec, ng, m_pad, E by the LDS budget, E) for a batch of 5
SLOTS = {3: (4, 1, 4, 8, 8), 32: (16, 2, 32, 4, 4), 80: (16, 5, 80, 1, 1), 144: (16, 9, 144, 1, 1)}


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


_FLAT, _EXACT = {}, {}


@pytest.fixture(scope="module", autouse=True)
def close_worlds():
    yield
    for w in _FLAT.values():
        w["vi"].close()
    _FLAT.clear()
    for w in _EXACT.values():
        w["ix"].close()
        w["dm"].close()
    _EXACT.clear()


def ask(w, gold, offsets="own", exclude="own", Q=None, handle=None):
    """The rank query of a world's handle (or of `handle`, made over the same codes or rows) over the world's range."""
    offsets = w["offsets"] if isinstance(offsets, str) else offsets
    exclude = w["exclude"] if isinstance(exclude, str) else exclude
    Q = w["Q"] if Q is None else Q
    if "vi" in w:
        return (handle or w["vi"]).batch_query_rank_raw(Q, gold, offsets, exclude, w["frm"], w["until"])
    return (handle or w["ix"]).batch_query_rank_raw(Q, gold, offsets, exclude)


# ---------------------------------------------------------------- the worlds
def flat_world(g, key, X, m, b, frm, until, twins, query_seed, offset_seed, pq=None, query_rows=None):
    """A PQIndex over the codes of X -- by a quantizer trained on X, or by `pq` -- b noisy copies of rows of [frm, until)
    (of `query_rows`, where given), the odd ones excluding the row they were made from; the handle's distances
    [b][until - frm]; offsets with a tenth +inf, equal on twin rows."""
    n = len(X)
    dm = g.DeviceMatrix.from_host(X)
    try:
        pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(K, m, ITERS)) if pq is None else pq
        enc = pq.encode(dm)
    finally:
        dm.close()
    vi = g.PQIndex(pq, enc)
    if query_rows is None:
        Q, exclude = noisy_queries(query_seed, X, b, frm, until)
    else:
        Q, exclude = noisy_queries(query_seed, query_rows, b, 0, len(query_rows))[0], None
    ids = np.arange(frm, until)
    dist = distances_by_row(vi.batch_query_raw(len(ids), Q, frm, until), ids)
    offsets = draw_offsets(offset_seed, n, twins)
    twin = None
    if twins:   # (with one dimension to a quantizer a training pass can leave two equal rows in cells whose centroids
        #          differ, on the oracle as on the device: a twin pair is one whose distances are equal bits here)
        equal = [(a, c) for a, c in twins if np.array_equal(bits(dist[:, a - frm]), bits(dist[:, c - frm]))]
        twin = rank_ref.pick_twins(equal, exclude)
        offsets[list(twin)] = 0.25
    _FLAT[key] = {"vi": vi, "pq": pq, "enc": enc, "X": X, "Q": Q, "exclude": exclude, "dist": dist, "ids": ids,
                  "offsets": offsets, "twin": twin, "frm": frm, "until": until, "n": n, "m": m}
    return _FLAT[key]


def with_twins(X, twins):
    for a, c in twins:
        X[c] = X[a]
    return X


def big_world(g, m, b=19):
    """test_gpu_rank_flat.world: 4 300 unit rows, twenty of them copies, the range [70, n - 33), two row chunks."""
    if ("big", m, b) in _FLAT:
        return _FLAT[("big", m, b)]
    X = with_twins(unit_rows(5 * m + N, N, DIMENSIONS[m]), TWINS)
    w = flat_world(g, ("big", m, b), X, m, b, FROM, UNTIL, TWINS, m + b, m + 7 * b)
    w["offsets"][[3, N - 5]] = 0.0                               # finite, but outside the range
    w["outside"] = N - 5
    return w


def small_world(g, m, b=5):
    """test_gpu_offset_paths.world with eight twin pairs: 327 unit rows, the range [5, n - 3)."""
    if ("small", m, b) in _FLAT:
        return _FLAT[("small", m, b)]
    X = with_twins(unit_rows(7 * m + SMALL_N, SMALL_N, DIMENSIONS[m]), SMALL_TWINS)
    w = flat_world(g, ("small", m, b), X, m, b, 5, SMALL_N - 3, SMALL_TWINS, m + b, 3 * m + b)
    w["offsets"][2] = 0.0
    w["outside"] = 2
    return w


def tie_world(g):
    """test_gpu_offset_paths.tie_world: 6 407 rows, row r = base[r % 8], encoded by the small m = 16 quantizer; five
    noisy copies of base rows as queries, none excludes a row."""
    if "ties" in _FLAT:
        return _FLAT["ties"]
    base = unit_rows(61, 8, DIMENSIONS[16])
    return flat_world(g, "ties", base[np.arange(TIE_N) % 8], 16, 5, 5, TIE_N - 3, (), 62, 0, pq=small_world(g, 16)["pq"],
                      query_rows=base)


def tie_offsets(n, classes, seed):
    """One offset per class, a tenth of the rows masked."""
    rng = np.random.default_rng(seed)
    offsets = LEVELS[rng.permutation(8)[:classes]][np.arange(n) % classes]
    offsets[rng.random(n) < 0.1] = np.inf
    return offsets


def exact_world(g, n, d, frm, until, b):
    """test_gpu_rank_exact.world: unit rows, twenty of them copies, the handle over [frm, until), b noisy copies of rows
    of the range, the odd ones excluding the row they were made from."""
    key = (n, d, frm, until, b)
    if key not in _EXACT:
        X = with_twins(unit_rows(n + d, n, d), EXACT_TWINS)
        Q, exclude = noisy_queries(b + d, X, b, frm, until)
        dm = g.DeviceMatrix.from_host(X)
        ix = g.ExactIndex(dm, "l2", frm, until)
        ids = np.arange(frm, until)
        dist = distances_by_row(ix.batch_query_raw(until - frm, Q), ids)
        offsets = draw_offsets(n + b, n, EXACT_TWINS)
        twin = rank_ref.pick_twins(EXACT_TWINS, exclude)
        offsets[list(twin)] = 0.25
        _EXACT[key] = {"ix": ix, "dm": dm, "X": X, "Q": Q, "exclude": exclude, "dist": dist, "ids": ids, "frm": frm,
                       "until": until, "n": n, "offsets": offsets, "twin": twin, "outside": 0 if frm > 0 else None}
    return _EXACT[key]


def exact_tie_world(g):
    """The "ties" world of test_gpu_offset_paths.py: row r = base[r % 4], 17 noisy copies of base rows as queries."""
    if "ties" not in _EXACT:
        n, d, frm, until = 700, 33, 37, 695
        base = unit_rows(73, 4, d)
        X = base[np.arange(n) % 4]
        Q = noisy_queries(74, base, 17, 0, 4)[0]
        dm = g.DeviceMatrix.from_host(X)
        ix = g.ExactIndex(dm, "l2", frm, until)
        ids = np.arange(frm, until)
        _EXACT["ties"] = {"ix": ix, "dm": dm, "X": X, "Q": Q, "exclude": None, "ids": ids, "frm": frm, "until": until,
                          "n": n, "dist": distances_by_row(ix.batch_query_raw(until - frm, Q), ids)}
    return _EXACT["ties"]


def keys(w, offsets, dist=None):
    """t [b][len(ids)] as the query forms it: one float32 addition."""
    with np.errstate(invalid="ignore", over="ignore"):
        return ((w["dist"] if dist is None else dist) + offsets[w["ids"]][None, :]).astype(np.float32)


# ---------------------------------------------------------------- A, D: long gold lists
def long_cases(g, w, positions, lengths):
    """Three turns of rank_ref.plant_long and one with a twin pair, each with the reference's answer; asserted: the
    lengths 65 and more all occur, the best row sits past index 63 for four queries or more of every case, at indexes 0,
    63, 64 and beyond 127 in some, at a position beyond 63 and at the last one in some, and the reference ranks every
    best row at its chosen position.  With the twins both rows are listed, the copy first: the row is the lower id."""
    order = rank_ref.full_order(g, w, w["offsets"])
    plants = [rank_ref.plant_long(order, w, w["offsets"], w["outside"], positions, lengths, turn, seed=turn)
              for turn in range(3)]
    plants.append(rank_ref.plant_long(order, w, w["offsets"], w["outside"], positions, lengths, 1, w["twin"], seed=9))
    cases = []
    for gold, at, expect in plants:
        assert {n for n in lengths if n >= 65} <= {len(x) for x in gold} and (at >= 64).sum() >= 4
        want = rank_ref.reference(g, w, w["offsets"], gold)
        assert rank_ref.shows_long(want, order, expect)
        cases.append((gold, want))
    seats = np.concatenate([at for _, at, _ in plants[:3]])
    assert {0, 63, 64} <= set(seats.tolist()) and seats.max() >= 128
    chosen = [(q, e[0]) for _, _, expect in plants[:3] for q, e in enumerate(expect) if e is not None]
    assert any(p >= 64 for _, p in chosen) and any(p == len(order[q]) - 1 for q, p in chosen)
    a, c = w["twin"]
    gold, _, expect = plants[3]
    both = [q for q, x in enumerate(gold) if len(x) >= 2]
    assert a < c and len(both) >= 10
    for q in both:
        assert gold[q][0] == c and gold[q].index(a) > 0 and expect[q][1] == a and order[q][expect[q][0] + 1] == c
    return cases


@pytest.mark.parametrize("m", (16, 25))
def test_flat_long_gold_lists(g, m):
    """m = 16: one 16-byte word, eight slots; m = 25: seven 4-byte words, four slots.  Lists of 65, 129 and 300 rows take
    two, three and five trips of the wave's lane loop; the best row is found on lane 0 and lane 63 of the first trip, on
    lane 0 of the second, and on a later one."""
    assert flat_slots(m, 19)[4] == {16: 8, 25: 4}[m] and flat_chunks(FROM, UNTIL, 19, m)[1] == 2
    w = big_world(g, m)
    for gold, want in long_cases(g, w, POSITIONS, rank_ref.LONG_LENGTHS):
        rank_ref.same(ask(w, gold), want)


def tiles_of(b):
    return [(lo, min(lo + 16, b)) for lo in range(0, b, 16)]


def test_exact_long_gold_lists(g):
    """37 queries in tiles of 16, 16 and 5.  From gold_offsets alone: a tile with more than 512 pairs (three 256-slot
    steps and more), a list that straddles a step of its tile, an empty list between two others inside a tile."""
    from gulon_amd.ranks import gold_lists
    b, lengths = 37, (0, 1, 65, 300, 2, 0, 130)
    w = exact_world(g, 700, 40, 37, 695, b)
    cases = long_cases(g, w, (0, 64, 200, -1, 7), lengths)
    for gold, _ in cases:
        goff = gold_lists(gold, b)[0].astype(np.int64)
        tiles = tiles_of(b)
        assert tiles[-1] == (32, 37)                                             # the ragged tile of 5 queries
        assert any(goff[hi] - goff[lo] > 512 for lo, hi in tiles)
        assert any(goff[q + 1] > goff[q] and (goff[q] - goff[lo]) // 256 != (goff[q + 1] - 1 - goff[lo]) // 256
                   for lo, hi in tiles for q in range(lo, hi))
        assert any(goff[q] > goff[lo] and goff[q + 1] == goff[q] and goff[hi] > goff[q + 1]
                   for lo, hi in tiles for q in range(lo + 1, hi - 1))
    for gold, want in cases:
        rank_ref.same(ask(w, gold), want)


def test_exact_one_query_with_the_whole_range_as_its_list(g):
    """b = 1: a tile of one query with 658 pairs -- three steps all owned by slot 0 -- and with all but the first ten of
    its order."""
    w = exact_world(g, 700, 40, 37, 695, 1)
    o = rank_ref.full_order(g, w, w["offsets"])[0]
    everything = list(range(37, 695))
    want = rank_ref.reference(g, w, w["offsets"], [everything])
    assert (want[0][0], want[1][0], want[3][0]) == (0, o[0], len(o))
    rank_ref.same(ask(w, [everything]), want)
    rest = sorted(set(everything) - set(o[:10].tolist()))
    want = rank_ref.reference(g, w, w["offsets"], [rest])
    assert len(rest) == 648 and (want[0][0], want[1][0]) == (10, o[10])
    rank_ref.same(ask(w, [rest]), want)


def test_exact_long_lists_in_the_second_pass(g):
    """The shape of test_gpu_rank_exact.test_two_passes_and_chunks_of_three_row_groups: 4 100 queries (37, repeated)
    over 4 400 rows of 8 dimensions, 4 096 of them in the first pass.  Queries 4 090 .. 4 099 carry lists of 300 rows, all
    others one row: the second pass reads gk and gold_rows from pair 5 890 on.  The reference answers those ten
    differently when it is given the lists of queries 0 .. 9."""
    n, b, base = 4400, 4100, 37
    assert rank_ref.knn_row_chunks(0, n, 256) == (6, 3) and rank_ref.knn_row_chunks(0, n, 1) == (18, 1)
    w = exact_world(g, n, 8, 0, n, base)
    offsets = w["offsets"]
    order = rank_ref.full_order(g, w, offsets)
    single = [[int(o[q % 5])] for q, o in enumerate(order)]
    short = rank_ref.reference(g, w, offsets, single)
    assert short[0].tolist() == [q % 5 for q in range(base)]
    pick, tail = np.arange(b) % base, np.arange(4090, 4100)
    there = dict(w, dist=w["dist"][pick[tail]], exclude=w["exclude"][pick[tail]])
    their_order = [order[q] for q in pick[tail]]
    long_gold, at, expect = rank_ref.plant_long(their_order, there, offsets, None, (70, 3, 500, -1, 0), (300,), seed=5)
    long_want = rank_ref.reference(g, there, offsets, long_gold)
    assert rank_ref.shows_long(long_want, their_order, expect) and (at >= 64).sum() >= 4
    other = rank_ref.reference(g, there, offsets, [single[q] for q in pick[:10]])
    assert (other[1] != long_want[1]).all()
    gold = [single[q] for q in pick]
    want = tuple(a[pick].copy() for a in short)
    for i, q in enumerate(tail):
        gold[q] = long_gold[i]
    for part, theirs in zip(want, long_want):
        part[tail] = theirs
    assert sum(len(x) for x in gold[:4096]) == 4090 + 6 * 300
    rank_ref.same(w["ix"].batch_query_rank_raw(w["Q"][pick], gold, offsets, w["exclude"][pick]), want)


# ---------------------------------------------------------------- B, C: classes of equal keys
def test_flat_equal_keys_in_every_lane(g):
    """The gold list of a query: 130 candidates of one class of the tie world, shuffled -- every lane of rank_flat_gold
    holds the same key on all three trips, and the row id alone decides the reduction.  The answer is the list's smallest
    id; ahead of it are the candidates of strictly better classes and the lower ids of its own."""
    w = tie_world(g)
    ids = w["ids"]
    assert flat_chunks(5, TIE_N - 3, 5, 16)[1:] == (3, 34) and flat_slots(16, 5)[4] == 8
    offsets = tie_offsets(TIE_N, 8, 63)
    cand = np.isfinite(offsets[ids])
    t = keys(w, offsets)
    rng = np.random.default_rng(64)
    classes = [(3 * q + 1) % 8 for q in range(5)]
    gold = [rng.permutation(ids[cand & (ids % 8 == c)])[:130].tolist() for c in classes]
    want = rank_ref.reference(g, w, offsets, gold)
    nearest = [int(ids[np.argmin(np.where(cand, t[q], np.inf))]) % 8 for q in range(5)]
    assert nearest != classes
    for q, c in enumerate(classes):
        mine = np.array(gold[q])
        best = mine.min()
        assert len(mine) == 130 and mine[0] != best and len(set(bits(t[q, mine - 5]).tolist())) == 1
        own = cand & (ids % 8 == c)
        assert (bits(t[q, own]) == bits(t[q, best - 5])).all()
        assert want[1][q] == best and bits(want[2])[q] == bits(t[q, best - 5])
        assert want[0][q] == (cand & (t[q] < t[q, best - 5])).sum() + (own & (ids < best)).sum()
    rank_ref.same(ask(w, gold, offsets), want)


def tie_case(w, offsets, dist, gold, exclude, group_of):
    """What the counting scan meets for one query of a tie world whose gold list is the one row `gold`: the candidates
    with the gold row's key and a lower id, and those with a higher id -- 64 or more of each, the row groups they lie in
    are all there are, and the gold row's own group holds some of both.  -> how many candidates are ahead of the row."""
    ids = w["ids"]
    with np.errstate(invalid="ignore"):
        t = (dist + offsets[ids]).astype(np.float32)
    cand = np.isfinite(t) & (ids != exclude)
    mine = t[gold - ids[0]]
    equal = cand & (t == mine)
    ahead, behind = ids[equal & (ids < gold)], ids[equal & (ids > gold)]
    assert len(ahead) >= 64 and len(behind) >= 64
    assert set(group_of(np.concatenate([ahead, behind])).tolist()) == set(group_of(ids).tolist())
    assert (group_of(ahead) == group_of(gold)).any() and (group_of(behind) == group_of(gold)).any()
    return int((cand & (t < mine)).sum()) + len(ahead)


@pytest.mark.parametrize("excluding", (False, True))
def test_flat_tie_classes_in_the_counting_scan(g, excluding):
    """Ten queries on the tie world, each with one gold row: the member at the median id of a class -- every class once,
    then the best and the worst class of query 0.  Hundreds of candidates have the gold row's key: those with a lower id
    count, those with a higher do not, and they fill the three row chunks (the lower ids the first chunks, the higher
    ones the last, both the gold row's own).  excluding: every query excludes the lowest candidate of its gold class."""
    w = tie_world(g)
    ids = w["ids"]
    offsets = tie_offsets(TIE_N, 8, 63)
    cand = np.isfinite(offsets[ids])
    t0 = np.where(cand, keys(w, offsets)[0], np.nan)
    by_class = [t0[cand & (ids % 8 == c)][0] for c in range(8)]
    pick = np.array([c % 5 for c in range(8)] + [0, 0])
    classes = list(range(8)) + [int(np.argmin(by_class)), int(np.argmax(by_class))]
    b = len(pick)
    per_pass, chunks, per_chunk = flat_chunks(5, TIE_N - 3, b, 16)
    assert (chunks, per_chunk) == (3, 34) and flat_slots(16, b)[4] == 8 and per_pass >= b
    members = [ids[cand & (ids % 8 == c)] for c in classes]
    gold = [[int(x[len(x) // 2])] for x in members]
    exclude = np.array([int(x[0]) if excluding else -1 for x in members], np.int32)
    v = dict(w, dist=w["dist"][pick], exclude=exclude)
    want = rank_ref.reference(g, v, offsets, gold)
    ranks = [tie_case(w, offsets, v["dist"][q], gold[q][0], exclude[q], lambda r: r // 64 // per_chunk) for q in range(b)]
    assert want[0].tolist() == ranks and want[1].tolist() == [x[0] for x in gold]
    equal_ahead = [int((x < gold[q][0]).sum()) - int(excluding) for q, x in enumerate(members)]
    behind = len(members[9]) - int(excluding) - equal_ahead[9] - 1           # of the worst class: nothing else is behind
    assert ranks[8] == equal_ahead[8] and want[3][9] - ranks[9] - 1 == behind
    rank_ref.same(ask(w, gold, offsets, exclude if excluding else None, Q=w["Q"][pick]), want)


@pytest.mark.parametrize("excluding", (False, True))
def test_exact_tie_classes_in_the_counting_scan(g, excluding):
    """Four classes of equal rows, 17 queries, the gold row the member at the median id of class q % 4: the candidates
    with its key lie in all three 256-row groups, so equal keys meet inside a wave's ballot, between the waves of a
    workgroup and between row chunks (knn_row_chunks: three chunks of one group)."""
    w = exact_tie_world(g)
    ids, b = w["ids"], 17
    assert rank_ref.knn_row_chunks(37, 695, 2) == (3, 1)
    offsets = tie_offsets(700, 4, 75)
    cand = np.isfinite(offsets[ids])
    members = [ids[cand & (ids % 4 == q % 4)] for q in range(b)]
    gold = [[int(x[len(x) // 2])] for x in members]
    exclude = np.array([int(x[0]) if excluding else -1 for x in members], np.int32)
    v = dict(w, exclude=exclude)
    want = rank_ref.reference(g, v, offsets, gold)
    ranks = [tie_case(w, offsets, w["dist"][q], gold[q][0], exclude[q], lambda r: r // 256) for q in range(b)]
    assert want[0].tolist() == ranks and want[1].tolist() == [x[0] for x in gold]
    rank_ref.same(ask(w, gold, offsets, exclude if excluding else None), want)


# ---------------------------------------------------------------- E: slot counts
def every_kind(g, w):
    order = rank_ref.full_order(g, w, w["offsets"])
    for kind in rank_ref.KINDS:
        gold = rank_ref.plant(kind, order, w, w["offsets"], w["twin"], w["outside"])
        want = rank_ref.reference(g, w, w["offsets"], gold)
        assert rank_ref.shows(kind, want, order, w["twin"]), kind
        rank_ref.same(ask(w, gold), want)


@pytest.mark.parametrize("m", (3, 32, 80, 144))
def test_flat_slot_counts_the_lds_budget_forces(g, oracle, m):
    """b = 5.  m = 3: one 4-byte word, a 4 KiB table in a slot of the 8 KiB list minimum, E = 8 -- the counters
    [16][8][2] take 1 KiB of the first slot.  m = 32: two 16-byte words, E = 4, two workgroups.  m = 80 and 144: five and
    nine words, E = 1, five workgroups; at m = 144 the one slot is the whole budget.  The handle's distances are the
    oracle's, bit for bit."""
    assert flat_slots(m, 5) == SLOTS[m]
    vec, ng, m_pad, _, e = SLOTS[m]
    assert e * max(m_pad, 8) <= 144 and (e == 8 or 2 * e * m_pad > 144)
    assert (m == 3 and vec == 4 and ng == 1) or (vec == 16 and ng >= 2 and ceil_div(5, e) >= 2)
    w = small_world(g, m)
    n = SMALL_N
    oi, od, oc = oracle.pq_batch_query(w["vi"].indices(), DIMENSIONS[m], K, w["pq"].flat_centroids(), w["Q"], n)
    full = distances_by_row((oi, od, oc), np.arange(n))
    assert np.array_equal(bits(full[:, 5:n - 3]), bits(w["dist"]))
    every_kind(g, w)


@pytest.mark.parametrize("b", (2, 3))
def test_flat_slot_counts_a_small_batch_lowers(g, b):
    """m = 16 fits eight slots; a batch of 2 takes E = 2, a batch of 3 takes E = 4 with one idle zero-table slot."""
    assert flat_slots(16, b) == (16, 1, 16, 8, {2: 2, 3: 4}[b]) and (b == 2 or flat_slots(16, b)[4] - b == 1)
    every_kind(g, small_world(g, 16, b))


# ---------------------------------------------------------------- F: non-finite queries, flat
def test_flat_non_finite_queries(g):
    """One workgroup of eight slots, six queries: a NaN component, a +inf component, components of 1e19 (every distance
    overflows), components of 3e18 against offsets of 3e38 (finite + finite overflows), two ordinary ones.  The first
    three have no candidate; the fourth ranks among the rows with small offsets only."""
    w = small_world(g, 16, 6)
    n, vi = SMALL_N, w["vi"]
    assert flat_slots(16, 6)[4] == 8
    at = (0, 1, 2, 3)
    Q = nonfinite_queries(w["Q"], at)
    dist = distances_in_steps(lambda kk, f, u: vi.batch_query_raw(kk, Q, f, u), 5, n - 3,
                              vi.batch_query_raw(n - 8, Q, 5, n - 3))
    keepers = np.arange(8, n - 3, 8)
    offsets = huge_offsets(500, n, keepers)
    nf = dict(w, dist=dist)
    order = rank_ref.full_order(g, nf, offsets)
    assert [len(order[q]) for q in at[:3]] == [0, 0, 0] and 0 < len(order[3]) <= len(keepers)
    assert set(order[3].tolist()) <= set(keepers.tolist()) and len(order[4]) > len(keepers)
    gold = [[int(o[len(o) // 2]), int(keepers[1])] if len(o) else [int(keepers[1]), int(keepers[2])] for o in order]
    want = rank_ref.reference(g, nf, offsets, gold)
    assert all(rank_ref.unranked(want, q) for q in at[:3]) and (want[3][list(at[:3])] == 0).all()
    assert (want[0][3:] >= 0).all() and want[3][3] == len(order[3])
    rank_ref.same(ask(w, gold, offsets, Q=Q), want)


# ---------------------------------------------------------------- G: negative and signed-zero keys
def signed_cases(g, w, seed):
    """Offsets from SIGNED_LEVELS, -1.5 at every query's nearest candidate.  Gold at positions 0 and 1, at the first
    candidate whose key is not negative, and at the first candidate whose offset is -0.0; asserted on the reference:
    the first key of every query is negative, the third is not and at least one candidate is ahead of it, the fourth
    is the bits of the row's distance.

    A key is -0.0 only if the distance is: x + (-0.0) is x for every other x, and a distance is a sum of squares (or of
    table entries) from +0.0, never -0.0.  So no draw holds a candidate whose key is +0.0 beside one whose key is -0.0,
    and the count cannot depend on how the signs of zeros compare; what is asserted is that no key of the draw is zero."""
    ids, frm = w["ids"], w["frm"]
    offsets = plant_nearest(draw_offsets(seed, w["n"], levels=SIGNED_LEVELS), w["dist"], ids, w["exclude"], -1.5)
    in_range = offsets[ids]
    minus_zero = (in_range == 0) & np.signbit(in_range)
    assert (in_range[np.isfinite(in_range)] < 0).any() and minus_zero.any() and ((in_range == 0) & ~minus_zero).any()
    t = keys(w, offsets)
    assert (t[np.isfinite(t)] != 0).all()
    order = rank_ref.full_order(g, w, offsets)
    golds = {"at0": [], "at1": [], "not negative": [], "minus zero": []}
    for q, o in enumerate(order):
        mine = t[q, o - frm]
        turn = int(np.flatnonzero(mine >= 0)[0])
        zero = int(np.flatnonzero(minus_zero[o - frm])[0])
        assert mine[0] < 0 and 1 <= turn < len(o)
        for name, j in (("at0", 0), ("at1", 1), ("not negative", turn), ("minus zero", zero)):
            golds[name].append([int(o[j])])
    cases = []
    for name, gold in golds.items():
        want = rank_ref.reference(g, w, offsets, gold)
        assert want[1].tolist() == [x[0] for x in gold] and (want[0] >= 0).all()
        if name in ("at0", "at1"):
            assert (want[2] < 0).all() or name == "at1"
            assert want[0].tolist() == [int(name[2])] * len(gold)
        elif name == "not negative":
            assert (want[2] >= 0).all() and (want[0] >= 1).all()
        else:
            rows = want[1] - frm
            assert np.array_equal(bits(want[2]), bits(w["dist"][np.arange(len(rows)), rows]))
        cases.append((offsets, gold, want))
    return cases


def test_flat_negative_and_signed_zero_keys(g):
    w = big_world(g, 16)
    for offsets, gold, want in signed_cases(g, w, 416):
        rank_ref.same(ask(w, gold, offsets), want)


def test_exact_negative_and_signed_zero_keys(g):
    w = exact_world(g, 700, 40, 37, 695, 37)
    for offsets, gold, want in signed_cases(g, w, 719):
        rank_ref.same(ask(w, gold, offsets), want)


# ---------------------------------------------------------------- H: row base and context
def test_flat_row_base_and_context(g):
    """A handle at row base 1000 over the big m = 16 world's codes: gold rows and exclude are global ids, offsets are
    indexed by local row, the answer's row carries the base and nothing else moves; the host checks move with the base;
    the contexts of both handles answer as their handles.  The lists are the long ones, so rank_flat_gold subtracts the
    base on every lane, and every odd query lists its excluded row -- the nearest row by far, at offset 0: the reference
    answers that row once it is not excluded."""
    w = big_world(g, 16)
    ids, ex, b = w["ids"], w["exclude"], 19
    offsets = w["offsets"].copy()
    offsets[ex[ex >= 0]] = 0.0
    order = rank_ref.full_order(g, w, offsets)
    gold, at, expect = rank_ref.plant_long(order, w, offsets, w["outside"], POSITIONS, turn=2, seed=11)
    want = rank_ref.reference(g, w, offsets, gold)
    assert rank_ref.shows_long(want, order, expect) and (at >= 64).sum() >= 4
    moved = [[r + BASE for r in x] for x in gold]
    exclude = np.where(ex >= 0, ex + BASE, -1).astype(np.int32)
    based_want = g.rank_query_reference(w["dist"], offsets[ids], moved, exclude, rows=ids + BASE)
    listed = [q for q in range(b) if ex[q] >= 0 and ex[q] in gold[q]]
    unexcluded = g.rank_query_reference(w["dist"], offsets[ids], moved, None, rows=ids + BASE)
    assert len(listed) >= 6 and all(unexcluded[1][q] == exclude[q] != based_want[1][q] for q in listed)
    rank_ref.same(based_want, (want[0], np.where(want[1] >= 0, want[1] + BASE, -1), want[2], want[3]))
    based = g.PQIndex(w["pq"], w["enc"], row_base=BASE)
    contexts = []
    try:
        got = based.batch_query_rank_raw(w["Q"], moved, offsets, exclude, FROM, UNTIL)
        rank_ref.same(got, based_want)
        plain = ask(w, gold, offsets)
        rank_ref.same(plain, want)
        for name, bad in (("gold", BASE - 1), ("gold", BASE + N), ("exclude", 5)):
            lists, rows = [list(x) for x in moved], exclude.copy()
            if name == "gold":
                lists[3][1] = bad
                words = r"gold_rows\[%d\] = %d" % (sum(len(x) for x in lists[:3]) + 1, bad)
            else:
                rows[1] = bad
                words = r"exclude\[1\]"
            with pytest.raises(ValueError, match=words):
                based.batch_query_rank_raw(w["Q"], lists, offsets, rows, FROM, UNTIL)
        contexts = [based.context(), w["vi"].context()]
        rank_ref.same(contexts[0].batch_query_rank_raw(w["Q"], moved, offsets, exclude, FROM, UNTIL), got)
        rank_ref.same(contexts[1].batch_query_rank_raw(w["Q"], gold, offsets, ex, FROM, UNTIL), plain)
        rank_ref.same(based.batch_query_rank_raw(w["Q"], moved, offsets, exclude, FROM, UNTIL), got)
    finally:
        for c in contexts:
            c.close()
        based.close()


# ---------------------------------------------------------------- I: history
def test_flat_handle_history(g):
    """One m = 25 handle through: 19 queries with long lists over [70, n - 33); one query with an empty list; 40 queries
    over all rows with no offsets; an empty range; the first call again -- ordinary, offset and 3CosMul queries in
    between -- each answer equal to a fresh handle's over the same codes.  The empty range is one row chunk, the others
    two: part is strided anew over what the call before left, and bk, br, gk and the tables shrink and grow."""
    w = big_world(g, 25)
    assert [flat_chunks(*r, b, 25)[1] for r, b in (((FROM, UNTIL), 19), ((FROM, UNTIL), 1), ((0, N), 40),
                                                    ((64, 64), 19))] == [2, 2, 2, 1]
    order = rank_ref.full_order(g, w, w["offsets"])
    gold, _, expect = rank_ref.plant_long(order, w, w["offsets"], w["outside"], POSITIONS, seed=21)
    want = rank_ref.reference(g, w, w["offsets"], gold)
    assert rank_ref.shows_long(want, order, expect) and sum(len(x) for x in gold) > 1000
    rng = np.random.default_rng(22)
    Q40 = noisy_queries(23, w["X"], 40, 0, N)[0]
    gold40 = [rng.integers(0, N, q % 7 * 20).tolist() for q in range(40)]
    steps = [(w["Q"], gold, w["offsets"], w["exclude"], FROM, UNTIL),
             (w["Q"][:1], [[]], w["offsets"], w["exclude"][:1], FROM, UNTIL),
             (Q40, gold40, None, None, 0, N),
             (w["Q"], gold, w["offsets"], w["exclude"], 64, 64),
             (w["Q"], gold, w["offsets"], w["exclude"], FROM, UNTIL)]
    used = g.PQIndex(w["pq"], w["enc"])
    try:
        answers = []
        for step in steps:
            answers.append(used.batch_query_rank_raw(*step))
            used.batch_query_raw(5, w["Q"])
            used.batch_query_offset_raw(10, w["Q"][:3], w["offsets"])
            used.batch_query_cosmul_raw(5, [[(100, 1.0), (200, -1.0), (300, 1.0)]] * 3, FROM, UNTIL)
        for step, answer in zip(steps, answers):
            fresh = g.PQIndex(w["pq"], w["enc"])
            try:
                rank_ref.same(answer, fresh.batch_query_rank_raw(*step))
            finally:
                fresh.close()
    finally:
        used.close()
    rank_ref.same(answers[0], want)
    rank_ref.same(answers[4], want)
    assert (answers[1][0] == -1).all() and (answers[1][3] > 0).all() and (answers[3][3] == 0).all()
    assert (answers[2][3] == N).all() and (answers[2][0][1:7] >= 0).all()


def test_exact_handle_history(g):
    """One exact handle over 4 400 rows of 8 dimensions through: 19 queries with long lists; one query with an empty
    list; 2 000 queries with no offsets; an empty batch; the first call again -- ordinary, offset and 3CosMul queries in
    between -- each answer equal to a fresh handle's over the same rows.  An exact handle's range is fixed when it is
    made, so it is the batch that changes the grid: 2 and 1 query tiles scan 18 row chunks, 125 tiles scan 9."""
    n, base = 4400, 37
    w = exact_world(g, n, 8, 0, n, base)
    assert [rank_ref.knn_row_chunks(0, n, ceil_div(b, 16))[0] for b in (19, 1, 2000)] == [18, 18, 9]
    first = dict(w, dist=w["dist"][:19], exclude=w["exclude"][:19])
    order = rank_ref.full_order(g, first, w["offsets"])
    gold, _, expect = rank_ref.plant_long(order, first, w["offsets"], None, POSITIONS, seed=31)
    want = rank_ref.reference(g, first, w["offsets"], gold)
    assert rank_ref.shows_long(want, order, expect) and sum(len(x) for x in gold) > 1000
    pick = np.arange(2000) % base
    rng = np.random.default_rng(32)
    many = [[int(r)] for r in rng.integers(0, n, 2000)]
    steps = [(w["Q"][:19], gold, w["offsets"], first["exclude"]),
             (w["Q"][:1], [[]], w["offsets"], first["exclude"][:1]),
             (w["Q"][pick], many, None, None),
             (np.zeros((0, 8), np.float32), [], None, None),
             (w["Q"][:19], gold, w["offsets"], first["exclude"])]
    used = g.ExactIndex(w["dm"], "l2", 0, n)
    try:
        answers = []
        for step in steps:
            answers.append(used.batch_query_rank_raw(*step))
            used.batch_query_raw(5, w["Q"])
            used.batch_query_offset_raw(10, w["Q"][:3], w["offsets"])
            used.batch_query_cosmul_raw(5, [[(100, 1.0), (200, -1.0), (300, 1.0)]] * 3)
        for step, answer in zip(steps, answers):
            fresh = g.ExactIndex(w["dm"], "l2", 0, n)
            try:
                rank_ref.same(answer, fresh.batch_query_rank_raw(*step))
            finally:
                fresh.close()
    finally:
        used.close()
    rank_ref.same(answers[0], want)
    rank_ref.same(answers[4], want)
    assert rank_ref.unranked(answers[1], 0) and answers[1][3][0] > 0 and [len(a) for a in answers[3]] == [0, 0, 0, 0]
    assert (answers[2][3] == n).all() and (answers[2][1] == [x[0] for x in many]).all()
