"""The reference side of test_gpu_group_select.py: which groups a grouped query searches, and in which order.

GroupedIndex.searchSpace (Index.scala:285-299) feeds every centroid's distance, in index order, through a TopKHeap of
capacity `limit` (LimitGroups) or g (LimitVectors), drains it with deleteAll and, for LimitVectors, walks the cumulative
row counts to the cut.  coarse_stage (grouped.hip) answers it with five kernels, only one of which is that heap; the
others sort by (distance, id) and flag the queries for which that order is not the heap's.  The hook
gulon_selftest_group_selection runs the stage alone; this module holds the plain numpy / Python reference and the cases.

  cdist_ref      MathUtils.distanceSq as an fp32 chain: dx = q_e - c_e, s = fl(s + fl(dx dx)), e ascending, unfused
  search_space   Index.scala:285-299 literally, on oracle/py_oracle.Heap
  sorted_order   (distance, id) order, NaN as +inf: what a level-1 query may show BEFORE its redo
  sorted_level   the level rule of the sorting kernels, restated (with and without the LimitVectors correction)
  tie_tags       where the (distance, id) order has equal neighbours: 'inside' (two searched entries), 'cut' (the last
                 searched entry and the first one left out), 'last2' (the last two searched entries), 'none'

Regimes: distinct (normal floats), pairs (every tenth centroid copied onto another id, half of the copies to a lower id
than their original, half to a higher one), lattice (integer coordinates in -2..2: small integer distances, many tie
classes), class (one centroid repeated T times), nan (one centroid with a NaN coordinate, one all-NaN query), inf (three
centroids with a coordinate of 1e20: their distance is inf; one query AT such a centroid, for which every other distance
is inf).  Queries are drawn from the centroids and from fresh points; in the tie regimes they are chosen among ~80
candidates so that the case holds a query of every tie structure it promises (Case.promise; asserted without a GPU in
test_group_select_ref_host.py).

LimitVectors cases share one data set per (g, regime) over five limits: 1, Lb, Lb + 1, n and n + 7.  Lb lies exactly on a
cumulative boundary of the reference's order for one query; in the tie regimes that query is one whose reference set
differs from the (distance, id) set with no tie at the cut -- the last two searched groups tie and the heap has the
larger one first (the failure gq_sorted_groups' level rule had to be corrected for).

What a name says: <path>-g<g>-<limit>-<regime>; path is the kernel the driver takes (kernel_path restates its dispatch):
nearest = gq_nearest_groups, sorted = gq_sorted_groups, select8 / select40 / select0 = gq_select_groups<KR>, lv = gq_sorted_groups
by rows, cdist = gq_cdist's shapes through the nearest path, unsupported = the LDS limit."""
import functools
from dataclasses import dataclass, field

import numpy as np

from oracle.py_oracle import Heap

f32 = np.float32
D = 6
ERR_UNSUPPORTED = -3
TIE_REGIMES = ("pairs", "lattice")


# ---- the reference ---------------------------------------------------------------------------------------------------
def cdist_ref(Q, C):
    """[B][g] float32: s = fl(s + fl(dx dx)) with dx = fl(q_e - c_e), e ascending (every numpy float32 operation rounds once)"""
    Q, C = np.asarray(Q, f32), np.asarray(C, f32)
    s = np.zeros((Q.shape[0], C.shape[0]), f32)
    with np.errstate(all="ignore"):
        for e in range(Q.shape[1]):
            dx = Q[:, e:e + 1] - C[None, :, e]
            s = s + dx * dx
    assert s.dtype == f32
    return s


def heap_order(cdist_q, cap):
    """exactNearestNeighbours(centroids, query, cap).deleteAll() (Index.scala:209-229, TopKHeap.scala)"""
    h = Heap(cap)
    for c, v in enumerate(cdist_q):
        h.update(c, v)
    return h.drain()[0]


def rows_cut(order, sizes, limit):
    """Index.scala:291-298: groups of `order` until they hold `limit` rows"""
    i = count = 0
    while i < len(order) and count < limit:
        count += int(sizes[order[i]])
        i += 1
    return i


def search_space(cdist_q, sizes, strategy, limit):
    if strategy == 0:
        return heap_order(cdist_q, limit)
    order = heap_order(cdist_q, len(cdist_q))
    return order[:rows_cut(order, sizes, limit)]


def sort_keys(cdist_q):
    with np.errstate(all="ignore"):
        return np.where(np.isnan(cdist_q), f32(np.inf), cdist_q).astype(f32)


def sorted_order(cdist_q):
    return np.lexsort((np.arange(len(cdist_q)), sort_keys(cdist_q)))


def sorted_cut(order, sizes, strategy, limit):
    return min(limit, len(order)) if strategy == 0 else rows_cut(order, sizes, limit)


def tie_tags(cdist_q, sizes, strategy, limit):
    """the tie structure of one query under the (distance, id) order and its cut"""
    o = sorted_order(cdist_q)
    v = sort_keys(cdist_q)[o]
    cnt = sorted_cut(o, sizes, strategy, limit)
    tags = set()
    if np.isnan(cdist_q).any():
        tags.add("nan")
    if (v[:cnt - 1] == v[1:cnt]).any():
        tags.add("inside")
    if cnt >= 2 and v[cnt - 2] == v[cnt - 1]:
        tags.add("last2")
    if cnt < len(o) and v[cnt - 1] == v[cnt]:
        tags.add("cut")
    if not tags:
        tags.add("none")
    return tags


def sorted_level(cdist_q, sizes, strategy, limit, corrected=True):
    """the level gq_sorted_groups / gq_select_groups give a query (grouped.hip), restated: 2 = the searched SET hangs on the
    heap's order (a NaN; a tie at the cut; LimitVectors: a tie between the last two searched -- `corrected`), 1 = only the
    ORDER does (any other tie among the searched), 0 = (distance, id) order is the heap's"""
    o = sorted_order(cdist_q)
    v = sort_keys(cdist_q)[o]
    cnt = sorted_cut(o, sizes, strategy, limit)
    level = 2 if np.isnan(cdist_q).any() else 0
    for e in range(min(cnt + 1, len(o)) - 1):
        if v[e] == v[e + 1]:
            level = max(level, 2 if e + 1 == cnt or (corrected and strategy == 1 and e + 2 == cnt) else 1)
    return level


def count_at_or_below(cdist_q, limit):
    """gq_select_groups' count: the entries whose key is at or below the limit-th smallest key (NaN keyed as +inf)"""
    keys = sort_keys(cdist_q).view(np.uint32)
    thr = np.sort(keys)[min(limit, len(keys)) - 1]
    return int((keys <= thr).sum())


def select_cap(limit):
    cap = 256
    while cap < limit + 128:
        cap *= 2
    return cap


def kernel_path(g, strategy, limit):
    """coarse_stage's dispatch (grouped.hip), restated"""
    if strategy == 0 and 1 <= limit <= 63:
        return "nearest"
    n2 = 64
    while n2 < g:
        n2 *= 2
    if n2 * 8 > 144 * 1024:
        return "unsupported"
    if strategy == 0 and 4 * limit <= g:
        return "select8" if g <= 2048 else "select40" if g <= 10240 else "select0"
    return "sorted"


def nn_stride(g, strategy, limit, sizes):
    n_empty = int((np.asarray(sizes) == 0).sum())
    return max(1, min(limit + (n_empty if strategy == 1 else 0), g))


# ---- cases -----------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    regime: str
    centroids: np.ndarray          # [g][d]
    sizes: np.ndarray              # [g] rows per group
    queries: np.ndarray            # [B][d]
    strategy: int                  # 0 LimitGroups, 1 LimitVectors
    limit: int
    promise: frozenset = frozenset()   # tie structures some query of the case must show (host test)
    claim: str = ""                # class cases: 'inside', 'cut', 'cap', 'cap1' -- about query 0
    expect_rc: int = 0
    shared: object = field(default=None, repr=False)   # LimitVectors: the data set's heap orders, shared over the limits

    @property
    def g(self):
        return len(self.centroids)

    @property
    def d(self):
        return self.centroids.shape[1]

    @property
    def b(self):
        return len(self.queries)

    @property
    def n(self):
        return int(self.sizes.sum())

    @property
    def offsets(self):
        return np.cumsum(self.sizes)[:-1].astype(np.int32)

    @property
    def path(self):
        return kernel_path(self.g, self.strategy, self.limit)


def _seed(*parts):
    h = 1469598103934665603
    for ch in "/".join(str(p) for p in parts).encode():
        h = ((h ^ ch) * 1099511628211) & ((1 << 64) - 1)
    return h


def make_centroids(regime, g, d, rng, T=0):
    if regime == "lattice":
        C = rng.integers(-2, 3, (g, d)).astype(f32)
    else:
        C = rng.standard_normal((g, d)).astype(f32)
    special = []
    if regime == "pairs" and g >= 2:
        npairs = max(1, g // 10)
        ids = rng.permutation(g)[:2 * npairs]
        a, b = np.minimum(ids[:npairs], ids[npairs:]), np.maximum(ids[:npairs], ids[npairs:])
        src = np.where(np.arange(npairs) % 2 == 0, b, a)      # even: the copy goes to the lower id
        dst = np.where(np.arange(npairs) % 2 == 0, a, b)
        C[dst] = C[src]
        special = dst.tolist()
    if regime == "class":
        ids = rng.permutation(g)[:T]
        C[ids] = C[ids[0]]
        special = [int(ids[0])]
    if regime == "nan":
        C[g // 2, min(1, d - 1)] = np.nan
    if regime == "inf":
        special = sorted({g // 4, g // 2, g - 1})
        C[special, 0] = f32(1e20)
        special = special[:1]
    return C, special


def make_candidates(regime, C, special, rng, ncand):
    """query candidates: the special centroids (a copy, the class centroid), other centroids, fresh points, interleaved"""
    g, d = C.shape
    finite = [c for c in range(g) if (np.abs(C[c]) < 1e19).all()]            # (not NaN, not a 1e20 coordinate)
    at = [c for c in special if regime != "inf"] + ([int(c) for c in rng.permutation(finite)[:ncand // 2]] if finite else [])
    if regime == "lattice":
        fresh = rng.integers(-2, 3, (ncand, d)).astype(f32)
    else:
        fresh = (rng.standard_normal((ncand, d)) * 1.5).astype(f32)
    out = []
    for i in range(ncand):
        if i < len(at):
            out.append(C[at[i]])
        out.append(fresh[i])
    return np.stack(out[:ncand]).astype(f32)


def pick_queries(cands, cd, sizes, strategy, limit, want, b, first=()):
    """`first`, then one candidate per wanted tag ('none' = only that tag), then the candidates in order: b queries"""
    chosen = list(first)
    tags = None
    if want:
        tags = [tie_tags(cd[i], sizes, strategy, limit) for i in range(len(cands))]
        for w in want:
            hit = [i for i in range(len(cands)) if w in tags[i] and i not in chosen]
            if w == "inside":                                   # strictly inside: no tie at the cut as well
                hit = [i for i in hit if "cut" not in tags[i]] or hit
            if hit:
                chosen.append(hit[0])
    for i in range(len(cands)):
        if len(chosen) >= b:
            break
        if i not in chosen:
            chosen.append(i)
    return chosen[:b]


def extras(regime, Q, C, special):
    """the regime's own queries, appended"""
    if regime == "nan":
        Q = np.concatenate([Q, np.full((1, Q.shape[1]), np.nan, f32)])
    if regime == "inf":
        Q = np.concatenate([Q, C[special[0]][None]])          # AT a centroid with a 1e20 coordinate
    return Q


def make_distinct(C, Q, rng):
    """the distinct regime's promise: thousands of float32 distances collide now and then -- redraw such centroids"""
    for _ in range(50):
        cd = cdist_ref(Q, C)
        bad = set()
        for q in range(len(Q)):
            o = np.argsort(cd[q], kind="stable")
            same = cd[q][o][1:] == cd[q][o][:-1]
            bad |= set(o[1:][same].tolist())
        if not bad:
            return C
        C[sorted(bad)] = rng.standard_normal((len(bad), C.shape[1])).astype(f32)
    raise AssertionError("distances stay tied")


def promise_for(regime, g, strategy, limit, designed=False):
    if regime not in TIE_REGIMES or g < 63:
        return frozenset()
    if strategy == 1 and limit == 1:
        return frozenset({"none"})
    if strategy == 0 and not 2 <= limit <= g - 8:             # (nearly every group searched: the cut sees the farthest few only)
        return frozenset({"none"}) if limit == 1 and regime == "lattice" else frozenset()
    if strategy == 1 and not designed:
        return frozenset()
    p = {"inside", "cut"}
    if (regime == "pairs" and strategy == 1) or limit <= 2:   # (beyond a few searched groups every query meets a tie)
        p.add("none")
    if strategy == 1:
        p.add("lv_set_differs")
    return frozenset(p)


def groups_case(name, regime, g, limit, b, d=D, T=0, claim=""):
    """a LimitGroups case: one row per group"""
    rng = np.random.default_rng(_seed("lg", regime, g, limit, d, T))
    C, special = make_centroids(regime, g, d, rng, T)
    cands = make_candidates(regime, C, special, rng, 80 if regime in TIE_REGIMES else b)
    sizes = np.ones(g, np.int64)
    promise = promise_for(regime, g, 0, limit)
    idx = pick_queries(cands, cdist_ref(cands, C) if promise else None, sizes, 0, limit, sorted(promise), b)
    Q = extras(regime, cands[idx], C, special)
    if regime == "distinct":
        C = make_distinct(C, Q, rng)
    return Case(name, regime, C, sizes, Q, 0, limit, promise, claim)


class VectorsData:
    """one LimitVectors data set: centroids, sizes, queries, the reference's full heap order per query, and Lb"""

    def __init__(self, regime, g, b):
        rng = np.random.default_rng(_seed("lv", regime, g))
        self.regime, self.g = regime, g
        self.C, special = make_centroids(regime, g, D, rng)
        kind = rng.integers(0, 3, g)
        sizes = np.where(kind == 0, 0, np.where(kind == 1, 1, rng.integers(150, 400, g)))
        if g >= 8:
            sizes[[0, 1, g // 2, g - 1]] = 0                    # empty groups at the front, in the interior, at the end
            sizes[[2, g // 2 + 1]] = [1, 300]
        elif g == 2:
            sizes[:] = [0, 5]
        else:
            sizes[:] = 3
        self.sizes = sizes.astype(np.int64)
        self.n = int(self.sizes.sum())
        cands = make_candidates(regime, self.C, special, rng, 80 if regime in TIE_REGIMES else b)
        cd = cdist_ref(cands, self.C)
        self.designed = False
        first = []
        self.Lb = None
        if regime in TIE_REGIMES and g >= 63:
            # a query whose reference set differs from the (distance, id) set with no tie at the cut, and the limit
            # (on a cumulative boundary of ITS reference order) at which it does
            tried = 0
            for i in range(len(cands)):
                o = sorted_order(cd[i])
                v = sort_keys(cd[i])[o]
                if not (v[:15] == v[1:16]).any() or tried >= 24:
                    continue
                tried += 1
                ref = heap_order(cd[i], g)
                cum = np.cumsum(self.sizes[ref])
                for j in range(1, min(16, g)):
                    L = int(cum[j - 1])
                    if L == 0 or (j >= 2 and cum[j - 2] == L):
                        continue
                    cnt = rows_cut(o, self.sizes, L)
                    if cnt >= 2 and set(o[:cnt].tolist()) != set(ref[:j]) and (cnt == g or v[cnt - 1] != v[cnt]) and \
                            min(self.sizes[o[cnt - 1]], self.sizes[o[cnt - 2]]) > 0:
                        self.Lb, first, self.designed = L, [i], True
                        break
                if self.designed:
                    break
            assert self.designed, (regime, g, "no query whose reference set differs from the sorted set")
        if self.Lb is None:
            ref = heap_order(cd[0], g)
            cum = np.cumsum(self.sizes[ref])
            self.Lb = max(1, int(cum[min(3, g) - 1]))
        if regime in TIE_REGIMES and g >= 63:                   # and one without any tie at LimitVectors(1)
            first += [i for i in range(len(cands)) if tie_tags(cd[i], self.sizes, 1, 1) == {"none"} and i not in first][:1]
        want = sorted(promise_for(regime, g, 1, self.Lb, self.designed) - {"lv_set_differs"})
        idx = pick_queries(cands, cd, self.sizes, 1, self.Lb, want, b, first)
        self.Q = extras(regime, cands[idx], self.C, special)
        if regime == "distinct":
            self.C = make_distinct(self.C, self.Q, rng)
        self.cdist = cdist_ref(self.Q, self.C)
        self._orders = {}

    def order(self, q):
        if q not in self._orders:
            self._orders[q] = heap_order(self.cdist[q], self.g)
        return self._orders[q]

    def limits(self):
        return {"one": 1, "Lb": self.Lb, "Lb1": self.Lb + 1, "n": self.n, "n7": self.n + 7}


@functools.lru_cache(maxsize=None)
def vectors_data(regime, g, b):
    return VectorsData(regime, g, b)


def vectors_case(name, regime, g, which, b):
    vd = vectors_data(regime, g, b)
    limit = vd.limits()[which]
    return Case(name, regime, vd.C, vd.sizes, vd.Q, 1, limit, promise_for(regime, g, 1, limit, vd.designed and which == "Lb"),
                shared=vd)


def example_case(name):
    """the four-group example: centroid distances [0, 1, 3, 3] of query 0, sizes [1, 3, 4, 100], LimitVectors(24)"""
    C = np.array([[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 1, 1]], f32)
    Q = np.array([[0, 0, 0, 0, 0, 0], [0.5, 0.25, 0, 0, 0, 1], [1, 1, 1, 1, 1, 1]], f32)
    return Case(name, "example", C, np.array([1, 3, 4, 100], np.int64), Q, 1, 24, frozenset({"lv_set_differs"}))


def unsupported_case(name, strategy, limit, rc):
    rng = np.random.default_rng(_seed(name))
    g = 16385
    C = rng.standard_normal((g, D)).astype(f32)
    Q = (rng.standard_normal((3, D)) * 1.5).astype(f32)
    C = make_distinct(C, Q, rng)
    return Case(name, "distinct", C, np.ones(g, np.int64), Q, strategy, limit, expect_rc=rc)


SELECT_SHAPES = [(256, 64), (2048, 64), (2048, 512), (1000, 128), (1000, 129), (2049, 64), (10240, 100), (10241, 64), (16384, 64)]
SORTED_SHAPES = [(100, 64), (255, 64), (300, 300), (300, 1000), (64, 64), (65, 64)]
VECTOR_GROUPS = [1, 2, 64, 65, 300, 2500]
VECTOR_B37 = ("lattice", 65)          # gq_literal_groups walks a query list of 37 with a grid of 16


def class_T(limit, claim):
    return {"inside": limit // 2, "cut": limit + 5, "cap": select_cap(limit), "cap1": select_cap(limit) + 1}[claim]


def _builders():
    B = {}
    for b in (1, 8, 9, 17):                                    # gq_cdist: the CD_Q = 8 tail, g around a workgroup, d
        for g in (1, 255, 257):
            for d in (1, 6, 33):
                B[f"cdist-b{b}-g{g}-d{d}"] = functools.partial(groups_case, regime="distinct", g=g, limit=1, b=b, d=d)
    for g in (1, 2, 63, 64, 65, 200):
        for limit in (1, 2, 63):
            for regime in ("distinct", "pairs", "lattice", "class", "nan", "inf"):
                T = max(1, min(g, limit + 1)) if regime == "class" else 0
                B[f"nearest-g{g}-{limit}-{regime}"] = functools.partial(groups_case, regime=regime, g=g, limit=limit, b=9, T=T)
    for g, limit in SORTED_SHAPES:
        for regime in ("distinct", "pairs", "lattice", "nan", "inf"):
            B[f"sorted-g{g}-{limit}-{regime}"] = functools.partial(groups_case, regime=regime, g=g, limit=limit, b=9)
    for g, limit in SELECT_SHAPES:
        path = kernel_path(g, 0, limit)
        b = 5 if g <= 2049 else 4
        for regime in ("distinct", "pairs", "nan", "inf"):
            B[f"{path}-g{g}-{limit}-{regime}"] = functools.partial(groups_case, regime=regime, g=g, limit=limit, b=b)
        for claim in ("inside", "cut", "cap", "cap1"):
            T = class_T(limit, claim)
            if T > g:                                          # (256, 64): cap + 1 = 257 entries do not exist
                continue
            B[f"{path}-g{g}-{limit}-class_{claim}"] = functools.partial(groups_case, regime="class", g=g, limit=limit, b=b, T=T,
                                                                         claim=claim)
    B["unsupported-g16385-64"] = functools.partial(unsupported_case, strategy=0, limit=64, rc=ERR_UNSUPPORTED)
    B["unsupported-g16385-vectors"] = functools.partial(unsupported_case, strategy=1, limit=100, rc=ERR_UNSUPPORTED)
    B["nearest-g16385-63-distinct"] = functools.partial(unsupported_case, strategy=0, limit=63, rc=0)
    for g in VECTOR_GROUPS:
        for regime in ("distinct", "pairs", "lattice", "nan", "inf"):
            b = 37 if (regime, g) == VECTOR_B37 else 9 if g <= 300 else 6
            for which in ("one", "Lb", "Lb1", "n", "n7"):
                B[f"lv-g{g}-{which}-{regime}"] = functools.partial(vectors_case, regime=regime, g=g, which=which, b=b)
    B["lv-example"] = example_case
    return B


BUILDERS = _builders()
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name](name)


@dataclass
class Ref:
    cdist: np.ndarray              # [B][g]
    space: list                    # per query: search_space, the reference's sequence
    order: list                    # per query: sorted_order (all g)
    tags: list                     # per query: tie_tags
    at_or_below: list              # per query: count_at_or_below (LimitGroups)
    distinct: np.ndarray           # per query: all g distances pairwise distinct and finite


@functools.lru_cache(maxsize=None)
def reference(name):
    """computed once per case and shared by the host test and both GPU runs; nothing changes it"""
    cs = case(name)
    cd = cs.shared.cdist if cs.shared is not None else cdist_ref(cs.queries, cs.centroids)
    space, order, tags, aob, distinct = [], [], [], [], []
    for q in range(cs.b):
        if cs.shared is not None:
            o = cs.shared.order(q)
            space.append(list(o[:rows_cut(o, cs.sizes, cs.limit)]))
        else:
            space.append(list(search_space(cd[q], cs.sizes, cs.strategy, cs.limit)))
        order.append(sorted_order(cd[q]))
        tags.append(tie_tags(cd[q], cs.sizes, cs.strategy, cs.limit))
        aob.append(count_at_or_below(cd[q], cs.limit) if cs.strategy == 0 else 0)
        distinct.append(bool(np.isfinite(cd[q]).all() and len(np.unique(cd[q])) == cs.g))
    return Ref(cd, space, order, tags, aob, np.array(distinct))


def sorted_space(cs, ref, q):
    """what the (distance, id) order searches"""
    o = ref.order[q]
    return [int(c) for c in o[:sorted_cut(o, cs.sizes, cs.strategy, cs.limit)]]
