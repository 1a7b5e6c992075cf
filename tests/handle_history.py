"""Call sequences for the handle-history tests: a used handle must answer like a fresh one.

A gulon_index handle owns about fifty scratch buffers that grow and are never cleared (DevBuf::ensure) and a few host
side hints that steer later calls (fb_hint, rp_hint, pend_*, last_filter_tiles, the knobs of gulon_index_tuning).  The
invariant the tests pin: the answer of a call depends on its arguments and the index, never on what the handle did
before.  This module holds what both test files share, and nothing of it needs a GPU:

    FORMS                         name -> (n, d, m, k): the smallest shape of each kernel family (value_regimes.FORMS)
                                  that still runs every filter stage under TUNE
    world(name)                   seeded code book and codes (random codes, flat code book, as _make of test_gpu_query.py)
                                  with PAIRS row pairs that share their codes
    Call                          one call on a handle, as a record; the constructors below build them
    scripted_sequence(w)          [(label, Call)]: the twelve named transitions T1 .. T12, a probe pair after each entry
    random_sequence(w, seed)      [(label, Call)]: 30 seeded draws from the same vocabulary, every third one a probe
    queries(oracle, w, call)      the query vectors of a query-like call
    expected(oracle, w, call)     the oracle's answer (cached per distinct call)
    same_answer(got, want)        the comparison rule of _check in test_gpu_query.py

test_handle_history.py checks, on the oracle alone, that the sequences are neither vacuous nor lenient;
test_gpu_handle_history.py plays them on one handle."""
import collections

import numpy as np

import replay_adversary as ra
import value_regimes as vr

TUNE = dict(GULON_FILTER_MIN_RB=4, GULON_FILTER_PERIOD=8, GULON_FILTER_STAGE0=1, GULON_FILTER_STAGE1=2,
            GULON_FILTER_SAMPLE=512)          # the thresholds of the `tune` fixture of test_gpu_filter.py
FORMS = {name: vr.FORMS[name] for name in ("m16", "m25", "m64", "k5", "w1024", "w5000")}
BYTE_FORMS = tuple(name for name, shape in FORMS.items() if shape[3] <= 256)
SEEDS = (1, 2, 3)
MAX_K, MAX_K_PEELED = 63, 8191
TIE, EXACT_REPLAY, NONFINITE = 3, 4, 8
INT_MAX = 2 ** 31 - 1

World = collections.namedtuple("World", "name n d m k cents idx pairs")
Call = collections.namedtuple("Call", "kind B K frm until qkind flags arg salt")
Answer = collections.namedtuple("Answer", "oi od oc tie ref_oc")     # tie[q]: two equal distances among the K + 1 smallest;
                                                                     # ref_oc: the oracle's counts where oc departs from them
Partial = collections.namedtuple("Partial", "pv pi sure")            # sure[q][e]: the distance is no one else's, so the id is
Terms = collections.namedtuple("Terms", "oi od oc operands K")       # the oracle at depth K + extra, before the drop

QUERY_LIKE = ("query", "partial", "bounded", "bounded_dropped", "query_rows", "query_terms")

_worlds, _queries, _expected = {}, {}, {}


# ---- worlds ----------------------------------------------------------------------------------------------------------
def make_world(name, n, d, m, k, seed):
    rng = np.random.default_rng(seed)
    cents = rng.standard_normal(k * d).astype(np.float32)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    rows = rng.permutation(n)[:2 * ra.PAIRS]
    a, b = np.sort(rows[:ra.PAIRS]), rows[ra.PAIRS:]
    idx[:, b] = idx[:, a]                                       # identical codes => exact distance ties
    return World(name, n, d, m, k, cents, np.ascontiguousarray(idx), tuple((int(x), int(y)) for x, y in zip(a, b)))


def world(name):
    if name not in _worlds:
        n, d, m, k = FORMS[name]
        _worlds[name] = make_world(name, n, d, m, k, [list(FORMS).index(name), n, d, m, k])
    return _worlds[name]


def gathered(w, rows, name):
    """The world of a view of `w` over `rows` (ascending): the gathered codes, the pairs that lie inside it."""
    rows = np.asarray(rows, np.int64)
    pos = {int(r): p for p, r in enumerate(rows)}
    pairs = tuple((pos[a], pos[b]) for a, b in w.pairs if a in pos and b in pos)
    return World(name, len(rows), w.d, w.m, w.k, w.cents, np.ascontiguousarray(w.idx[:, rows]), pairs)


def view_rows(w):
    """every third row plus one contiguous run of 300 rows"""
    run = np.arange(w.n // 2 + 1, w.n // 2 + 301)
    return np.union1d(np.arange(0, w.n, 3), run).astype(np.int32)


# ---- the vocabulary --------------------------------------------------------------------------------------------------
def _call(kind, B=0, K=0, rows=(0, 0), qkind=None, flags=True, arg=None, salt=0):
    return Call(kind, int(B), int(K), int(rows[0]), int(rows[1]), qkind, bool(flags), arg, int(salt))


def query(B, K, rows, qkind="gauss", flags=True, salt=0):
    return _call("query", B, K, rows, qkind, flags, None, salt)


def partial(B, K, rows, salt=0):
    return _call("partial", B, K, rows, "gauss", salt=salt)


def bounded(B, K, rows, salt=0):
    return _call("bounded", B, K, rows, "gauss", salt=salt)


def bounded_dropped(B, K, rows, salt=0):
    return _call("bounded_dropped", B, K, rows, "gauss", salt=salt)


def rejected(w, which):
    """frm > until, until > n, or K above GULON_MAX_K_PEELED"""
    rows, K = {"order": ((10, 5), 5), "length": ((0, w.n + 1), 5), "k": ((0, w.n), MAX_K_PEELED + 1)}[which]
    return _call("rejected", 1, K, rows, "gauss", arg=which)


def decode_rows(rows):
    return _call("decode_rows", len(rows), 0, arg=tuple(int(r) for r in rows))


def query_rows(w, K, rows, frm_until=None):
    return _call("query_rows", len(rows), K, frm_until or (0, w.n), arg=tuple(int(r) for r in rows))


def query_terms(w, K, expressions, extra, frm_until=None):
    arg = (tuple(tuple((int(r), float(x)) for r, x in e) for e in expressions), int(extra))
    return _call("query_terms", len(expressions), K, frm_until or (0, w.n), arg=arg)


def tuning(key, value):
    return _call("tuning", arg=(key, int(value)))


def full(w):
    return 0, w.n


def small_range(w):
    """three row blocks -- fewer than FILTER_MIN_RB = 4: the exact scan -- cut inside a 64-row block at both ends"""
    return 64 * 5 + 17, 64 * 8 - 9


def probes(w):
    return query(3, 1, vr.sub_range(w.n), salt=901), query(17, 10, full(w), salt=902)


def work(call):
    """the size of a call's per-query scratch: B * (K + 1) entries"""
    return call.B * (call.K + 1) if call.kind in QUERY_LIKE else 0


def _some_rows(w, count, seed):
    rng = np.random.default_rng([seed, w.n])
    return [0, w.n - 1, (w.n // 64) * 64 - 1] + rng.integers(0, w.n, count - 3).tolist()


def _some_terms(w, count, seed):
    """two distinct operands each: a - b, a + b, 0.3 a - 1.7 b"""
    rng = np.random.default_rng([seed, w.n, 7])
    out = []
    for q in range(count):
        a, b = (int(r) for r in rng.choice(w.n, 2, replace=False))
        out.append(((a, 1.0), (b, -1.0)) if q % 3 == 0 else ((a, 1.0), (b, 1.0)) if q % 3 == 1 else ((a, 0.3), (b, -1.7)))
    return out


def scripted_sequence(w):
    """[(label, Call)]: the transitions T1 .. T12 in order, the two probes after every entry."""
    first = query(40, 63, full(w), salt=1)
    entries = [
        ("T1 large filtered batch", first),
        ("T2 peeled batch", query(5, 200, full(w), salt=2)),
        ("T3 exact scan of a short range", query(17, 10, small_range(w), salt=3)),
        ("T4 empty range", query(4, 5, (100, 100), salt=4)),
        ("T4 K = 0", query(4, 0, full(w), salt=4)),
        ("T4 B = 0", query(0, 5, full(w), salt=4)),
        ("T5 tied batch of 40", query(40, 10, full(w), "tied", salt=5)),
        ("T5 tied batch, null flags", query(9, 10, full(w), "tied", flags=False, salt=5)),
        ("T6 tied batch of 1", query(1, 10, full(w), "tied", salt=6)),
        ("T7 nan", query(6, 10, full(w), "nan", salt=7)),
        ("T7 huge", query(6, 10, vr.sub_range(w.n), "huge", salt=7)),
        ("T8 rejected from > until", rejected(w, "order")),
        ("T8 rejected until > n", rejected(w, "length")),
        ("T8 rejected K", rejected(w, "k")),
        ("T8 bounded scan dropped", bounded_dropped(4, 3, full(w), salt=8)),
        ("T9 partial, K + 1 = 64", partial(11, 63, full(w), salt=9)),
        ("T9 bounded", bounded(11, 10, full(w), salt=9)),
        ("T10 filter off", tuning("GULON_SCAN_FILTER", 0)),
        ("T10 exact scan of a batch", query(40, 10, full(w), "rows", salt=10)),
        ("T10 filter on", tuning("GULON_SCAN_FILTER", 1)),
        ("T10 nadd 2", tuning("GULON_FILTER_NADD", 2)),
        ("T10 nadd 4", tuning("GULON_FILTER_NADD", 4)),
        ("T10 nadd 0", tuning("GULON_FILTER_NADD", 0)),
        ("T10 cap 128", tuning("GULON_FILTER_CAP", 128)),
        ("T10 queue overflow", query(24, 31, full(w), salt=11)),
        ("T10 cap 32768", tuning("GULON_FILTER_CAP", 32768)),
        ("T11 decode_rows", decode_rows(_some_rows(w, 21, 11))),
        ("T11 query_rows", query_rows(w, 10, _some_rows(w, 21, 12))),
        ("T11 query_terms", query_terms(w, 10, _some_terms(w, 13, 13), 2)),
        ("T12 the first call again", first),
    ]
    out = []
    for label, call in entries:
        out.append((label, call))
        out.extend(("probe", p) for p in probes(w))
    return out


def _draw(w, rng, salt, big):
    """one call of the vocabulary; big: a valid query-like call with at least 20 queries or a peeled K"""
    ranges = [full(w), vr.sub_range(w.n)] if big else [full(w), vr.sub_range(w.n), small_range(w), (70, 70)]
    rows = ranges[int(rng.integers(len(ranges)))]
    B = int(rng.choice([20, 24, 33, 40])) if big else int(rng.integers(1, 41))
    K = int(rng.choice([11, 31, 63, 64, 100, 200] if big else [1, 2, 10, 31, 63, 64, 100]))
    if K > MAX_K:
        B = min(B, 5 if not big else 20)
    kinds = ["query"] * 6 + ["partial", "bounded", "query_rows", "query_terms"]
    if not big:
        kinds += ["bounded_dropped", "rejected", "decode_rows", "tuning", "tuning"]
    kind = kinds[int(rng.integers(len(kinds)))]
    if kind == "query":
        qkind = ["gauss", "gauss", "rows", "tied", "nan", "huge"][int(rng.integers(6))]
        return query(B, K, rows, qkind, flags=bool(rng.integers(4)), salt=salt)
    if kind in ("partial", "bounded", "bounded_dropped"):
        K = min(K, MAX_K)
        return _call(kind, B, K, full(w) if kind != "partial" else rows, "gauss", salt=salt)
    if kind == "rejected":
        return rejected(w, ["order", "length", "k"][int(rng.integers(3))])
    if kind == "decode_rows":
        return decode_rows(_some_rows(w, B + 3, salt))
    if kind == "query_rows":
        return query_rows(w, K, _some_rows(w, B + 3, salt), rows)
    if kind == "query_terms":
        return query_terms(w, min(K, 61) if K <= MAX_K else K, _some_terms(w, B, salt), 2, rows)
    key, values = [("GULON_SCAN_FILTER", (0, 1)), ("GULON_FILTER_NADD", (0, 2, 4)),
                   ("GULON_FILTER_CAP", (128, 32768))][int(rng.integers(3))]
    return tuning(key, values[int(rng.integers(len(values)))])


def random_sequence(w, seed, length=30):
    """[(label, Call)]: positions 0, 3, 6, ... any call of the vocabulary, 1, 4, 7, ... a large valid batch, 2, 5, 8, ...
    one of the two probes in turn -- so a small call always follows a larger one, and a call that must raise is
    followed by a valid one."""
    rng = np.random.default_rng([seed, list(FORMS).index(w.name) if w.name in FORMS else 99])
    out = []
    for i in range(length):
        if i % 3 == 2:
            out.append(("probe", probes(w)[(i // 3) % 2]))
        else:
            out.append((f"draw {i}", _draw(w, rng, 1000 * seed + i, big=i % 3 == 1)))
    return out


def sequences(w):
    """name -> sequence: the scripted one and the three seeded ones"""
    return {"scripted": scripted_sequence(w), **{f"seed{s}": random_sequence(w, s) for s in SEEDS}}


# ---- query vectors ---------------------------------------------------------------------------------------------------
def decoded(oracle, w, rows):
    rows = np.asarray(rows, np.int64)
    if len(rows) == 0:
        return np.zeros((0, w.d), np.float32)
    return oracle.pq_decode(np.ascontiguousarray(w.idx[:, rows]), w.d, w.k, w.cents)


def _distinct(od, c):
    return len(np.unique(od[:c].view(np.uint32))) == c


def _gauss(oracle, w, B, depth, frm, until, rng):
    """B queries off the data whose `depth` smallest distances over [frm, until) are pairwise distinct: candidates that
    meet a duplicated pair (or two rows that round to one float32) among them are drawn again.  k5 has 625 distinct
    codes in 20 000 rows: every query ties there, none is rejected."""
    c = min(depth, until - frm)
    if B == 0 or c <= 1 or w.name == "k5":
        return rng.standard_normal((B, w.d)).astype(np.float32)
    kept = []
    while len(kept) < B:
        cand = rng.standard_normal((B + 8, w.d)).astype(np.float32)
        od = oracle.pq_batch_query(w.idx, w.d, w.k, w.cents, cand, depth, frm, until)[1]
        kept.extend(cand[q] for q in range(len(cand)) if _distinct(od[q], c))
    return np.stack(kept[:B])


def depth_of(call):
    """how many of the smallest distances the call's answer hangs on"""
    if call.kind == "query_terms":
        return call.K + call.arg[1]
    return call.K + 1 if call.kind in ("partial", "bounded", "bounded_dropped") else call.K


def queries(oracle, w, call):
    """[B][d] float32: the query vectors of a query-like call"""
    key = (w.name, call)
    if key in _queries:
        return _queries[key]
    rng = np.random.default_rng([call.salt, call.B, call.K, call.frm, call.until % 1000, w.n])
    B, frm, until = call.B, call.frm, call.until
    inside = 0 <= frm < until <= w.n
    if call.kind == "query_rows":
        Q = decoded(oracle, w, call.arg)
    elif call.kind == "query_terms":
        from gulon_amd.expressions import compose_reference
        Q = np.stack([compose_reference(decoded(oracle, w, [r for r, _ in e]), [x for _, x in e]) for e in call.arg[0]])
    elif call.qkind == "gauss":
        Q = _gauss(oracle, w, B, depth_of(call) + 1, frm, until, rng) if inside and call.kind != "rejected" \
            else rng.standard_normal((B, w.d)).astype(np.float32)
    elif call.qkind == "rows":
        lo, hi = (frm, until) if inside else (0, w.n)
        Q = decoded(oracle, w, rng.integers(lo, hi, B))
    elif call.qkind == "tied":
        pairs = [p for p in w.pairs if not inside or (frm <= p[0] < until and frm <= p[1] < until)]
        rows = [pairs[q % len(pairs)][0] for q in range(B)] if pairs else rng.integers(0, w.n, B)
        Q = decoded(oracle, w, rows)
    elif call.qkind in ("nan", "huge"):
        Q = rng.standard_normal((B, w.d)).astype(np.float32)
        if call.qkind == "nan":
            Q[B // 2, 3 % w.d] = np.nan
        else:
            Q[B // 3, :] = 1e30
    else:
        raise KeyError(call.qkind)
    _queries[key] = Q = np.ascontiguousarray(Q, np.float32)
    return Q


# ---- the oracle's answers --------------------------------------------------------------------------------------------
def _ties(od, oc, depth):
    """[B] bool: two equal distances (or a NaN) among the first min(depth, count) entries of each list"""
    out = np.zeros(len(oc), bool)
    for q in range(len(oc)):
        v = np.sort(od[q, :min(depth, oc[q])])
        out[q] = bool(np.isnan(v).any() or (len(v) > 1 and (v[1:] == v[:-1]).any()))
    return out


def _answer(oracle, w, Q, K, frm, until):
    """The oracle's answer, with the one documented departure of the library ("Non-finite distances" and the
    wide / peeled sections): the literal heap that reproduces the reference's answer to a NaN query runs on byte codes
    at K <= 63 only; on 16-bit codes and above 63 neighbours a NaN distance is never eligible, so a query with a NaN
    component comes back empty.  (All-+inf distances come in row order there: equal to the oracle up to the tie.)"""
    oi, od, ref_oc = oracle.pq_batch_query(w.idx, w.d, w.k, w.cents, Q, K, frm, until)
    oc = ref_oc.copy()
    if w.k > 256 or K > MAX_K:
        oc[np.isnan(Q).any(axis=1)] = 0
    with np.errstate(invalid="ignore"):
        deep = oracle.pq_batch_query(w.idx, w.d, w.k, w.cents, Q, K + 1, frm, until)
        return Answer(oi, od, oc, _ties(deep[1], deep[2], K + 1), ref_oc)


def _partial(oracle, w, Q, K, frm, until):
    """gulon_index_scan_partial_dev: the K + 1 smallest, ascending by (distance, row id), (+inf, INT32_MAX) after them"""
    keff = K + 1
    oi, od, oc = oracle.pq_batch_query(w.idx, w.d, w.k, w.cents, Q, keff, frm, until)
    deep = oracle.pq_batch_query(w.idx, w.d, w.k, w.cents, Q, keff + 1, frm, until)[1]
    pv = np.full((len(Q), keff), np.inf, np.float32)
    pi = np.full((len(Q), keff), INT_MAX, np.int32)
    sure = np.zeros((len(Q), keff), bool)
    for q in range(len(Q)):
        c = oc[q]
        order = np.lexsort((oi[q, :c], od[q, :c]))
        pv[q, :c], pi[q, :c] = od[q, :c][order], oi[q, :c][order]
        values, counts = np.unique(deep[q, :min(keff + 1, until - frm)], return_counts=True)
        sure[q, :c] = np.isin(pv[q, :c], values[counts == 1])
    return Partial(pv, pi, sure)


def expected(oracle, w, call):
    """the oracle's answer to one call; None for the calls that answer nothing (tuning) or must raise"""
    key = (w.name, call)
    if key in _expected:
        return _expected[key]
    if call.kind in ("tuning", "rejected"):
        out = None
    elif call.kind == "decode_rows":
        out = decoded(oracle, w, call.arg)
    else:
        Q = queries(oracle, w, call)
        if call.kind in ("query", "query_rows"):
            out = _answer(oracle, w, Q, call.K, call.frm, call.until)
        elif call.kind in ("partial", "bounded"):
            out = _partial(oracle, w, Q, call.K, call.frm, call.until)
        elif call.kind == "bounded_dropped":
            out = None
        else:
            depth = depth_of(call)
            oi, od, oc = oracle.pq_batch_query(w.idx, w.d, w.k, w.cents, Q, depth, call.frm, call.until)
            out = Terms(oi, od, oc, [{r for r, _ in e} for e in call.arg[0]], call.K)
    _expected[key] = out
    return out


# ---- comparisons -----------------------------------------------------------------------------------------------------
def _same_up_to_ties(rows, dist, orows):
    """_same_up_to_ties of test_gpu_query.py: an unreplayed tie may differ in WHICH rows of the last distance's tie group
    it holds and in the order inside a group; every row strictly below the last distance is in both, none twice"""
    rows, orows, dist = np.asarray(rows), np.asarray(orows), np.asarray(dist)
    with np.errstate(invalid="ignore"):
        inner = dist < dist[-1] if len(dist) else np.zeros(0, bool)
    assert set(rows[inner].tolist()) == set(orows[inner].tolist())
    assert len(set(rows.tolist())) == len(rows)


def same_answer(got, want, must_replay=False, idmap=None):
    """got = (idx, dist, count, flags or None) of a query call, want = the oracle's Answer.  Counts and distance bits are
    equal (NaN by position); ids are equal where the flags are 0 or carry EXACT_REPLAY, else equal up to the rows of a
    tie group.  A tie flag is set exactly where the oracle's K + 1 smallest hold two equal distances.  must_replay (a
    byte form at K <= 63 whose batches stay inside the replay's limits): every tie-flagged query was replayed.  idmap
    (a view): the oracle's positions -> the row ids the handle answers in."""
    oi, od, oc, of = got
    K = oi.shape[1]
    assert np.array_equal(oc, want.oc), (oc.tolist(), want.oc.tolist())
    for q in range(len(oc)):
        c = int(oc[q])
        vr.same_bits(od[q, :c], want.od[q, :c], nan_by_position=True)
        ids = want.oi[q, :c] if idmap is None else idmap[want.oi[q, :c]]
        finite = bool(np.isfinite(want.od[q, :c]).all())
        if of is None:
            exact = not want.tie[q]
        else:
            f = int(of[q])
            exact = f == 0 or bool(f & EXACT_REPLAY)
            if finite and not f & NONFINITE:
                if c == K:
                    assert bool(f & TIE) == bool(want.tie[q]), (q, f, bool(want.tie[q]))
                if must_replay and f & TIE:
                    assert f & EXACT_REPLAY, (q, f)
        if exact:
            assert oi[q, :c].tolist() == ids.tolist(), q
        else:
            _same_up_to_ties(oi[q, :c], od[q, :c], ids)


def same_partial(got, want):
    """(dist [B][K+1], idx [B][K+1]) of a partial scan against the oracle's Partial"""
    pv, pi = got
    vr.same_bits(pv, want.pv, nan_by_position=True)
    assert np.array_equal(pi[want.sure], want.pi[want.sure])
    assert np.array_equal(pi == INT_MAX, want.pi == INT_MAX)
    for q in range(len(pi)):
        live = pi[q][pi[q] != INT_MAX]
        assert len(set(live.tolist())) == len(live)


def same_terms(got, want, idmap=None):
    """gulon_index_query_terms against the oracle at depth K + extra with the operands dropped and the first K kept;
    (-1, +inf) after the last entry"""
    oi, od, oc, of = got
    for q in range(len(oc)):
        keep = [p for p in range(int(want.oc[q])) if int(want.oi[q, p]) not in want.operands[q]][:want.K]
        c = len(keep)
        assert oc[q] == c, (q, int(oc[q]), c)
        vr.same_bits(od[q, :c], want.od[q, keep], nan_by_position=True)
        assert (oi[q, c:] == -1).all() and np.isposinf(od[q, c:]).all(), q
        ids = want.oi[q, keep] if idmap is None else idmap[want.oi[q, keep]]
        f = int(of[q])
        if f == 0 or f & EXACT_REPLAY:
            assert oi[q, :c].tolist() == ids.tolist(), (q, f)
        else:
            _same_up_to_ties(oi[q, :c], od[q, :c], ids)


def same_as_fresh(used, fresh, want):
    """A query call on the used handle against the same call on a fresh one: idx, dist and count bit for bit; flags
    equal apart from EXACT_REPLAY on queries whose ids are the oracle's already (the road may differ, the answer not)."""
    assert np.array_equal(used[2], fresh[2])
    assert np.array_equal(used[0], fresh[0])
    assert np.array_equal(np.ascontiguousarray(used[1]).view(np.uint32), np.ascontiguousarray(fresh[1]).view(np.uint32))
    if used[3] is None or fresh[3] is None:
        return
    differ = np.flatnonzero(used[3] != fresh[3])
    for q in differ:
        assert (int(used[3][q]) ^ int(fresh[3][q])) == EXACT_REPLAY, (q, int(used[3][q]), int(fresh[3][q]))
        c = int(want.oc[q])
        assert used[0][q, :c].tolist() == want.oi[q, :c].tolist(), q


# ---- what the replay has to carry (test_handle_history.py) ------------------------------------------------------------
def replay_load(oracle, w, q, K, frm, until):
    """(insertions, candidates) of one query over [frm, until): the reference heap's successful insertions
    (replay_adversary.insertions), and an upper bound of the rows the replay collects -- the insertions of its first
    level (the first L0_ROWS rows from the range's first row block) plus every later row at or below that level's K-th
    smallest distance: a segment seeded with level 0's bound lets nothing else through."""
    dist = ra.distances(oracle, w.cents, w.idx, w.d, w.m, w.k, q)[frm:until]
    ins = ra.insertions(dist, K)
    l0 = max(0, ra.L0_ROWS - frm % 64)
    head, tail = dist[:l0], dist[l0:]
    if len(head) < K or len(tail) == 0:
        return ins, ins
    bound = np.sort(head)[K - 1]
    return ins, ra.insertions(head, K) + int((tail <= bound).sum())
