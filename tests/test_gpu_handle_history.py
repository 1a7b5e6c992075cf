"""A used handle must answer like a fresh one: the sequences of handle_history.py played on ONE gulon_index.

A handle's scratch buffers grow and are never cleared, and a few host-side hints steer its later calls; here one handle
lives through large, peeled, short, empty, tied, non-finite, rejected, dropped, partial, re-tuned, decode and expression
calls, a small probe after each.  After every call the answer is the oracle's (same_answer, the rule of _check in
test_gpu_query.py), and for query calls it is, bit for bit, what a handle opened for that call alone returns.  The
conditions that keep this from being vacuous are checked without a GPU in test_handle_history.py."""
import ctypes as C

import numpy as np
import pytest

import handle_history as hh
import value_regimes as vr
from conftest import bits

pytestmark = pytest.mark.gpu

DEFAULTS = {"GULON_SCAN_FILTER": 1, "GULON_FILTER_ORDER": 1, "GULON_FILTER_MIN_RB": 512, "GULON_FILTER_PERIOD": 128,
            "GULON_FILTER_STAGE0": 0, "GULON_FILTER_STAGE1": 10, "GULON_FILTER_CAP": 32768,
            "GULON_FILTER_NADD": 0, "GULON_FILTER_SAMPLE": 65536}


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


@pytest.fixture
def tune(g):
    """Knobs for the handles created from now on (the environment) and for the ones already open (gulon_index_tuning)."""
    import os
    before = {k: os.environ.get(k) for k in DEFAULTS}
    g.tune_live(**hh.TUNE)
    yield g.tune_live
    g.tune_live(**DEFAULTS)
    for k, v in before.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


_PARTS = {}


def _parts(g, w):
    """(ProductQuantizer, EncodedMatrix) of a world, built once"""
    if w.name not in _PARTS:
        pq = g.ProductQuantizer.from_flat(w.k, w.d, w.m, w.cents)
        coder = pq.coder_factory(w.n)
        _PARTS[w.name] = (pq, g.EncodedMatrix(coder, [coder.build_code(w.idx[j]) for j in range(w.m)]))
    return _PARTS[w.name]


_NULL_FLAGS = {}


def _null_flags_entry(g, name):
    """gulon_index_batch_query / gulon_index_view_batch_query with a pointer type that takes NULL for out_flags"""
    if name not in _NULL_FLAGS:
        f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
        i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
        fn = getattr(C.CDLL(g.native.LIB_PATH), name)
        fn.restype = C.c_int32
        fn.argtypes = [C.c_void_p, f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, i32p, f32p, i32p, C.c_void_p]
        _NULL_FLAGS[name] = fn
    return _NULL_FLAGS[name]


def _query(g, ix, call, Q):
    """(idx [B][K], dist [B][K], count [B], flags [B] or None)"""
    if call.flags:
        return ix.batch_query_raw(call.K, Q, call.frm, call.until)
    entry = "gulon_index_view_batch_query" if isinstance(ix, g.PQIndexView) else "gulon_index_batch_query"
    b, k = call.B, call.K
    oi, od = np.zeros((b, max(k, 1)), np.int32), np.zeros((b, max(k, 1)), np.float32)
    oc = np.zeros(max(b, 1), np.int32)
    g.native.check(_null_flags_entry(g, entry)(ix._h, Q.reshape(-1) if b else np.zeros(1, np.float32), b, k, call.frm,
                                               call.until, oi.reshape(-1), od.reshape(-1), oc, None))
    return oi[:, :k], od[:, :k], oc[:b], None


class Player:
    """Plays calls on one handle and holds every answer against the oracle."""

    def __init__(self, g, oracle, w, ix, fresh=False, idmap=None):
        self.g, self.oracle, self.w, self.ix, self.fresh, self.idmap = g, oracle, w, ix, fresh, idmap
        self.must_replay = w.name in hh.BYTE_FORMS and idmap is None

    def _lists(self, call, Q, interleave=None):
        """gulon_index_scan_partial_dev, or the two halves of the bounded scan (lists = 1) with `interleave` between"""
        N = self.g.native
        L = N.lib()
        B, keff = call.B, call.K + 1
        dq, dv, di, db = (C.c_void_p() for _ in range(4))
        try:
            for p, size in ((dq, Q.nbytes), (dv, B * keff * 4), (di, B * keff * 4), (db, B * keff * 4)):
                N.check(L.gulon_dev_malloc(C.byref(p), size))
            N.check(L.gulon_memcpy_h2d(dq, Q.ctypes.data_as(C.c_void_p), Q.nbytes))
            args = (self.ix._h, dq, B, call.K, call.frm, call.until)
            if call.kind == "partial":
                N.check(L.gulon_index_scan_partial_dev(*args, dv, di, None))
            else:
                N.check(L.gulon_index_scan_bounds_dev(*args, db, None))
                if interleave is not None:
                    self.play(interleave)
                N.check(L.gulon_index_scan_partial_bounded_dev(*args, db, 1, dv, di, None))
            N.check(L.gulon_device_synchronize())
            v, i = np.zeros((B, keff), np.float32), np.zeros((B, keff), np.int32)
            N.check(L.gulon_memcpy_d2h(v.ctypes.data_as(C.c_void_p), dv, v.nbytes))
            N.check(L.gulon_memcpy_d2h(i.ctypes.data_as(C.c_void_p), di, i.nbytes))
            return v, i
        finally:
            N.check(L.gulon_device_synchronize())
            for p in (dq, dv, di, db):
                if p.value:
                    N.check(L.gulon_dev_free(p))

    def play(self, call):
        g, w, ix, oracle = self.g, self.w, self.ix, self.oracle
        want = hh.expected(oracle, w, call)
        if call.kind == "tuning":
            g.native.check(g.native.lib().gulon_index_tuning(ix._h, call.arg[0].encode(), call.arg[1]))
        elif call.kind == "rejected":
            Q = hh.queries(oracle, w, call)
            with pytest.raises(NotImplementedError if call.arg == "k" else ValueError):
                ix.batch_query_raw(call.K, Q, call.frm, call.until)
        elif call.kind == "decode_rows":
            vr.same_bits(ix.decode_rows(np.asarray(call.arg, np.int32)), want)
        elif call.kind == "query":
            Q = hh.queries(oracle, w, call)
            got = _query(g, ix, call, Q)
            hh.same_answer(got, want, must_replay=self.must_replay and call.K <= hh.MAX_K, idmap=self.idmap)
            if self.fresh:
                alone = g.PQIndex(*_parts(g, w))
                try:
                    hh.same_as_fresh(got, _query(g, alone, call, Q), want)
                finally:
                    alone.close()
        elif call.kind == "query_rows":
            got = ix.batch_query_rows_raw(call.K, np.asarray(call.arg, np.int32), call.frm, call.until)
            hh.same_answer(got, want, must_replay=self.must_replay and call.K <= hh.MAX_K, idmap=self.idmap)
        elif call.kind == "query_terms":
            exprs, extra = call.arg
            got = ix.batch_query_terms_raw(call.K, [list(e) for e in exprs], extra, call.frm, call.until)
            hh.same_terms(got, want)
        elif call.kind in ("partial", "bounded"):
            hh.same_partial(self._lists(call, hh.queries(oracle, w, call)), want)
        elif call.kind == "bounded_dropped":
            with pytest.raises(ValueError, match="must follow scan_bounds"):
                self._lists(call, hh.queries(oracle, w, call), interleave=hh.probes(w)[0])
        else:
            raise KeyError(call.kind)


def _report(g, e, message):
    """A failure names where it happened; a HIP runtime failure ends the session (nothing more runs on that device)."""
    if isinstance(e, g.native.GulonDeviceError):
        pytest.exit(f"device error -- {message}", returncode=3)
    raise AssertionError(message) from e


def _play(player, seq, where, only=None):
    """the whole sequence on the player's handle; a failure names the form, the sequence, the position and the call
    before it"""
    prev = None
    for pos, (label, call) in enumerate(seq):
        if only is not None and not only(call):
            continue
        try:
            player.play(call)
        except (Exception, pytest.fail.Exception) as e:
            _report(player.g, e, f"{where}: position {pos} ({label}) {call}\n  after {prev}\n  {type(e).__name__}: {e}")
        prev = (label, call)


@pytest.mark.parametrize("sequence", ["scripted"] + [f"seed{s}" for s in hh.SEEDS])
@pytest.mark.parametrize("form", list(hh.FORMS))
def test_one_handle_answers_like_a_fresh_one(oracle, g, tune, form, sequence):
    w = hh.world(form)
    ix = g.PQIndex(*_parts(g, w))
    try:
        _play(Player(g, oracle, w, ix, fresh=True), hh.sequences(w)[sequence], f"form {form}, sequence {sequence}")
    finally:
        ix.close()


def test_parent_and_context_take_the_calls_in_turn(oracle, g, tune):
    """An index and a context of it, each playing the full scripted sequence, alternately: two workspaces over one copy
    of the codes, neither sees the other's history."""
    w = hh.world("m16")
    ix = g.PQIndex(*_parts(g, w))
    ctx = ix.context()
    try:
        players = [Player(g, oracle, w, ix), Player(g, oracle, w, ctx)]
        prev = None
        for pos, (label, call) in enumerate(hh.scripted_sequence(w)):
            for who, player in zip(("parent", "context"), players):
                try:
                    player.play(call)
                except (Exception, pytest.fail.Exception) as e:
                    _report(g, e, f"m16 {who}: position {pos} ({label}) {call}\n  after {prev}\n  {type(e).__name__}: {e}")
            prev = (label, call)
    finally:
        ctx.close()
        ix.close()


def test_a_view_has_a_history_of_its_own(oracle, g, tune):
    """PQIndex.select over every third row plus a run of 300: the query kinds of the scripted sequence, in the view's
    positions, against the oracle on the gathered codes with the ids mapped through view.rows."""
    w = hh.world("m16")
    ix = g.PQIndex(*_parts(g, w))
    rows = hh.view_rows(w)
    view = ix.select(rows=rows)
    try:
        v = hh.gathered(w, rows, "m16-view")
        assert view.length == v.n and np.array_equal(view.rows, rows)
        _play(Player(g, oracle, v, view, idmap=view.rows), hh.scripted_sequence(v), "view of m16",
              only=lambda call: call.kind == "query")
    finally:
        view.close()
        ix.close()


@pytest.mark.parametrize("form", ["m16", "w1024"])
def test_a_sharded_index_has_no_memory(oracle, g, tune, form):
    """NodeShardedIndex over three shards on one device: the query kinds of the scripted sequence over the whole index
    (its entry takes no range), K <= 1000 -- equal to the unsharded fresh handle and to the oracle."""
    from gulon_amd.sharded import NodeShardedIndex
    w = hh.world(form)
    pq, enc = _parts(g, w)
    sx = NodeShardedIndex(pq, enc, [0, 0, 0])
    prev = None
    try:
        for pos, (label, call) in enumerate(hh.scripted_sequence(w)):
            if call.kind != "query" or (call.frm, call.until) != (0, w.n) or call.K > 1000:
                continue
            try:
                Q = hh.queries(oracle, w, call)
                res = sx.batch_query_raw(call.K, Q)
                alone = g.PQIndex(pq, enc)
                full = alone.batch_query_raw(call.K, Q)
                alone.close()
                want = hh.expected(oracle, w, call)
                # (a NaN query: the sharded entry reproduces the reference's answer at every code width, the unsharded
                # one on byte codes only -- on 16-bit codes it comes back empty, handle_history._answer)
                there = want.oc == want.ref_oc
                vr.same_bits(res[1][there], full[1][there], nan_by_position=True)
                assert np.array_equal(res[2][there], full[2][there])
                if w.k <= 256:     # wide codes: no exact replay across shards; ids agree wherever no tie was flagged
                    assert np.array_equal(res[0], full[0]) and np.array_equal(res[3], full[3])
                hh.same_answer(res, want._replace(oc=want.ref_oc))
            except (Exception, pytest.fail.Exception) as e:
                _report(g, e, f"sharded {form}: position {pos} ({label}) {call}\n  after {prev}\n  {type(e).__name__}: {e}")
            prev = (label, call)
    finally:
        sx.close()


# ---- grouped index ---------------------------------------------------------------------------------------------------
GROUPED_CALLS = [("query", 40, 63), ("query", 3, 1), ("query", 17, 10), ("lookup", 21, 0), ("query", 3, 1),
                 ("query", 40, 100), ("query", 3, 1), ("query", 17, 10), ("rows", 17, 10), ("query", 3, 63),
                 ("terms", 13, 10), ("query", 3, 1), ("query", 17, 100), ("query", 40, 1), ("query", 3, 10),
                 ("rows", 40, 63), ("query", 17, 10), ("terms", 5, 100), ("query", 3, 1), ("query", 40, 10),
                 ("query", 17, 63), ("lookup", 40, 0), ("query", 3, 100), ("query", 17, 1), ("query", 40, 63)]


def test_a_grouped_index_has_no_memory(oracle, g):
    """GroupedIndex at the by_group shape of value_regimes.GROUPED_PATHS: batches of 40, 3 and 17 queries at K = 63, 1,
    10 and 100 (above 63: the literal heaps), lookups, queries by row and expression queries between them, on one
    handle -- each equal to the oracle's grouped query, ids and order included."""
    from test_gpu_lookup import ref_lookup
    from gulon_amd.expressions import compose_reference
    assert {(b, k) for kind, b, k in GROUPED_CALLS if kind == "query"} == {(b, k) for b in (40, 3, 17) for k in (63, 1, 10, 100)}
    n, d, groups, m, k, limit, _ = vr.GROUPED_PATHS["by_group"]
    rng = np.random.default_rng(7)
    X = (rng.standard_normal((n, d)) + 3.0 * rng.integers(0, 4, (n, 1))).astype(np.float32)
    dm = g.DeviceMatrix.from_host(X)
    coarse = g.KMeans.compute_clusters(g.Vectors(dm), g.KMeansConfig(groups, 2))
    gv = g.group(dm, coarse)
    pq = g.ProductQuantizer.apply(gv.residuals, g.ProductQuantizerConfig(k, m, 2))
    index = g.Index.grouped(gv, pq, g.LimitGroups(limit))
    codes, cents = index.data.indices(), pq.flat_centroids()
    cache = {}

    def reference(Q, K):
        return oracle.grouped_query(codes, d, k, cents, gv.centroids, gv.offsets, Q, K, 0, limit)

    def same(got, want, where):
        assert np.array_equal(got[2], want[2]), where
        for q in range(len(want[2])):
            c = int(want[2][q])
            assert got[0][q, :c].tolist() == want[0][q, :c].tolist(), (where, q)
            assert np.array_equal(bits(got[1][q, :c]), bits(want[1][q, :c])), (where, q)

    prev = None
    try:
        for pos, (kind, B, K) in enumerate(GROUPED_CALLS):
            where = f"grouped: position {pos} {(kind, B, K)} after {prev}"
            r = np.random.default_rng([B, K, len(kind)])
            rows = r.integers(0, n, B).astype(np.int32)
            if kind == "query":
                if (B, K) not in cache:
                    Q = np.concatenate([X[r.integers(0, n, B - 1)], (r.standard_normal((1, d)) * 2).astype(np.float32)])
                    cache[B, K] = (Q, reference(Q, K))
                Q, want = cache[B, K]
                same(index.batch_query_raw(K, Q), want, where)
            elif kind == "lookup":
                assert np.array_equal(bits(index.lookup_rows(rows)),
                                      bits(ref_lookup(oracle, codes, d, k, cents, gv.centroids, gv.offsets, rows))), where
            elif kind == "rows":
                Q = ref_lookup(oracle, codes, d, k, cents, gv.centroids, gv.offsets, rows)
                same(index.batch_query_rows_raw(K, rows), reference(Q, K), where)
            else:
                exprs = [[(int(a), 1.0), (int(b) if b != a else (int(a) + 1) % n, -1.0)]
                         for a, b in zip(rows, r.integers(0, n, B))]
                Q = np.stack([compose_reference(ref_lookup(oracle, codes, d, k, cents, gv.centroids, gv.offsets,
                                                           [x for x, _ in e]), [x for _, x in e]) for e in exprs])
                ei, ed, ec = reference(Q, K + 2)
                oi, od, oc = index.batch_query_terms_raw(K, exprs, 2)
                for q, e in enumerate(exprs):
                    keep = [p for p in range(int(ec[q])) if int(ei[q, p]) not in {x for x, _ in e}][:K]
                    assert oc[q] == len(keep), (where, q)
                    assert oi[q, :len(keep)].tolist() == ei[q, keep].tolist(), (where, q)
                    assert np.array_equal(bits(od[q, :len(keep)]), bits(ed[q, keep])), (where, q)
            prev = (kind, B, K)
    finally:
        index.close()
