"""The stream contract of every device-pointer entry point of include/gulon_hip.h (helpers: stream_contract.py).

Completeness: the header's functions with a `void *stream` parameter are exactly the keys of TABLE.
Kind A (test_behind_pending_work): the call's work is enqueued on the caller's stream.  The reference of a case is the
same entry point with stream = NULL on a fresh handle, everything synchronised around it (and the host-pointer form
where there is one), so nothing here needs the CPU oracle: the arithmetic is pinned elsewhere.
Kind B (test_two_streams_one_handle): two calls on one handle on two independent streams are ordered on the device.

Run with -s to see, per case, the warm call's return time and the delay it was given."""
import ctypes as C
import functools

import numpy as np
import pytest

import stream_contract as sc
from stream_contract import F_FILL, I_FILL, Case, Handle

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
FILTER_TUNING = ((b"GULON_FILTER_MIN_RB", 4), (b"GULON_FILTER_PERIOD", 8), (b"GULON_FILTER_STAGE0", 1),
                 (b"GULON_FILTER_STAGE1", 2), (b"GULON_FILTER_SAMPLE", 512))      # test_gpu_filter.tune's thresholds

# device-pointer entry points WITHOUT a stream parameter: they work on the null stream by contract (the header says so)
NULL_STREAM_BY_CONTRACT = {"gulon_index_select_mask_dev", "gulon_index_view_rows_dev", "gulon_dataset_pair_moment_dev"}


def G():
    import gulon_amd
    return gulon_amd


def NL():
    from gulon_amd import native as N
    return N, N.lib()


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert G().native.device_count() >= 1
    return t


@pytest.fixture(scope="module")
def delay(torch):
    return sc.Delay(torch)


# ---------------------------------------------------------------- worlds: host data, built once; handles are made fresh
@functools.lru_cache(maxsize=None)
def flat_world(n, d, m, k, seed, dup=0, scale=1.0):
    g = G()
    rng = np.random.default_rng(seed)
    cents = (rng.standard_normal(k * d) * scale).astype(np.float32)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    if dup:
        idx[:, -dup:] = idx[:, :dup]
    return {"n": n, "d": d, "m": m, "k": k, "cents": cents, "idx": idx, "parts": _parts(g, cents, idx, k, d, m)}


def _parts(g, cents, idx, k, d, m):
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    coder = pq.coder_factory(idx.shape[1])
    return pq, g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(m)])


def decoded(w, rows):
    """ProductQuantizer.decode of rows of a flat world, on the host (a gather: no arithmetic)"""
    fr, un = G().subvector_bounds(w["d"], w["m"])
    out = np.zeros((len(rows), w["d"]), np.float32)
    for j, (f, u) in enumerate(zip(fr, un)):
        book = w["cents"][w["k"] * f: w["k"] * u].reshape(w["k"], u - f)
        out[:, f:u] = book[w["idx"][j, rows]]
    return out


def flat_maker(w, tuning=(), context=False, view=None, lo=0, hi=None, dataset=None, fine=None):
    def make():
        g = G()
        N, L = NL()
        if lo or hi is not None:                 # a row shard
            ix = g.PQIndex(*_parts(g, w["cents"], w["idx"][:, lo:hi], w["k"], w["d"], w["m"]), row_base=lo)
        else:
            ix = g.PQIndex(*w["parts"])
        for key, v in tuning:
            N.check(L.gulon_index_tuning(ix._h, key, v))
        keep, top, more = [ix], ix, {}
        if context:
            top = ix.context()
            keep.insert(0, top)
        if view is not None:
            top = ix.select(rows=view)
            keep.insert(0, top)
        if dataset is not None:
            dm = g.DeviceMatrix.from_host(dataset)
            keep.append(dm)
            more["ds"] = dm._h
        if fine is not None:
            fx = g.PQIndex(*fine["parts"])
            keep.append(fx)
            more["fine"] = fx._h
        return Handle(top._h, keep, ix=ix, **more)
    return make


PLAIN = (20000, 64, 16, 256, 1)                  # n, d, m, k, seed
# 101 code blocks: three row chunks in the cosmul and offset scans; rows of about unit length, so that 3CosMul's
# (1 + cos) / 2 is not clamped to 0 everywhere
LOOKUP = (6407, 32, 16, 256, 2, 0, 32 ** -0.5)
GROUPED = dict(n=6000, d=16, m=4, B=16)
EXACT_N, EXACT_D = 700, 33


@functools.lru_cache(maxsize=None)
def grouped_world(k, groups=20):
    g = G()
    n, d, m = GROUPED["n"], GROUPED["d"], GROUPED["m"]
    rng = np.random.default_rng(40 + k + groups)
    cents = rng.standard_normal(k * d).astype(np.float32)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    sizes = [n // (groups - 2)] * groups
    sizes[2] = sizes[11] = 0                      # two empty groups
    sizes[0] += n - sum(sizes)
    assert sum(sizes) == n and min(sizes[0], sizes[-1]) > 0
    offsets = np.cumsum(sizes)[:-1].astype(np.int32)
    gc = (rng.standard_normal((groups, d)) * 3).astype(np.float32)
    vectors = rng.standard_normal((n, d)).astype(np.float32)
    return {"n": n, "d": d, "m": m, "k": k, "parts": _parts(g, cents, idx, k, d, m), "gc": gc, "offsets": offsets,
            "vectors": vectors, "groups": groups, "empty": 2}


def grouped_maker(k=16, fine=None, groups=20):
    def make():
        g = G()
        w = grouped_world(k, groups)
        gx = g.GroupedIndex(*w["parts"], w["gc"], w["offsets"], g.LimitGroups(3))
        dm = g.DeviceMatrix.from_host(w["vectors"])
        keep, more = [gx, dm], {}
        if fine is not None:
            fx = g.PQIndex(*fine["parts"])
            keep.append(fx)
            more["fine"] = fx._h
        return Handle(gx._h, keep, ds=dm._h, **more)
    return make


@functools.lru_cache(maxsize=None)
def exact_world():
    X = np.random.default_rng(7).standard_normal((EXACT_N, EXACT_D))
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)      # unit rows, as 3CosMul expects


def exact_maker():
    def make():
        g = G()
        dm = g.DeviceMatrix.from_host(exact_world())
        ex = g.ExactIndex(dm)
        return Handle(ex._h, [ex, dm], ds=dm._h)
    return make


def dataset_maker(X):
    def make():
        dm = G().DeviceMatrix.from_host(X)
        return Handle(dm._h, [dm], ds=dm._h)
    return make


def free_maker():
    return lambda: Handle(None, [])


# ---------------------------------------------------------------- shared pieces of the cases
def query_outs(B, K, flags=True, dist="dist", fill=F_FILL):
    o = {"idx": ((B, K), np.int32, I_FILL), dist: ((B, K), np.float32, fill), "count": ((B,), np.int32, I_FILL)}
    if flags:
        o["flags"] = ((B,), np.int32, I_FILL)
    return o


def host_buffers(outs):
    return {k: np.full(shape, fill, dtype=dt) for k, (shape, dt, fill) in outs.items()}


def flat_row_error(H):
    N, L = NL()
    v = C.c_int32(-1)
    N.check(L.gulon_index_row_error(H.h, C.byref(v)))
    return v.value


def grouped_row_error(H):
    N, L = NL()
    v = C.c_int32(-1)
    N.check(L.gulon_grouped_index_row_error(H.h, C.byref(v)))
    return v.value


def filter_tiles(H):
    N, L = NL()
    t, r = C.c_int32(-1), C.c_int32(-1)
    N.check(L.gulon_index_filter_stats(H.h, C.byref(t), C.byref(r)))
    return t.value


def two_queries(seed, B, d, scale=1.0):
    rng = np.random.default_rng(seed)
    return tuple((rng.standard_normal((B, d)) * scale).astype(np.float32) for _ in range(2))


def csr_terms(seed, b, n, cosmul=False, max_terms=3):
    """b expressions of 1 .. max_terms terms over rows [0, n): the same offsets, two sets of rows and weights"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, max_terms + 1, b)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    T = int(off[-1])
    sets = []
    for _ in range(2):
        rows = rng.integers(0, n, T).astype(np.int32)
        if cosmul:
            w = rng.choice(np.array([1.0, -1.0], np.float32), T)
            w[off[:-1]] = 1.0                      # a positive term per expression
        else:
            w = (rng.standard_normal(T) + 2).astype(np.float32)
        sets.append((rows, w.astype(np.float32)))
    return off, sets


def term_ins(off, sets):
    return {"off": (off, off), "rows": (sets[0][0], sets[1][0]), "w": (sets[0][1], sets[1][1])}


def spoil_entry(name, index, value):
    def spoil(ins):
        ins = dict(ins)
        a = ins[name].copy()
        a.reshape(-1)[index] = value
        ins[name] = a
        return ins
    return spoil


def mask_refused(outs):
    """refine forms: a query with count -1 has its other outputs undefined"""
    outs = {k: v.copy() for k, v in outs.items()}
    bad = outs["count"] == -1
    outs["idx"][bad] = 0
    outs["dist"][bad] = 0
    return outs


# ---------------------------------------------------------------- cases: flat index queries
def batch_query_case(name, make, Qs, K, n, check_ref=None, entry="gulon_index_batch_query_dev",
                     host_entry="gulon_index_batch_query", frm=0, until=None):
    B = len(Qs[0])
    until = n if until is None else until
    outs = query_outs(B, K)

    def call(H, p, st, host):
        return getattr(NL()[1], entry)(H.h, p["q"], B, K, frm, until, p["idx"], p["dist"], p["count"], p["flags"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        assert getattr(NL()[1], host_entry)(H.h, ins["q"].reshape(-1), B, K, frm, until, o["idx"].reshape(-1),
                                            o["dist"].reshape(-1), o["count"], o["flags"]) == 0
        return o
    return Case(name, (entry,), make, {"q": Qs}, outs, call, host_form, check_ref=check_ref)


def plain_scan():
    w = flat_world(*PLAIN)
    return batch_query_case("plain scan", flat_maker(w), two_queries(11, 40, w["d"]), 10, w["n"],
                            check_ref=lambda H, ref: _expect(filter_tiles(H) == 0, "took the filter"))


def filtered_scan():
    w = flat_world(*PLAIN)
    return batch_query_case("filtered scan", flat_maker(w, FILTER_TUNING), two_queries(12, 40, w["d"]), 10, w["n"],
                            check_ref=lambda H, ref: _expect(filter_tiles(H) > 0, "did not take the filter"))


def _expect(ok, what):
    assert ok, "this case is named after a path it " + what


TIES = (20000, 64, 16, 256, 3, 5000)


def tie_queries():
    w = flat_world(*TIES)
    return w, (decoded(w, np.arange(10, 4000, 350)), decoded(w, np.arange(77, 4000, 350)))    # 12 queries each


def tie_replay():
    w, Qs = tie_queries()

    def check(H, ref):
        _expect(((ref["flags"] & 3) != 0).all() and ((ref["flags"] & 4) != 0).all(), "did not replay every query")
    return batch_query_case("tie replay", flat_maker(w), Qs, 10, w["n"], check_ref=check)


def nonfinite_pass():
    w = flat_world(*PLAIN)
    Qr, Qd = two_queries(13, 8, w["d"])
    Qr[1, 7], Qr[3, :] = np.nan, 1e30
    Qd[2, 5], Qd[4, :] = np.nan, 1e30
    return batch_query_case("non-finite literal pass", flat_maker(w), (Qr, Qd), 10, w["n"],
                            check_ref=lambda H, ref: _expect(ref["flags"][1] & 8 and ref["flags"][3] & 8, "did not flag"))


def peeled_k100():
    w = flat_world(*PLAIN)
    return batch_query_case("peeled K = 100", flat_maker(w), two_queries(14, 5, w["d"]), 100, w["n"])


WIDE = (20000, 64, 16, 1024, 4)


def wide_codes(K):
    w = flat_world(*WIDE)
    return batch_query_case(f"wide codes K = {K}", flat_maker(w), two_queries(15 + K, 6, w["d"]), K, w["n"])


def wide_filter():
    w = flat_world(40000, 64, 16, 1024, 5)         # test_gpu_wide.py: 8 queries per entry
    rng = np.random.default_rng(16)
    Qs = tuple(np.concatenate([decoded(w, rng.integers(0, w["n"], 19)), rng.standard_normal((2, w["d"]))])
               .astype(np.float32) for _ in range(2))
    return batch_query_case("wide filter", flat_maker(w, ((b"GULON_FILTER_MIN_RB", 4),)), Qs, 10, w["n"],
                            check_ref=lambda H, ref: _expect(filter_tiles(H) > 0, "did not take the filter"))


def context_handle():
    w = flat_world(*PLAIN)
    return batch_query_case("context handle", flat_maker(w, context=True), two_queries(17, 40, w["d"]), 10, w["n"])


# ---------------------------------------------------------------- cases: the sharded pieces
def partial_outs(B, K):
    return {"pd": ((B, K + 1), np.float32, F_FILL), "pi": ((B, K + 1), np.int32, I_FILL)}


def scan_partial_case(lo=10000, hi=20000, Qs=None, K=10):
    w = flat_world(*PLAIN)
    Qs = two_queries(18, 40, w["d"]) if Qs is None else Qs
    B = len(Qs[0])

    def call(H, p, st, host):
        return NL()[1].gulon_index_scan_partial_dev(H.h, p["q"], B, K, 0, hi - lo, p["pd"], p["pi"], st)
    return Case("scan_partial, second shard", ("gulon_index_scan_partial_dev",), flat_maker(w, lo=lo, hi=hi), {"q": Qs},
                partial_outs(B, K), call)


def _synchronised(torch, case, which):
    H = case.make()
    try:
        rc, out, _, _ = sc.run_synchronised(torch, case, H, case.inputs(which))
        assert rc == 0
        return out
    finally:
        H.close()


def shard_lists(torch, Qs, K=10):
    """[which][2 lists][B][K+1] partial lists of the two shards of the plain world"""
    halves = [scan_partial_case(0, 10000, Qs, K), scan_partial_case(10000, 20000, Qs, K)]
    per = [[_synchronised(torch, c, which) for c in halves] for which in (0, 1)]
    return tuple((np.stack([o["pd"] for o in lists]), np.stack([o["pi"] for o in lists])) for lists in per)


def topk_merge_case(torch):
    w = flat_world(*PLAIN)
    Qs, K = two_queries(19, 40, w["d"]), 10
    B = len(Qs[0])
    (pdr, pir), (pdd, pid) = shard_lists(torch, Qs, K)
    outs = query_outs(B, K)

    def call(H, p, st, host):
        return NL()[1].gulon_topk_merge_dev(p["pd"], p["pi"], 2, 0, B, K, p["idx"], p["dist"], p["count"], p["flags"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        assert NL()[1].gulon_topk_merge(ins["pd"].reshape(-1), ins["pi"].reshape(-1), 2, B, K, o["idx"].reshape(-1),
                                        o["dist"].reshape(-1), o["count"], o["flags"]) == 0
        return o
    return Case("topk_merge of two shards", ("gulon_topk_merge_dev",), free_maker(), {"pd": (pdr, pdd), "pi": (pir, pid)},
                outs, call, host_form)


def nan_fix_case(torch):
    w = flat_world(*PLAIN)
    Qr, Qd = two_queries(20, 8, w["d"])
    Qr[1, 7] = np.nan
    Qd[3, 2] = np.nan
    B, K = 8, 10
    rng = np.random.default_rng(21)
    merged = {"idx": rng.integers(0, w["n"], (B, K)).astype(np.int32),
              "dist": np.sort(rng.random((B, K)).astype(np.float32), axis=1),
              "count": np.full(B, K, np.int32), "flags": np.zeros(B, np.int32)}
    ins = {"q": (Qr, Qd)}
    ins.update({k: (v, v) for k, v in merged.items()})

    def call(H, p, st, host):
        return NL()[1].gulon_nan_queries_fix_dev(p["q"], B, w["d"], K, w["n"], p["idx"], p["dist"], p["count"], p["flags"],
                                                 st)
    return Case("nan_queries_fix", ("gulon_nan_queries_fix_dev",), free_maker(), ins, {}, call,
                inout=("idx", "dist", "count", "flags"))


def bounded_scan_case():
    w = flat_world(*PLAIN)
    Qs, K = two_queries(22, 40, w["d"]), 10
    B, n = 40, w["n"]
    outs = partial_outs(B, K)
    outs["bounds"] = ((B, K + 1), np.float32, F_FILL)

    def call(H, p, st, host):
        L = NL()[1]
        rc = L.gulon_index_scan_bounds_dev(H.h, p["q"], B, K, 0, n, p["bounds"], st)
        return rc or L.gulon_index_scan_partial_bounded_dev(H.h, p["q"], B, K, 0, n, p["bounds"], 1, p["pd"], p["pi"], st)

    def check(H, ref):
        _expect(np.isfinite(ref["bounds"]).any(), "has no sample bounds")
    return Case("scan_bounds then scan_partial_bounded",
                ("gulon_index_scan_bounds_dev", "gulon_index_scan_partial_bounded_dev"), flat_maker(w, FILTER_TUNING),
                {"q": Qs}, outs, call, check_ref=check)


def replay_case(torch):
    """The sharded tie replay on one list: the merged (distance, row id) answer of tie-flagged queries, then
    replay_collect and replay_apply on the stream."""
    w, Qs = tie_queries()
    B, K, n = len(Qs[0]), 10, w["n"]
    N, L = NL()
    words = int(L.gulon_replay_pack_words(N.REPLAY_MAX_FLAGGED, N.REPLAY_POOL))
    merged = []
    for which in (0, 1):
        lists = Case("lists", (), flat_maker(w), {"q": Qs}, partial_outs(B, K),
                     lambda H, p, st, host: L.gulon_index_scan_partial_dev(H.h, p["q"], B, K, 0, n, p["pd"], p["pi"], st))
        o = _synchronised(torch, lists, which)
        merge = Case("merge", (), free_maker(), {"pd": (o["pd"],) * 2, "pi": (o["pi"],) * 2}, query_outs(B, K),
                     lambda H, p, st, host: L.gulon_topk_merge_dev(p["pd"], p["pi"], 1, 0, B, K, p["idx"], p["dist"],
                                                                   p["count"], p["flags"], st))
        merged.append(_synchronised(torch, merge, 0))
    ins = {"q": Qs}
    ins.update({k: (merged[0][k], merged[1][k]) for k in ("idx", "dist", "count", "flags")})

    def call(H, p, st, host):
        rc = L.gulon_index_replay_collect_dev(H.h, p["q"], B, K, 0, n, p["flags"], 0, N.REPLAY_MAX_FLAGGED, N.REPLAY_POOL,
                                              p["pack"], st)
        return rc or L.gulon_replay_apply_dev(p["pack"], 1, N.REPLAY_MAX_FLAGGED, N.REPLAY_POOL, B, K, p["idx"], p["dist"],
                                              p["count"], p["flags"], st)

    def check(H, ref):
        _expect(((merged[0]["flags"] & 3) != 0).all() and (merged[0]["flags"] & 4 == 0).all(), "has no unreplayed ties")
        _expect(((ref["flags"] & 4) != 0).all(), "did not replay every query")
    return Case("replay_collect then replay_apply", ("gulon_index_replay_collect_dev", "gulon_replay_apply_dev"),
                flat_maker(w), ins, {}, call, inout=("idx", "dist", "count", "flags"),
                scratch={"pack": ((words,), np.int32)}, check_ref=check)


# ---------------------------------------------------------------- cases: rows, expressions, cosmul, offsets on a flat index
def lookup_world():
    return flat_world(*LOOKUP)


def row_ids(seed, b, n):
    rng = np.random.default_rng(seed)
    return tuple(np.concatenate([rng.integers(0, n, b - 2), [0, n - 1]]).astype(np.int32) for _ in range(2))


def decode_rows_case():
    w = lookup_world()
    b, d = 33, w["d"]
    outs = {"out": ((b, d), np.float32, F_FILL)}

    def call(H, p, st, host):
        return NL()[1].gulon_index_decode_rows_dev(H.h, p["rows"], b, 1, p["out"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        assert NL()[1].gulon_index_decode_rows(H.h, ins["rows"], b, 1, o["out"].reshape(-1)) == 0
        return o
    return Case("decode_rows", ("gulon_index_decode_rows_dev",), flat_maker(w), {"rows": row_ids(30, b, w["n"])}, outs,
                call, host_form, status=flat_row_error, spoil=spoil_entry("rows", 5, w["n"]))


def query_rows_case():
    w = lookup_world()
    b, K, n = 33, 10, w["n"]
    outs = query_outs(b, K)

    def call(H, p, st, host):
        return NL()[1].gulon_index_query_rows_dev(H.h, p["rows"], b, K, 0, 0, n, p["idx"], p["dist"], p["count"],
                                                  p["flags"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        assert NL()[1].gulon_index_query_rows(H.h, ins["rows"], b, K, 0, 0, n, o["idx"].reshape(-1), o["dist"].reshape(-1),
                                              o["count"], o["flags"]) == 0
        return o
    return Case("index query_rows", ("gulon_index_query_rows_dev",), flat_maker(w), {"rows": row_ids(31, b, n)}, outs,
                call, host_form, status=flat_row_error, spoil=spoil_entry("rows", 5, -1))


def compose_case(kind):
    """kind: flat / grouped / dataset"""
    b = 9
    if kind == "flat":
        w = lookup_world()
        n, d, make = w["n"], w["d"], flat_maker(w)
        dev, hst = "gulon_index_compose_rows_dev", "gulon_index_compose_rows"
    elif kind == "grouped":
        w = grouped_world(16)
        n, d, make = w["n"], w["d"], grouped_maker()
        dev, hst = "gulon_grouped_index_compose_rows_dev", "gulon_grouped_index_compose_rows"
    else:
        n, d, make = EXACT_N, EXACT_D, dataset_maker(exact_world())
        dev, hst = "gulon_dataset_compose_rows_dev", "gulon_dataset_compose_rows"
    off, sets = csr_terms(32, b, n)
    outs = {"out": ((b, d), np.float32, F_FILL)}
    if kind == "dataset":
        outs["err"] = ((1,), np.int32, 0)          # the caller zeroes it

    def call(H, p, st, host):
        args = (H.h, p["off"], p["rows"], p["w"], b, 1, 1, p["out"])
        return getattr(NL()[1], dev)(*args, *((p["err"],) if kind == "dataset" else ()), st)

    def host_form(H, ins):
        o = {"out": np.full((b, d), F_FILL, np.float32)}
        assert getattr(NL()[1], hst)(H.h, ins["off"], ins["rows"], ins["w"], b, 1, 1, o["out"].reshape(-1)) == 0
        return o
    status = {"flat": flat_row_error, "grouped": grouped_row_error, "dataset": None}[kind]
    return Case(f"{kind} compose_rows", (dev,), make, term_ins(off, sets), outs, call, host_form, status=status,
                spoil=spoil_entry("rows", 4, n + 5))


def query_terms_case(kind, K=10):
    """kind: flat / grouped / exact"""
    b, extra = 9, 3
    if kind == "flat":
        w = lookup_world()
        n, make = w["n"], flat_maker(w)
    elif kind == "grouped":
        w = grouped_world(16)
        n, make = w["n"], grouped_maker()
    else:
        n, make = EXACT_N, exact_maker()
    off, sets = csr_terms(33, b, n)
    outs = query_outs(b, K, flags=kind != "grouped")
    L = NL()[1]

    def call(H, p, st, host):
        head = (H.h, p["off"], p["rows"], p["w"], b, K, extra, 0, 0)
        if kind == "flat":
            return L.gulon_index_query_terms_dev(*head, 0, n, p["idx"], p["dist"], p["count"], p["flags"], st)
        if kind == "grouped":
            return L.gulon_grouped_index_query_terms_dev(*head, 0, 3, p["idx"], p["dist"], p["count"], st)
        return L.gulon_exact_index_query_terms_dev(*head, p["idx"], p["dist"], p["count"], p["flags"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        head = (H.h, ins["off"], ins["rows"], ins["w"], b, K, extra, 0, 0)
        res = (o["idx"].reshape(-1), o["dist"].reshape(-1), o["count"])
        if kind == "flat":
            rc = L.gulon_index_query_terms(*head, 0, n, *res, o["flags"])
        elif kind == "grouped":
            rc = L.gulon_grouped_index_query_terms(*head, 0, 3, *res)
        else:
            rc = L.gulon_exact_index_query_terms(*head, *res, o["flags"])
        assert rc == 0
        return o
    entry = {"flat": "gulon_index_query_terms_dev", "grouped": "gulon_grouped_index_query_terms_dev",
             "exact": "gulon_exact_index_query_terms_dev"}[kind]
    status = {"flat": flat_row_error, "grouped": grouped_row_error, "exact": None}[kind]
    return Case(f"{kind} query_terms K = {K}", (entry,), make, term_ins(off, sets), outs, call, host_form,
                syncs=kind == "exact", status=status, spoil=spoil_entry("rows", 4, n + 5) if status else None)


def cosmul_case(kind, K=10):
    b = 9
    exact = kind == "exact"
    if exact:
        n, make = EXACT_N, exact_maker()
    else:
        w = lookup_world()
        n, make = w["n"], flat_maker(w)
    off, sets = csr_terms(34, b, n, cosmul=True)
    outs = query_outs(b, K, flags=False, dist="score")
    if exact:
        outs["err"] = ((1,), np.int32, 0)
    L = NL()[1]

    def call(H, p, st, host):
        if exact:
            return L.gulon_exact_index_query_cosmul_dev(H.h, p["off"], p["rows"], p["w"], b, K, 1, p["idx"], p["score"],
                                                        p["count"], p["err"], st)
        return L.gulon_index_query_cosmul_dev(H.h, p["off"], p["rows"], p["w"], b, K, 1, 0, n, p["idx"], p["score"],
                                              p["count"], st)

    def host_form(H, ins):
        o = host_buffers({k: v for k, v in outs.items() if k != "err"})
        res = (o["idx"].reshape(-1), o["score"].reshape(-1), o["count"])
        if exact:
            rc = L.gulon_exact_index_query_cosmul(H.h, ins["off"], ins["rows"], ins["w"], b, K, 1, *res)
        else:
            rc = L.gulon_index_query_cosmul(H.h, ins["off"], ins["rows"], ins["w"], b, K, 1, 0, n, *res)
        assert rc == 0
        return o
    def three_chunks(H, ref):                    # the launcher's own arithmetic, as test_gpu_cosmul_paths.py reads it
        shape = np.zeros(3, np.int32)
        hooks = NL()[0].hooks_lib()
        assert hooks.gulon_selftest_cosmul_flat_shape(H.h, b, 0, n, shape) == 0
        _expect(shape[0] >= b and shape[1] == 3, f"left: one pass over three row chunks (shape {shape.tolist()})")
    entry = "gulon_exact_index_query_cosmul_dev" if exact else "gulon_index_query_cosmul_dev"
    return Case(f"{kind} query_cosmul", (entry,), make, term_ins(off, sets), outs, call, host_form,
                check_ref=None if exact else three_chunks,
                status=None if exact else flat_row_error, spoil=spoil_entry("rows", 4, n + 5))


def offset_case(kind, K=10):
    b = 8
    exact = kind == "exact"
    if exact:
        n, d, make = EXACT_N, EXACT_D, exact_maker()
    else:
        w = lookup_world()
        n, d, make = w["n"], w["d"], flat_maker(w)
    rng = np.random.default_rng(35)
    ins = {"q": two_queries(36, b, d), "roff": tuple(rng.random(n).astype(np.float32) * 4 for _ in range(2)),
           "excl": tuple(rng.integers(-1, n, b).astype(np.int32) for _ in range(2))}
    outs = query_outs(b, K, flags=False, dist="key")
    L = NL()[1]

    def call(H, p, st, host):
        if exact:
            return L.gulon_exact_index_query_offset_dev(H.h, p["q"], b, K, p["roff"], p["excl"], p["idx"], p["key"],
                                                        p["count"], st)
        return L.gulon_index_query_offset_dev(H.h, p["q"], b, K, 0, n, p["roff"], p["excl"], p["idx"], p["key"],
                                              p["count"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        res = (o["idx"].reshape(-1), o["key"].reshape(-1), o["count"])
        if exact:
            rc = L.gulon_exact_index_query_offset(H.h, ins["q"].reshape(-1), b, K, ins["roff"], vp(ins["excl"]), *res)
        else:
            rc = L.gulon_index_query_offset(H.h, ins["q"].reshape(-1), b, K, 0, n, ins["roff"], vp(ins["excl"]), *res)
        assert rc == 0
        return o
    def three_chunks(H, ref):                    # offset.hip's launch arithmetic, restated in offset_ref.py
        from offset_ref import flat_chunks
        shape = flat_chunks(0, n, b, w["m"])
        _expect(shape[0] >= b and shape[1] == 3, f"left: one pass over three row chunks (shape {shape})")
    entry = "gulon_exact_index_query_offset_dev" if exact else "gulon_index_query_offset_dev"
    return Case(f"{kind} query_offset", (entry,), make, ins, outs, call, host_form,
                check_ref=None if exact else three_chunks)


def mean_similarity_case():
    b, kin, K = 33, 10, 10
    rng = np.random.default_rng(37)
    ins = {"lists": tuple((rng.random((b, kin)) * 2).astype(np.float32) for _ in range(2)),
           "counts": tuple(rng.integers(0, kin + 1, b).astype(np.int32) for _ in range(2))}
    outs = {"out": ((b,), np.float32, F_FILL)}

    def call(H, p, st, host):
        return NL()[1].gulon_mean_similarity_dev(p["lists"], p["counts"], b, kin, K, p["out"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        assert NL()[1].gulon_mean_similarity(ins["lists"].reshape(-1), vp(ins["counts"]), b, kin, K, o["out"]) == 0
        return o
    return Case("mean_similarity", ("gulon_mean_similarity_dev",), free_maker(), ins, outs, call, host_form)


# ---------------------------------------------------------------- cases: pair distances, row errors, refine forms
def pair_distances_case(kind):
    """kind: flat / grouped / dataset.  130 pairs.  The _dev forms synchronise the stream once and report a bad id."""
    npairs = 130
    if kind == "flat":
        w = lookup_world()
        n, make = w["n"], flat_maker(w)
    elif kind == "grouped":
        w = grouped_world(16)
        n, make = w["n"], grouped_maker()
    else:
        n, make = EXACT_N, dataset_maker(exact_world())
    rng = np.random.default_rng(38)
    ins = {"a": tuple(rng.integers(0, n, npairs).astype(np.int32) for _ in range(2)),
           "b": tuple(rng.integers(0, n, npairs).astype(np.int32) for _ in range(2))}
    outs = {"out": ((npairs,), np.float32, F_FILL)}
    stem = {"flat": "gulon_index_pair_distances", "grouped": "gulon_grouped_index_pair_distances",
            "dataset": "gulon_dataset_pair_distances"}[kind]

    def call(H, p, st, host):
        return getattr(NL()[1], stem + "_dev")(H.h, p["a"], p["b"], npairs, p["out"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        assert getattr(NL()[1], stem)(H.h, ins["a"], ins["b"], npairs, o["out"]) == 0
        return o
    return Case(f"{kind} pair_distances", (stem + "_dev",), make, ins, outs, call, host_form, syncs=True,
                spoil=spoil_entry("b", 77, n))


def row_errors_case(kind):
    if kind == "flat":
        w = lookup_world()
        vectors = np.random.default_rng(39).standard_normal((w["n"], w["d"])).astype(np.float32)
        make, stem = flat_maker(w, dataset=vectors), "gulon_index_row_errors"
    else:
        w = grouped_world(16)
        make, stem = grouped_maker(), "gulon_grouped_index_row_errors"
    n, m = w["n"], w["m"]
    frm, until = 5, n - 3
    rng = np.random.default_rng(40)
    ins = {"map": tuple(rng.permutation(n).astype(np.int32) for _ in range(2))}
    outs = {"err": ((until - frm,), np.float32, F_FILL), "norm": ((until - frm,), np.float32, F_FILL)}

    def call(H, p, st, host):
        host["qerr"] = np.zeros(m, np.float64)
        return getattr(NL()[1], stem + "_dev")(H.h, H.ds, p["map"], n, frm, until, p["err"], p["norm"], host["qerr"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        o["host:qerr"] = np.zeros(m, np.float64)
        assert getattr(NL()[1], stem)(H.h, H.ds, vp(ins["map"]), n, frm, until, vp(o["err"]), vp(o["norm"]),
                                      o["host:qerr"]) == 0
        return o
    return Case(f"{kind} row_errors", (stem + "_dev",), make, ins, outs, call, host_form, syncs=True)


def refine_case(kind):
    """kind: dataset (gulon_refine_topk_dev) / flat / grouped (gulon_*_refine_codes_topk_dev)"""
    b, c, K = 9, 20, 10
    L = NL()[1]
    if kind == "dataset":
        n, d, make = EXACT_N, EXACT_D, dataset_maker(exact_world())
        dev, hst = L.gulon_refine_topk_dev, L.gulon_refine_topk
    elif kind == "flat":
        w = lookup_world()
        n, d = w["n"], w["d"]
        make = flat_maker(w, fine=flat_world(n, d, 8, 16, 50))
        dev, hst = L.gulon_index_refine_codes_topk_dev, L.gulon_index_refine_codes_topk
    else:
        w = grouped_world(16)
        n, d = w["n"], w["d"]
        make = grouped_maker(fine=flat_world(n, d, 2, 16, 51))
        dev, hst = L.gulon_grouped_index_refine_codes_topk_dev, L.gulon_grouped_index_refine_codes_topk
    rng = np.random.default_rng(41)
    ins = {"q": two_queries(42, b, d),
           "cand": tuple(np.stack([rng.choice(n, c, replace=False) for _ in range(b)]).astype(np.int32) for _ in range(2)),
           "map": tuple(rng.permutation(n).astype(np.int32) for _ in range(2))}
    outs = query_outs(b, K, flags=False)

    def first(H):
        return (H.h,) if kind == "dataset" else (H.h, H.fine)

    def call(H, p, st, host):
        return dev(*first(H), p["q"], b, p["cand"], c, p["map"], n, K, p["idx"], p["dist"], p["count"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        assert hst(*first(H), ins["q"].reshape(-1), b, ins["cand"].reshape(-1), c, vp(ins["map"]), n, K,
                   o["idx"].reshape(-1), o["dist"].reshape(-1), o["count"]) == 0
        return o
    return Case(f"{kind} refine", (dev.__name__,), make, ins, outs, call, host_form,
                spoil=spoil_entry("cand", 4 * c + 7, n + 3), defined=mask_refused)


# ---------------------------------------------------------------- cases: the grouped index
def grouped_query_case(name, strategy, limit, K, k=16, groups=20):
    w = grouped_world(k, groups)
    # coarse_stage searches at most nn_stride = min(limit + the empty groups (LimitVectors only), groups) groups per query;
    # LimitVectors with nn_stride > 64 reads the largest count of the batch back on the stream and waits for it
    nn_stride = max(1, min(limit + (w["empty"] if strategy == 1 else 0), w["groups"]))
    reads_back = strategy == 1 and nn_stride > 64
    B = GROUPED["B"]
    Qs = two_queries(43 + K, B, w["d"], scale=3.0)
    outs = query_outs(B, K, flags=False)

    def call(H, p, st, host):
        return NL()[1].gulon_grouped_index_batch_query_dev(H.h, p["q"], B, K, strategy, limit, p["idx"], p["dist"],
                                                           p["count"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        assert NL()[1].gulon_grouped_index_batch_query(H.h, ins["q"].reshape(-1), B, K, strategy, limit,
                                                       o["idx"].reshape(-1), o["dist"].reshape(-1), o["count"]) == 0
        return o
    return Case("grouped batch_query " + name, ("gulon_grouped_index_batch_query_dev",), grouped_maker(k, groups=groups),
                {"q": Qs}, outs, call, host_form, syncs=reads_back, waits=reads_back)


def grouped_rows_case(query):
    w = grouped_world(16)
    b, K, n, d = GROUPED["B"], 10, w["n"], w["d"]
    L = NL()[1]
    if query:
        outs = query_outs(b, K, flags=False)

        def call(H, p, st, host):
            return L.gulon_grouped_index_query_rows_dev(H.h, p["rows"], b, K, 0, 0, 3, p["idx"], p["dist"], p["count"], st)

        def host_form(H, ins):
            o = host_buffers(outs)
            assert L.gulon_grouped_index_query_rows(H.h, ins["rows"], b, K, 0, 0, 3, o["idx"].reshape(-1),
                                                    o["dist"].reshape(-1), o["count"]) == 0
            return o
        entry = "gulon_grouped_index_query_rows_dev"
    else:
        outs = {"out": ((b, d), np.float32, F_FILL)}

        def call(H, p, st, host):
            return L.gulon_grouped_index_lookup_rows_dev(H.h, p["rows"], b, 0, p["out"], st)

        def host_form(H, ins):
            o = host_buffers(outs)
            assert L.gulon_grouped_index_lookup_rows(H.h, ins["rows"], b, 0, o["out"].reshape(-1)) == 0
            return o
        entry = "gulon_grouped_index_lookup_rows_dev"
    return Case(entry[len("gulon_"):-len("_dev")], (entry,), grouped_maker(), {"rows": row_ids(44, b, n)}, outs, call,
                host_form, status=grouped_row_error, spoil=spoil_entry("rows", 5, n))


# ---------------------------------------------------------------- cases: the exact index
def exact_query_case(K, rows=False):
    B = 17
    outs = query_outs(B, K)
    L = NL()[1]
    if rows:
        ins = {"rows": row_ids(45, B, EXACT_N)}

        def call(H, p, st, host):
            return L.gulon_exact_index_query_rows_dev(H.h, p["rows"], B, K, p["idx"], p["dist"], p["count"], p["flags"], st)

        def host_form(H, ins):
            o = host_buffers(outs)
            assert L.gulon_exact_index_query_rows(H.h, ins["rows"], B, K, o["idx"].reshape(-1), o["dist"].reshape(-1),
                                                  o["count"], o["flags"]) == 0
            return o
        entry = "gulon_exact_index_query_rows_dev"
    else:
        ins = {"q": two_queries(46 + K, B, EXACT_D)}

        def call(H, p, st, host):
            return L.gulon_exact_index_batch_query_dev(H.h, p["q"], B, K, p["idx"], p["dist"], p["count"], p["flags"], st)

        def host_form(H, ins):
            o = host_buffers(outs)
            assert L.gulon_exact_index_batch_query(H.h, ins["q"].reshape(-1), B, K, o["idx"].reshape(-1),
                                                   o["dist"].reshape(-1), o["count"], o["flags"]) == 0
            return o
        entry = "gulon_exact_index_batch_query_dev"
    # the header: "the call itself waits for the stream once per batch"
    return Case(f"{entry[len('gulon_'):-len('_dev')]} K = {K}", (entry,), exact_maker(), ins, outs, call, host_form,
                syncs=True)


# ---------------------------------------------------------------- cases: free functions
def rotate_case():
    n = d = 65
    rng = np.random.default_rng(47)
    ins = {"x": tuple(rng.standard_normal((n, d)).astype(np.float32) for _ in range(2)),
           "r": tuple(rng.standard_normal((d, d)).astype(np.float32) for _ in range(2))}
    outs = {"out": ((n, d), np.float32, F_FILL)}

    def call(H, p, st, host):
        return NL()[1].gulon_rotate_rows_dev(p["x"], n, d, p["r"], 1, p["out"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        assert NL()[1].gulon_rotate_rows(ins["x"].reshape(-1), n, d, ins["r"].reshape(-1), 1, o["out"].reshape(-1)) == 0
        return o
    return Case("rotate_rows", ("gulon_rotate_rows_dev",), free_maker(), ins, outs, call, host_form)


def rank_sums_case():
    n, sections = 257, 3
    rng = np.random.default_rng(48)
    ins = {"x": tuple(rng.integers(0, 40, n).astype(np.float32) for _ in range(2)),
           "y": tuple(rng.standard_normal(n).astype(np.float32) for _ in range(2)),
           "sec": tuple(rng.integers(0, sections, n).astype(np.int32) for _ in range(2))}
    outs = {"out": ((sections, 5), np.int64, I_FILL)}

    def call(H, p, st, host):
        return NL()[1].gulon_rank_sums_dev(p["x"], p["y"], p["sec"], n, sections, p["out"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        assert NL()[1].gulon_rank_sums(ins["x"], ins["y"], vp(ins["sec"]), n, sections, o["out"].reshape(-1)) == 0
        return o
    return Case("rank_sums", ("gulon_rank_sums_dev",), free_maker(), ins, outs, call, host_form)


def mutual_rows_case():
    ns, nt = 257, 300
    rng = np.random.default_rng(49)
    ins = {"fwd": tuple(rng.integers(-1, nt, ns).astype(np.int32) for _ in range(2)),
           "bwd": tuple(rng.integers(0, ns, nt).astype(np.int32) for _ in range(2))}
    for fwd, bwd in zip(*ins.values()):            # half of the rows choose each other
        live = np.flatnonzero(fwd[::2] >= 0) * 2
        bwd[fwd[live]] = live
    outs = {"out": ((ns,), np.int32, I_FILL)}

    def call(H, p, st, host):
        return NL()[1].gulon_mutual_rows_dev(p["fwd"], ns, p["bwd"], nt, p["out"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        assert NL()[1].gulon_mutual_rows(vp(ins["fwd"]), ns, vp(ins["bwd"]), nt, vp(o["out"])) == 0
        return o
    return Case("mutual_rows", ("gulon_mutual_rows_dev",), free_maker(), ins, outs, call, host_form)


def analogy_counts_case():
    b, kin, nks, sections = 33, 10, 3, 3
    rng = np.random.default_rng(50)
    ks = np.array([1, 5, 10], np.int32)
    lists = tuple(np.stack([rng.choice(1000, kin, replace=False) for _ in range(b)]).astype(np.int32) for _ in range(2))
    ins = {"lists": lists, "counts": tuple(rng.integers(0, kin + 1, b).astype(np.int32) for _ in range(2)),
           "expected": tuple(np.where(rng.random(b) < 0.7, l[np.arange(b), rng.integers(0, kin, b)],
                                      rng.integers(0, 1000, b)).astype(np.int32) for l in lists),
           "section": tuple(rng.integers(0, sections, b).astype(np.int32) for _ in range(2)), "ks": (ks, ks)}
    outs = {"hits": ((sections, nks), np.int32, 0), "asked": ((sections,), np.int32, 0),     # they accumulate: zeroed
            "rank": ((b,), np.int32, I_FILL)}

    def call(H, p, st, host):
        return NL()[1].gulon_analogy_counts_dev(p["lists"], p["counts"], b, kin, p["expected"], p["section"], p["ks"], nks,
                                                sections, p["hits"], p["asked"], p["rank"], st)

    def host_form(H, ins):
        o = host_buffers(outs)
        assert NL()[1].gulon_analogy_counts(ins["lists"].reshape(-1), ins["counts"], b, kin, ins["expected"],
                                            ins["section"], ins["ks"], nks, sections, o["hits"].reshape(-1), o["asked"],
                                            vp(o["rank"])) == 0
        return o
    return Case("analogy_counts", ("gulon_analogy_counts_dev",), free_maker(), ins, outs, call, host_form)


# ---------------------------------------------------------------- cases: views
VIEW = (200, 16, 4, 16, 6)
VIEW_ROWS = np.arange(1, 200, 3, dtype=np.int32)[:67]


def view_query_case():
    w = flat_world(*VIEW)
    return batch_query_case("view batch_query", flat_maker(w, view=VIEW_ROWS), two_queries(52, 8, w["d"]), 5, len(VIEW_ROWS),
                            entry="gulon_index_view_batch_query_dev", host_entry="gulon_index_view_batch_query")


def view_map_case():
    w = flat_world(*VIEW)
    rng = np.random.default_rng(53)
    count = 8 * 5
    ins = {"idx": tuple(np.concatenate([rng.integers(0, 67, count - 3), [-1, INT32_MAX, 66]]).astype(np.int32)
                        for _ in range(2))}

    def call(H, p, st, host):
        return NL()[1].gulon_index_view_map_rows_dev(H.h, p["idx"], count, st)
    return Case("view map_rows", ("gulon_index_view_map_rows_dev",), flat_maker(w, view=VIEW_ROWS), ins, {}, call,
                inout=("idx",))


# ---------------------------------------------------------------- the table
NEEDS_TORCH = {topk_merge_case, nan_fix_case, replay_case}      # their inputs are the outputs of earlier calls

P = functools.partial
TABLE = {
    "gulon_index_batch_query_dev": [plain_scan, filtered_scan, tie_replay, nonfinite_pass, peeled_k100,
                                    P(wide_codes, 10), P(wide_codes, 100), wide_filter, context_handle],
    "gulon_index_scan_partial_dev": [scan_partial_case],
    "gulon_index_scan_bounds_dev": [bounded_scan_case],
    "gulon_index_scan_partial_bounded_dev": [bounded_scan_case],
    "gulon_index_replay_collect_dev": [replay_case],
    "gulon_replay_apply_dev": [replay_case],
    "gulon_topk_merge_dev": [topk_merge_case],
    "gulon_nan_queries_fix_dev": [nan_fix_case],
    "gulon_index_decode_rows_dev": [decode_rows_case],
    "gulon_index_query_rows_dev": [query_rows_case],
    "gulon_index_compose_rows_dev": [P(compose_case, "flat")],
    "gulon_grouped_index_compose_rows_dev": [P(compose_case, "grouped")],
    "gulon_dataset_compose_rows_dev": [P(compose_case, "dataset")],
    "gulon_index_query_terms_dev": [P(query_terms_case, "flat")],
    "gulon_grouped_index_query_terms_dev": [P(query_terms_case, "grouped")],
    "gulon_exact_index_query_terms_dev": [P(query_terms_case, "exact"), P(query_terms_case, "exact", 64)],
    "gulon_index_query_cosmul_dev": [P(cosmul_case, "flat")],
    "gulon_exact_index_query_cosmul_dev": [P(cosmul_case, "exact")],
    "gulon_index_query_offset_dev": [P(offset_case, "flat")],
    "gulon_exact_index_query_offset_dev": [P(offset_case, "exact")],
    "gulon_mean_similarity_dev": [mean_similarity_case],
    "gulon_grouped_index_batch_query_dev": [P(grouped_query_case, "LimitGroups3", 0, 3, 10),
                                            P(grouped_query_case, "LimitVectors700", 1, 700, 10),
                                            # 72 groups, two of them empty: nn_stride = min(700 + 2, 72) = 72 > 64, so the
                                            # call reads a counter back on the stream and waits for it: results only
                                            P(grouped_query_case, "LimitVectors700_72_groups", 1, 700, 10, groups=72),
                                            P(grouped_query_case, "K200_heaps_in_LDS", 0, 3, 200),
                                            P(grouped_query_case, "wide_codes_k300", 0, 3, 10, k=300)],
    "gulon_grouped_index_query_rows_dev": [P(grouped_rows_case, True)],
    "gulon_grouped_index_lookup_rows_dev": [P(grouped_rows_case, False)],
    "gulon_grouped_index_pair_distances_dev": [P(pair_distances_case, "grouped")],
    "gulon_grouped_index_row_errors_dev": [P(row_errors_case, "grouped")],
    "gulon_index_pair_distances_dev": [P(pair_distances_case, "flat")],
    "gulon_dataset_pair_distances_dev": [P(pair_distances_case, "dataset")],
    "gulon_index_row_errors_dev": [P(row_errors_case, "flat")],
    "gulon_refine_topk_dev": [P(refine_case, "dataset")],
    "gulon_index_refine_codes_topk_dev": [P(refine_case, "flat")],
    "gulon_grouped_index_refine_codes_topk_dev": [P(refine_case, "grouped")],
    "gulon_exact_index_batch_query_dev": [P(exact_query_case, 10), P(exact_query_case, 64)],
    "gulon_exact_index_query_rows_dev": [P(exact_query_case, 10, rows=True), P(exact_query_case, 64, rows=True)],
    "gulon_rotate_rows_dev": [rotate_case],
    "gulon_rank_sums_dev": [rank_sums_case],
    "gulon_mutual_rows_dev": [mutual_rows_case],
    "gulon_analogy_counts_dev": [analogy_counts_case],
    "gulon_index_view_batch_query_dev": [view_query_case],
    "gulon_index_view_map_rows_dev": [view_map_case],
}


def _label(factory):
    f = factory
    args = ""
    if isinstance(f, functools.partial):
        args = "-" + "-".join(str(a) for a in f.args + tuple(f.keywords.values()))
        f = f.func
    return (f.__name__.replace("_case", "") + args).replace(" ", "_")


def _factories():
    seen, out = set(), []
    for fs in TABLE.values():
        for f in fs:
            if _label(f) not in seen:
                seen.add(_label(f))
                out.append(f)
    return out


# the cases that have a status word: covered twice, once clean and once with exactly one offending id
HAS_BAD = {"decode_rows", "query_rows", "compose-flat", "compose-grouped", "compose-dataset", "query_terms-flat",
           "query_terms-grouped", "cosmul-flat", "cosmul-exact", "pair_distances-flat", "pair_distances-grouped",
           "pair_distances-dataset", "refine-dataset", "refine-flat", "refine-grouped", "grouped_rows-True",
           "grouped_rows-False"}
KIND_A = [(f, bad) for f in _factories() for bad in ((False, True) if _label(f) in HAS_BAD else (False,))]


def build(factory, torch):
    f = factory.func if isinstance(factory, functools.partial) else factory
    return factory(torch) if f in NEEDS_TORCH else factory()


# ---------------------------------------------------------------- completeness
def test_every_stream_parameter_has_a_case():
    text = sc.header_text()
    declared = sc.stream_entry_points(text)
    assert len(declared) == 40, sorted(declared)
    assert declared == set(TABLE), (sorted(declared - set(TABLE)), sorted(set(TABLE) - declared))
    assert all(TABLE[name] for name in TABLE)
    assert set(HAS_BAD) <= {_label(f) for f in _factories()}
    # device pointers without a stream parameter: on the null stream by contract, and the header says so
    assert sc.device_pointer_entry_points_without_stream(text) == NULL_STREAM_BY_CONTRACT
    for name in NULL_STREAM_BY_CONTRACT:
        assert any("null stream" in " ".join(c.split()) for c in sc.comments_naming(text, name)), name


def test_cases_name_the_entry_points_they_call(torch):
    for name, factories in TABLE.items():
        for f in factories:
            assert name in build(f, torch).entries, (name, _label(f))


# ---------------------------------------------------------------- kind A
def reported(case, rc, word, outs):
    """Did the call report an offending id, by whichever status word it has?"""
    return bool(rc != 0 or (word or 0) != 0 or ("count" in outs and (outs["count"] == -1).any())
                or ("err" in outs and outs["err"].dtype == np.int32 and outs["err"].any()))


@pytest.mark.parametrize("factory,bad", KIND_A, ids=[_label(f) + ("-bad_id" if b else "") for f, b in KIND_A])
def test_behind_pending_work(torch, delay, factory, bad):
    case = build(factory, torch)
    real, decoy = case.inputs(0, bad), case.inputs(1)
    ref_handle = case.make()
    try:
        rc0, ref, word0, _ = sc.run_synchronised(torch, case, ref_handle, real)              # stream = NULL, fresh handle
        if case.check_ref and not bad:
            case.check_ref(ref_handle, ref)
        idle = torch.cuda.Stream()
        rcd, ref_decoy, wordd, returned = sc.run_synchronised(torch, case, ref_handle, decoy, idle)   # warm: timed
        host = case.host(ref_handle, real) if case.host and not bad else None
    finally:
        ref_handle.close()
    assert not reported(case, rcd, wordd, ref_decoy), "the decoy is a valid input"
    assert reported(case, rc0, word0, ref) == bad, (rc0, word0)
    assert sc.differs(ref, ref_decoy), "the decoy's answer equals the real one: the case proves nothing"
    if host is not None:
        sc.assert_same(ref, host, "stream = NULL against the host-pointer form")
    ms = sc.delay_ms_for(returned)
    H = case.make()
    try:
        r = sc.run_behind_delay(torch, delay, case, H, real, decoy, ms)
    finally:
        H.close()
    print(f"\n[{case.name}{' (bad id)' if bad else ''}] warm call returned in {returned * 1e3:.3f} ms, delay {ms:.0f} ms, "
          f"call behind it returned in {r.return_ms:.3f} ms, delay pending at return: {r.pending_at_return}")
    assert r.rc == rc0
    if sc.differs(r.outputs, ref) and not sc.differs(r.outputs, ref_decoy):
        raise AssertionError(f"{case.name}: the call returned the DECOY's answer -- some of its work did not wait for "
                             f"the stream it was given")
    sc.assert_same(r.outputs, ref, f"{case.name} behind {ms:.0f} ms of pending work against stream = NULL")
    assert r.word == word0
    if case.waits:
        assert not r.pending_at_return, f"{case.name}: named after a read-back on the stream, but it did not wait for it"
    if not case.syncs:
        assert r.pending_at_return, (f"{case.name}: documented not to synchronise, but the {ms:.0f} ms delay was over when "
                                     f"it returned after {r.return_ms:.1f} ms")


# ---------------------------------------------------------------- kind B
@pytest.fixture(scope="module")
def stream_pair(torch, delay):
    pair = sc.independent_streams(torch, delay)
    assert pair is not None, ("no two of eight streams ran independently (GPU_MAX_HW_QUEUES?): streams that share a "
                              "hardware queue cannot show whether a handle orders its calls")
    return pair


def _scan_partial_whole():
    w = lookup_world()
    Qs, K, n = two_queries(60, 8, w["d"]), 10, w["n"]
    return Case("scan_partial", ("gulon_index_scan_partial_dev",), flat_maker(w), {"q": Qs}, partial_outs(8, K),
                lambda H, p, st, host: NL()[1].gulon_index_scan_partial_dev(H.h, p["q"], 8, K, 0, n, p["pd"], p["pi"], st))


def _lookup_batch():
    w = lookup_world()
    return batch_query_case("batch_query", flat_maker(w), two_queries(61, 8, w["d"]), 10, w["n"])


KIND_B = {
    "flat-batch_query-batch_query": (plain_scan, plain_scan),
    "flat-query_cosmul-batch_query": (P(cosmul_case, "flat"), _lookup_batch),
    "flat-query_offset-query_terms": (P(offset_case, "flat"), P(query_terms_case, "flat")),
    "flat-scan_partial-batch_query": (_scan_partial_whole, _lookup_batch),
    "context-batch_query-batch_query": (context_handle, context_handle),
    "view-batch_query-batch_query": (view_query_case, view_query_case),
    "grouped-batch_query-batch_query": (P(grouped_query_case, "LimitGroups3", 0, 3, 10),) * 2,
    "grouped-compose_rows-batch_query": (P(compose_case, "grouped"), P(grouped_query_case, "LimitGroups3", 0, 3, 10)),
    "grouped-query_rows-batch_query": (P(grouped_rows_case, True), P(grouped_query_case, "LimitGroups3", 0, 3, 10)),
    # X waits for its stream by contract (the exact index reads its counters back): passes trivially, kept for the table
    "exact-batch_query-query_offset": (P(exact_query_case, 10), P(offset_case, "exact")),
}


@pytest.mark.parametrize("pair", list(KIND_B), ids=list(KIND_B))
def test_two_streams_one_handle(torch, delay, stream_pair, pair):
    A, B = stream_pair
    X, Y = (build(f, torch) for f in KIND_B[pair])
    x_warm, x_in, y_warm, y_in = X.inputs(1), X.inputs(0), Y.inputs(0), Y.inputs(1)
    ref_handle = X.make()                          # the same four calls, one after the other
    try:
        sc.run_synchronised(torch, X, ref_handle, x_warm)
        sc.run_synchronised(torch, Y, ref_handle, y_warm)
        rcx, ref_x, _, _ = sc.run_synchronised(torch, X, ref_handle, x_in)
        rcy, ref_y, _, _ = sc.run_synchronised(torch, Y, ref_handle, y_in)
    finally:
        ref_handle.close()
    assert rcx == 0 and rcy == 0
    H = X.make()
    try:
        _, _, _, returned = sc.run_synchronised(torch, X, H, x_warm, A)       # warm: scratch grown, kernels loaded
        sc.run_synchronised(torch, Y, H, y_warm, B)
        ms = sc.delay_ms_for(returned)
        r = sc.run_two_streams(torch, delay, X, Y, H, x_in, y_in, A, B, ms)
    finally:
        H.close()
    print(f"\n[{pair}] X's warm call returned in {returned * 1e3:.3f} ms, delay {ms:.0f} ms; Y returned while the delay "
          f"was pending: {r.y_returned_pending}; Y finished after the delay: {r.ordered}")
    assert r.rc == (0, 0)
    if not X.syncs and not Y.syncs:
        assert r.y_returned_pending, f"{pair}: Y's call blocked on the host until A's delay was over"
    assert r.ordered, (f"{pair}: Y's device work on stream B finished while stream A still slept in front of X -- the "
                       f"handle did not order the two calls")
    sc.assert_same(r.outputs[0], ref_x, f"{pair}: X against its synchronised reference")
    sc.assert_same(r.outputs[1], ref_y, f"{pair}: Y against its synchronised reference")
