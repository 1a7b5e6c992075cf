"""The C oracle and the independent numpy.float32 Python restatement must agree
bit for bit on small inputs (both are written from the Scala source)."""
import numpy as np
import pytest

import filter_stage_ref as fs
import grouped_stage_ref as gs
import value_regimes as vr
from conftest import bits
from oracle import py_oracle as po


def _data(seed, n, d, scale=1.0, dup=False):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, d)) * scale).astype(np.float32)
    if dup:                      # duplicate rows => duplicate init centroids => tie-break RNG
        X[n // 2:] = X[: n - n // 2]
    return X


@pytest.mark.parametrize("seed,n,d,fr,un,k,dup", [
    (0, 200, 6, 0, 6, 5, False), (1, 300, 9, 3, 7, 8, False), (2, 120, 4, 1, 3, 16, True),
    (3, 64, 3, 0, 1, 4, True)])
def test_kmeans_pieces(oracle, seed, n, d, fr, un, k, dup):
    _kmeans_pieces(oracle, _data(seed, n, d, dup=dup), seed, fr, un, k, nan=False)


@pytest.mark.parametrize("regime", vr.BUILD_REGIMES)
@pytest.mark.parametrize("seed,n,d,fr,un,k", [(0, 200, 6, 0, 6, 5), (1, 300, 9, 3, 7, 8), (2, 120, 4, 1, 3, 16)])
def test_kmeans_pieces_value_regimes(oracle, regime, seed, n, d, fr, un, k):
    """The two CPU references agree at the value-range edges too: this pins the oracle before a GPU result is compared with it."""
    with np.errstate(all="ignore"):
        _kmeans_pieces(oracle, vr.build_case(oracle, regime, n, d, fr, un - fr, k, seed, dup=seed == 2), seed, fr, un, k, nan=True)


def _kmeans_pieces(oracle, X, seed, fr, un, k, nan):
    s = un - fr
    C0, rows = oracle.kmeans_init(X, fr, s, k, seed)
    P0 = po.kmeans_init(X.tolist(), fr, un, k, seed)
    vr.same_bits(C0, np.array(P0, np.float32), nan)
    vr.same_bits(oracle.kmeans_offsets(C0), np.array(po.kmeans_offsets(P0), np.float32), nan)
    for rb in (0, 50):
        a = oracle.kmeans_assign(X, fr, s, C0, rb)
        b = po.kmeans_assign(X.tolist(), fr, P0, rb)
        assert a.tolist() == b
    C1 = oracle.kmeans_from_assignment(X, fr, s, k, a)
    P1 = po.kmeans_from_assignment(X.tolist(), fr, s, k, b)
    vr.same_bits(C1, np.array(P1, np.float32), nan)


def test_compute_clusters(oracle):
    X = _data(5, 400, 8, dup=True)
    for (fr, un, k, it, seed) in [(0, 4, 6, 5, 0), (4, 8, 3, 20, 1)]:
        Cc, reps = oracle.kmeans_compute_clusters(X, fr, un - fr, k, it, seed)
        Pc, preps = po.kmeans_compute_clusters(X.tolist(), fr, un, k, it, seed)
        assert np.array_equal(bits(Cc), bits(np.array(Pc, np.float32)))
        assert [(r["num_iterations"], r["converged"]) for r in reps] == preps


def test_tie_break_stream_crosses_batches(oracle):
    # all-zero centroids but one: every row ties k-1 times; RNG restarts per batch
    rng = np.random.default_rng(7)
    X = rng.standard_normal((130, 2)).astype(np.float32)
    C = np.zeros((4, 2), np.float32)
    for rb in (0, 25, 64):
        a = oracle.kmeans_assign(X, 0, 2, C, rb)
        b = po.kmeans_assign(X.tolist(), 0, C.tolist(), rb)
        assert a.tolist() == b
    assert len(set(oracle.kmeans_assign(X, 0, 2, C, 0).tolist())) > 1


@pytest.mark.parametrize("n,d,m,k,B,K,fr,un", [(300, 10, 4, 7, 3, 5, 0, 300), (5000, 6, 3, 16, 2, 10, 100, 4700),
                                                (20, 4, 2, 3, 2, 30, 0, 20), (50, 5, 5, 1, 1, 4, 10, 10)])
def test_query_path(oracle, n, d, m, k, B, K, fr, un):
    rng = np.random.default_rng(n)
    cents = rng.standard_normal(k * d).astype(np.float32)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    Q = rng.standard_normal((B, d)).astype(np.float32)
    _query_path(oracle, cents, idx, Q, n, d, m, k, B, K, fr, un, nan=False)


@pytest.mark.parametrize("regime", vr.QUERY_REGIMES)
@pytest.mark.parametrize("n,d,m,k,B,K,fr,un", [(300, 10, 4, 7, 5, 5, 0, 300), (3000, 12, 6, 16, 5, 10, 100, 2700)])
def test_query_path_value_regimes(oracle, regime, n, d, m, k, B, K, fr, un):
    with np.errstate(all="ignore"):
        cents, idx, Q = vr.query_case(oracle, regime, n, d, m, k, B)
        _query_path(oracle, cents, idx, Q, n, d, m, k, B, K, fr, un, nan=True)


def _query_path(oracle, cents, idx, Q, n, d, m, k, B, K, fr, un, nan):
    T = oracle.prepare_query(cents, d, m, k, Q)
    sub = po.subvectors(d, m)
    quant = [(f, [[np.float32(v) for v in cents[k * f + c * (u - f): k * f + (c + 1) * (u - f)]]
                  for c in range(k)]) for f, u in sub]
    PT = po.prepare_query(quant, Q.tolist())
    vr.same_bits(T, np.array(PT, np.float32), nan)
    oi, od, oc = oracle.pq_batch_query(idx, d, k, cents, Q, K, fr, un)
    pres = po.pq_batch_query(quant, idx.tolist(), n, Q.tolist(), K, fr, un)
    for q in range(B):
        ks, vs = pres[q]
        assert oc[q] == len(ks) == min(K, un - fr)
        assert oi[q, :oc[q]].tolist() == ks
        vr.same_bits(od[q, :oc[q]], np.array(vs, np.float32), nan)


def test_exact_knn(oracle):
    _exact_knn(oracle, _data(11, 500, 7), _data(12, 3, 7), nan=False)


@pytest.mark.parametrize("regime", vr.BUILD_REGIMES)
def test_exact_knn_value_regimes(oracle, regime):
    with np.errstate(all="ignore"):
        X = vr.build_case(oracle, regime, 503, 7, 0, 7, 4)
        _exact_knn(oracle, X[3:], X[:3] if regime == "degenerate" else vr.build_case(oracle, regime, 3, 7, 0, 7, 4, seed=1), nan=True)


def _exact_knn(oracle, X, Q, nan):
    oi, od, oc = oracle.exact_knn(X, Q, 10, 20, 480)
    for q in range(3):
        ks, vs = po.exact_knn(X.tolist(), Q[q].tolist(), 10, 20, 480)
        assert oi[q].tolist() == ks
        vr.same_bits(od[q], np.array(vs, np.float32), nan)


@pytest.mark.parametrize("regime", vr.QUERY_REGIMES)
@pytest.mark.parametrize("form", list(vr.FORMS))
def test_query_regimes_exhibit_their_edge(oracle, regime, form):
    """A regime that does not show its edge at some shape of the GPU tests is a broken test: this is where that shows."""
    n, d, m, k = vr.FORMS[form]
    with np.errstate(all="ignore"):
        cents, idx, Q = vr.query_case(oracle, regime, n, d, m, k, vr.QUERY_B)
        vr.query_predicate(oracle, regime, cents, idx, Q, d, m, k, K=10)


@pytest.mark.parametrize("name,shape,B", [(f, s, vr.PRODUCTION_B) for f, s in vr.PRODUCTION_FORMS.items()]
                         + [("tie_" + f, s[:4], s[5]) for f, s in vr.TIE_FORMS.items()])
def test_tight_regime_is_tight_at_the_large_shapes(oracle, name, shape, B):
    n, d, m, k = shape
    cents, idx, Q = vr.query_case(oracle, "tight", n, d, m, k, B, per=50 if name.startswith("tie_") else vr.PRODUCTION_PER)
    vr.query_predicate(oracle, "tight", cents, idx, Q, d, m, k, K=vr.PRODUCTION_K)


@pytest.mark.parametrize("regime", vr.BUILD_REGIMES)
@pytest.mark.parametrize("form", list(vr.BUILD_FORMS))
def test_build_regimes_exhibit_their_edge(oracle, regime, form):
    d, frm, s, k = vr.BUILD_FORMS[form]
    with np.errstate(all="ignore"):
        X = vr.build_case(oracle, regime, vr.BUILD_N, d, frm, s, k)
        vr.build_predicate(oracle, regime, X, frm, s, k)


@pytest.mark.parametrize("regime", vr.BUILD_REGIMES)
def test_other_build_inputs_exhibit_their_edge(oracle, regime):
    """... and the rows of the exact-kNN case, of the product quantizer's training (every sub-vector) and of the grouped index"""
    with np.errstate(all="ignore"):
        n, d = vr.KNN_SHAPE
        vr.build_predicate(oracle, regime, vr.build_case(oracle, regime, n, d, 0, d, 16), 0, d, 16)
        n, d, m, k = vr.PQ_BUILD
        X = vr.build_case(oracle, regime, n, d, 0, d // m, k)
        for f, u in po.subvectors(d, m)[: 1 if regime == "degenerate" else m]:      # (its constant and zero columns: the first)
            vr.build_predicate(oracle, regime, X, f, u - f, k)
        if regime in vr.GROUPED_REGIMES:
            for n, d, groups, m, k, limit, K in vr.GROUPED_PATHS.values():
                vr.build_predicate(oracle, regime, vr.build_case(oracle, regime, n, d, 0, d, groups), 0, d, groups)


def test_tight_rows_of_the_exact_knn_case(oracle):
    n, d = vr.KNN_SHAPE
    cents, idx, Q = vr.query_case(oracle, "tight", n, d, *vr.KNN_TIGHT_MK, 12)
    vr.query_predicate(oracle, "tight", cents, idx, Q, d, *vr.KNN_TIGHT_MK, K=10)


@pytest.mark.parametrize("form,regime", fs.CASES)
def test_filter_stage_cases_meet_their_preconditions(oracle, form, regime):
    """What test_gpu_filter_stage.py needs of its data, from the oracle alone: for every bound of every case the rows a
    sound and tight stage may keep (the upper set) are at most a quarter of the range and fit one survivor sub-queue
    -- but for the combinations filter_stage_ref.LOOSE names -- and a faithful numpy model of the stage passes every
    check of the GPU test."""
    ref = fs.reference(oracle, form, regime)
    wide = form in fs.WIDE_FORMS
    for frm, until in fs.ranges():
        tau = ref.taus(frm, until)
        for nadd in ((4,) if wide else (4, 2)):
            qmax = fs.qmax_of(form, nadd)
            ref.preconditions(frm, until, tau, qmax)
            levels = fs.model_levels(ref, tau, qmax, wide=wide)
            fs.check_stage(ref, frm, until, tau, qmax, fs.CAP, *fs.model_stage(ref, frm, until, levels, qmax), levels)


@pytest.mark.parametrize("form,regime,nadd,broken", [
    ("m16", "tight", 4, "widen"), ("m100", "tight", 2, "widen"), ("m16", "offset", 4, "widen"), ("k5", "tight", 4, "widen"),
    ("m16", "large", 4, "shrink"), ("m16", "mixed_mild", 4, "shrink"), ("m16", "mixed_mild", 2, "shrink"),
    ("m16", "mixed", 4, "budget"), ("k5", "tight", 2, "budget")])
def test_filter_stage_checks_reject_a_broken_stage(oracle, form, regime, nadd, broken):
    """The checks are not vacuous: a model of qt_quantize without the 2 m_pad u widening of tau, without the 2^-21 shrink of
    the reciprocal (at the bounds of reciprocal_edge_taus), or with a budget test off by one in the generous direction
    fails them, and the faithful model passes at the same bounds."""
    ref = fs.reference(oracle, form, regime)
    frm, until = fs.ranges()[0]
    qmax = fs.qmax_of(form, nadd)
    tau = ref.taus(frm, until)
    if broken == "shrink":
        tau, found = fs.reciprocal_edge_taus(ref, qmax, frm, until)
        assert found.sum() >= 6

    def run(extra=0, **mutation):
        levels = fs.model_levels(ref, tau, qmax, **mutation)
        fs.check_stage(ref, frm, until, tau, qmax, fs.CAP, *fs.model_stage(ref, frm, until, levels, qmax, extra), levels)
    run()
    with pytest.raises(AssertionError):
        run(**({"extra": -1} if broken == "budget" else {broken: False}))


@pytest.mark.parametrize("name", gs.FINITE)
def test_grouped_stage_cases_meet_their_preconditions(oracle, name):
    """What test_gpu_grouped_stage.py needs of its data, without a GPU: on a numpy model of the pre-selection every query's
    upper set holds at most a third of its searched rows (but for grouped_stage_ref.LOOSE) and fewer than GF_CAP rows,
    every regular case has a query with 64 searched rows, no certificate sits on its edge, and the model passes every
    check of the GPU test."""
    cs = gs.case(oracle, name)
    out = gs.stage_model(cs)
    gs.preconditions(cs, out)
    stats, worst, certified, edges = gs.check_stage(cs, out, oracle)
    assert edges == 0 and worst <= 1.0
    assert name not in gs.REGULAR or name in gs.LOOSE + ("k63",) or certified[0] > 0      # (K = 63: ek IS the 64th distance)


@pytest.mark.parametrize("name,broken", [("m3", "lim")] + [(n, "margin") for n in ("m16", "m5", "g90", "b17")]
                         + [(n, "padding") for n in ("m16", "g90", "b17")])
def test_grouped_stage_checks_reject_a_broken_stage(oracle, name, broken):
    """The checks are not vacuous: a model of gf_filter whose limit lacks its `+ 2`, of gf_quant whose budget lacks the
    margin, or of gf_filter with a limit for a tile's padding slots fails them.  (The limit: on m3 alone.  A row's m + 1 levels
    are rounded down, half a step each on average, so with more tables no row the checks insist on comes within reach of
    a limit two steps lower.)"""
    cs = gs.case(oracle, name)
    mutation = {"lim": dict(lim_plus=0), "margin": dict(with_margin=False), "padding": dict(pad_limit=1)}[broken]
    with pytest.raises(AssertionError):
        gs.check_stage(cs, gs.stage_model(cs, **mutation), oracle)
