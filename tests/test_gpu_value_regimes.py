"""GPU parity at the edges of the value range and with tight bounds, for every kernel form.

The inputs come from tests/value_regimes.py (what each regime is and what it must exhibit is checked on the CPU in
test_oracle_cross.py).  Everything is compared with the CPU oracle bit for bit -- ids and order under the rules of
test_gpu_query._check / test_gpu_filter._check_nonfinite, NaNs by position -- and no tolerance appears anywhere.
Each case prints its filter statistics (`STATS ...`; run with -s to see them)."""
import re

import numpy as np
import pytest

import value_regimes as vr
from conftest import bits
from test_gpu_filter import tune  # noqa: F401  (the small-threshold fixture)
from test_gpu_grouped import _build, _oracle_side
from test_gpu_query import _same_up_to_ties
from test_gpu_wide import _filtered

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def _same_bits(a, b):
    vr.same_bits(a, b, nan_by_position=True)


def _index(g, cents, idx, n, d, m, k):
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    coder = pq.coder_factory(n)
    enc = g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(m)])
    return pq, g.PQIndex(pq, enc)


_stats = _filtered            # (g, ix) -> query tiles of the last batch that took the filter, and those of them redone


def _tuning(g, ix, key, value):
    g.native.check(g.native.lib().gulon_index_tuning(ix._h, key, value))


def _check(res, oi, od, oc, distances_only=False):
    """distances bit for bit (NaNs by position); ids and order are the reference's where there is no tie, where the tie
    was replayed (flag 4) and where the literal heap ran (flag 8); an unreplayed tie leaves the order inside its group open"""
    for q, r in enumerate(res):
        assert len(r) == oc[q], q
        _same_bits(r.distances, od[q, :oc[q]])
        if distances_only:
            continue
        if r.flags == 0 or (r.flags & 4) or (r.flags & 8):
            assert r.rows.tolist() == oi[q, :oc[q]].tolist(), (q, r.flags)
        else:
            _same_up_to_ties(r.rows, r.distances, oi[q, :oc[q]])


def _same_results(a, b):
    for x, y in zip(a, b):
        assert x.rows.tolist() == y.rows.tolist()
        _same_bits(x.distances, y.distances)
        assert x.flags == y.flags


def _fallback_expected(form, regime):
    """Structural, whatever the thresholds: under `subnormal` the byte-code filters' budget is below what an fp32 level can
    resolve (1 / delta overflows, every level is 0), nothing is pruned, the survivor queues overflow and every tile is
    redone (MI355X: 404 of 404 tiles over the eight byte-code forms).  The wide filter prunes there (0 of 640)."""
    return regime == "subnormal" and form in vr.BYTE_FORMS


def _no_claim(form, regime, K):
    """Runs that sit on or next to the first stage's give-up threshold with today's knobs (3 % of the pairs, a 512-row
    sample): whether the tiles are pruned or redone is a matter of tuning, so only `tiles > 0` is asserted and the
    statistics are printed.  There `filtered == exact` may compare the exact scan with itself.  Observed on an MI355X
    (redone/tiles for K = 1, 10, 63 over the full range and K = 10 over the sub-range):
      straddle    m16 5/5 4/5 5/5 2/5, m25 10/10 10/10 10/10 9/10, m64 15/20 20/20 20/20 20/20, other byte forms all
      K = 63      every tile for large, offset, degenerate and tight on m16 .. m100 (uniform or clustered codes, the
                  64th neighbour of a 512-row sample is a loose bound); on m8 and k5 only for tight
      m64, m100   large/offset/degenerate: m64 6..16/20 at K = 1 and all beyond, m100 all; tight at K = 10:
                  m64 16/20 and 10/20, m100 11/40 and 22/40
      k5          mixed 3/3 everywhere (one table holds all the levels, the other three none); tight 3/3 3/3 3/3 2/3
      tight K=10  m16 3/5 and 3/5, m32 1/10 and 0/10
    Everything else -- every wide form, mixed_mild, mixed but on k5, and K = 1 and 10 (on m8 and k5 also K = 63) of large, offset,
    degenerate and tight on m8 .. m36 and k5 -- redid no tile and must keep pruning (`redone < tiles`)."""
    if form in vr.WIDE_FORMS or regime == "mixed_mild":
        return False
    if regime == "mixed":
        return form == "k5"
    if regime == "straddle":
        return True
    if K == 63:
        return regime == "tight" or form not in ("m8", "k5")
    if form in ("m64", "m100"):
        return regime != "tight" or K == 10
    if form == "k5":
        return regime == "tight"
    return regime == "tight" and K == 10 and form in ("m16", "m32")


@pytest.mark.parametrize("regime", vr.QUERY_REGIMES)
@pytest.mark.parametrize("form", list(vr.FORMS))
def test_query_regime(oracle, g, tune, form, regime):
    """Regime x kernel form: Index.prepareQuery, then the filtered scan (small thresholds, so that 20-40 K rows go through
    every filter stage) and the exact scan of the same handle, K in {1, 10, 63}, the full range and one that cuts row
    blocks and ordering windows -- each against the oracle, and filtered == exact.  gulon_index_filter_stats shows
    that the filtered runs took the filter, and, for a finite bound, that the filter was not a detour to the exact scan."""
    n, d, m, k = vr.FORMS[form]
    wide = form in vr.WIDE_FORMS
    with np.errstate(all="ignore"):
        cents, idx, Q = vr.query_case(oracle, regime, n, d, m, k, vr.QUERY_B)
        pq, ix = _index(g, cents, idx, n, d, m, k)
        _same_bits(g.prepare_query(pq, Q), oracle.prepare_query(cents, d, m, k, Q))
        dist_only = wide and regime == "partial_inf"         # (distance, row) rule of the wide index on non-finite distances
        runs = [(K, 0, n) for K in vr.QUERY_KS] + [(10,) + vr.sub_range(n)]
        want = [oracle.pq_batch_query(idx, d, k, cents, Q, K, frm, until) for K, frm, until in runs]
        got, seen = [], []
        for (K, frm, until), (oi, od, oc) in zip(runs, want):
            res = ix.batch_query(K, Q, frm, until)
            tiles, redone = _stats(g, ix)
            print(f"STATS query {form} {regime} K={K} range=[{frm},{until}) tiles={tiles} redone={redone}")
            seen.append((tiles, redone))
            _check(res, oi, od, oc, dist_only)
            got.append(res)
        _tuning(g, ix, b"GULON_SCAN_FILTER", 0)
        for (K, frm, until), (oi, od, oc), res in zip(runs, want, got):
            exact = ix.batch_query(K, Q, frm, until)
            assert _stats(g, ix)[0] == 0
            _check(exact, oi, od, oc, dist_only)
            _same_results(res, exact)
        ix.close()
    for run, ((K, frm, until), (tiles, redone)) in enumerate(zip(runs, seen)):
        assert tiles == vr.QUERY_B if wide else tiles > 0
        if regime == "partial_inf":
            # a query whose K+1 nearest include +inf has no finite bound: it is redone
            kp = oracle.pq_batch_query(idx, d, k, cents, Q, K + 1, frm, until)[1]
            if np.isinf(kp).any():
                assert redone >= 1, (K, tiles, redone)
        elif _fallback_expected(form, regime):
            assert redone == tiles, (K, tiles, redone)
        elif not _no_claim(form, regime, K):
            assert redone < tiles, (K, tiles, redone)


@pytest.mark.parametrize("regime", vr.QUERY_REGIMES)
def test_exact_knn_regime(oracle, g, regime):
    (n, d), B = vr.KNN_SHAPE, 12
    with np.errstate(all="ignore"):
        if regime == "tight":
            cents, idx, Q = vr.query_case(oracle, regime, n, d, *vr.KNN_TIGHT_MK, B)
            X = vr.decode(cents, idx, d, *vr.KNN_TIGHT_MK)             # clustered rows with exact duplicates
        else:
            X = vr.build_case(oracle, regime, n, d, 0, d, 16)
            Q = np.concatenate([X[:4], vr.build_case(oracle, regime, B - 4, d, 0, d, 16, seed=1)])
        for K, frm, until in ((10, 0, n), (63, ) + vr.sub_range(n)):
            res = g.exact_nearest_neighbours(g.DeviceMatrix.from_host(X), Q, K, frm, until)
            oi, od, oc = oracle.exact_knn(X, Q, K, frm, until)
            _check(res, oi, od, oc)


@pytest.mark.parametrize("form", list(vr.PRODUCTION_FORMS))
def test_tight_at_production_thresholds(oracle, g, form):
    """`tight` with the library's own knobs (period 128, stage 1 of 10, sample ~ sqrt(rows), >= 768 row blocks per
    workgroup, ordering windows of four blocks): enough rows for several chunks per tile, no tuning.
    m = 64 and m = 100 (8 and 4 queries per table entry) sit on the first stage's give-up threshold -- MI355X: m = 64: 11 of
    12 tiles redone over the full range, 12 of 12 over the sub-range; m = 100: 17 and 21 of 24 -- so for them only
    `tiles > 0` is asserted; with their coarser levels they are also the two forms whose pruning does not react to a tau
    shrunk by 1e-6: `tight` is tight for m <= 36 and the wide forms, not for these two."""
    n, d, m, k = vr.PRODUCTION_FORMS[form]
    B, K = vr.PRODUCTION_B, vr.PRODUCTION_K
    cents, idx, Q = vr.query_case(oracle, "tight", n, d, m, k, B, per=vr.PRODUCTION_PER)
    pq, ix = _index(g, cents, idx, n, d, m, k)
    for frm, until in ((0, n), vr.sub_range(n)):
        res = ix.batch_query(K, Q, frm, until)
        tiles, redone = _stats(g, ix)
        print(f"STATS production {form} tight K={K} range=[{frm},{until}) tiles={tiles} redone={redone}")
        oi, od, oc = oracle.pq_batch_query(idx, d, k, cents, Q, K, frm, until)
        _check(res, oi, od, oc)
        assert tiles == B if form in vr.WIDE_FORMS else tiles > 0
        if form not in ("m64", "m100"):
            assert redone < tiles, (tiles, redone)      # (observed: none redone)
    ix.close()


@pytest.mark.parametrize("form", list(vr.TIE_FORMS))
def test_tie_replay_under_tight(oracle, g, form):
    """Clustered codes hold equal rows, so most queries meet exact ties among their nearest: every flagged query is
    replayed and ids and order are the reference heap's -- on the first call (segment scans) and on the second one on
    the same handle (the long level through the quantized filter)."""
    n, d, m, k, K, B = vr.TIE_FORMS[form]
    cents, idx, Q = vr.query_case(oracle, "tight", n, d, m, k, B)
    pq, ix = _index(g, cents, idx, n, d, m, k)
    oi, od, oc = oracle.pq_batch_query(idx, d, k, cents, Q, K)
    tied = np.array([len(set(od[q].tolist())) < K for q in range(B)])
    assert tied.sum() >= 32
    for call in range(2):
        gi, gd, gc, gf = ix.batch_query_raw(K, Q)
        print(f"STATS ties {form} call {call}: flagged={int(((gf & 3) != 0).sum())} replayed={int(((gf & 4) != 0).sum())} "
              f"filter={_stats(g, ix)}")
        assert np.array_equal(gc, oc) and np.array_equal(bits(gd), bits(od))
        flagged = (gf & 3) != 0
        assert flagged[tied].all() and flagged.sum() >= 32
        assert ((gf & 4) != 0)[flagged].all()
        assert np.array_equal(gi, oi)                           # every query is either untied or replayed
    ix.close()


# ---- build path ------------------------------------------------------------------------------------------------------
BUILD_CASES = [(r, False) for r in vr.BUILD_REGIMES] + [("offset", True)]


@pytest.mark.parametrize("regime,dup", BUILD_CASES, ids=[r + ("_dup" if dd else "") for r, dd in BUILD_CASES])
@pytest.mark.parametrize("form", list(vr.BUILD_FORMS))
def test_build_regime(oracle, g, form, regime, dup):
    """Regime x assign kernel: KMeans.init, assign, parAssign (one restart of its random stream), fromAssignment and two
    iterations.  Under `subnormal` every comparison of the MFMA filter falls inside the 1e-30 floor of its band and every
    row comes back through the exact kernel; equality with the oracle is the test."""
    d, frm, s, k = vr.BUILD_FORMS[form]
    n = vr.BUILD_N
    with np.errstate(all="ignore"):
        X = vr.build_case(oracle, regime, n, d, frm, s, k, dup=dup)
        v = g.Vectors(g.DeviceMatrix.from_host(X), frm, frm + s)
        km = g.KMeans.init(k, v, 0)
        C0, _ = oracle.kmeans_init(X, frm, s, k, 0)
        _same_bits(km.centroids, C0)
        for rb, fn in ((0, km.assign), (25000, km.par_assign)):
            a = fn(v)
            assert np.array_equal(a, oracle.kmeans_assign(X, frm, s, C0, rb)), rb
        nxt = g.KMeans.from_assignment(k, s, v, a)
        _same_bits(nxt.centroids, oracle.kmeans_from_assignment(X, frm, s, k, a))
        _same_bits(km.iterate(v, 2).centroids, oracle.kmeans_iterate(X, frm, s, C0, 2))


@pytest.mark.parametrize("regime", vr.BUILD_REGIMES)
def test_pq_build_regime(oracle, g, regime):
    n, d, m, k = vr.PQ_BUILD
    with np.errstate(all="ignore"):
        X = vr.build_case(oracle, regime, n, d, 0, d // m, k)      # (exponents sized for one sub-vector)
        dm = g.DeviceMatrix.from_host(X)
        pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(k, m, 2))
        cents, _, _ = oracle.pq_train(X, m, k, 2)
        _same_bits(pq.flat_centroids(), cents)
        enc = pq.encode(dm)
        idx = oracle.pq_encode(X, m, k, cents)
        assert np.array_equal(enc.indices(), idx)
        _same_bits(pq.decode(enc).data, oracle.pq_decode(idx, d, k, cents))


# ---- grouped index ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", vr.GROUPED_REGIMES)
@pytest.mark.parametrize("path", list(vr.GROUPED_PATHS))
def test_grouped_regime(oracle, g, monkeypatch, capfd, path, regime):
    """GroupedIndex over rows of a regime: the by-group pre-selection with 8-bit bound tables (its statistics line shows
    that it ran), the literal heaps (K = 100) and a wide residual code book.  Grouping, residuals and codes are compared
    on the way (_oracle_side)."""
    monkeypatch.setenv("GULON_GROUPED_STATS", "1")
    n, d, groups, m, k, limit, K = vr.GROUPED_PATHS[path]
    B = 24
    with np.errstate(all="ignore"):
        X0 = vr.build_case(oracle, regime, n, d, 0, d, groups)
        X, dm, coarse, gv, pq = _build(oracle, g, n, d, groups, m, k, seed=1, iters=2, X=X0)
        R, cents, offsets = _oracle_side(oracle, X, coarse, gv, pq, n)
        index = g.Index.grouped(gv, pq, g.LimitGroups(limit))
        codes = index.data.indices()
        assert np.array_equal(codes, oracle.pq_encode(R, m, k, pq.flat_centroids()))
        rng = np.random.default_rng(5)
        Q = np.concatenate([X[rng.integers(0, n, B - 2)], vr.build_case(oracle, regime, 2, d, 0, d, groups, seed=1)])
        capfd.readouterr()
        oi, od, oc = index.batch_query_raw(K, Q)
        err = capfd.readouterr().err
        print("STATS grouped", path, regime, err.strip().replace("\n", " | "))
        if path == "by_group":
            assert "by-group filter" in err
            stats = re.search(r"(\d+) queues overflowed, (\d+) queries keep all", err)
            redone = re.search(r"pre-selection: (\d+) of \d+ queries redone", err)
            # the pre-selection must not be a detour to the literal heaps for the whole batch -- except where it is seen
            # to be one (MI355X: `subnormal`: all 24 queues overflow, `offset`: 22 of 24; every query redone literally):
            # the margin underflows / the residuals cancel, and all ~18 000 rows of the searched groups survive
            assert int(stats.group(2)) < B
            if regime in ("subnormal", "offset"):
                assert int(redone.group(1)) == B
            else:
                assert int(redone.group(1)) < B and int(stats.group(1)) < B
        ei, ed, ec = oracle.grouped_query(codes, d, k, pq.flat_centroids(), cents, offsets, Q, K, 0, limit)
        assert np.array_equal(oc, ec)
        for q in range(B):
            assert oi[q, :oc[q]].tolist() == ei[q, :ec[q]].tolist(), q
            _same_bits(od[q, :oc[q]], ed[q, :ec[q]])
        index.close()
