"""The exact scan's shared pruning thresholds (scan.hip, scan_body) and the ScanTuning keys that shape its launch:
GULON_SCAN_BLOCKS, GULON_SCAN_PRUNE, GULON_SCAN_PRUNE_FROM, and GULON_FILTER_BLOCKS for the filter.

Wave 0 of a workgroup trades its thresholds with the other workgroups of its query tile once per 32 row blocks of its
own walk, so a chunk needs 512 row blocks before that code runs at all.  Every case here asserts through scan_ref.py
(checked by hand in test_scan_ref_host.py) that its launch has two or more chunks and one or more exchanges per wave,
then asks one handle the same questions at every knob setting: each answer must be the answer at the default knobs --
rows, distance bits, counts and flags -- and that one is checked against the oracle.  GULON_SCAN_FILTER=0 per handle
keeps the filter out; gulon_index_filter_stats shows that no filter tile ran.

The indexes are built so that a wrong threshold changes an answer instead of slowing the scan down:
  planted    queries alternate between decoded code rows (distances of a few units) and random vectors scaled by four
             (distances of thousands) inside one query tile.  For every query the nearest codes there are (one byte of
             its best code changed, nearest first) are dealt to the LAST rows of every chunk, behind the exchange, and the
             next-nearest ones fill two row blocks that one wave walks first: that wave's list is full at once, the
             thresholds are as tight as they may be when they are traded, and the answer arrives afterwards.  Query 0
             has three rows tied at its 64th distance: two early in the last chunk, one at the very end of chunk 0, in a
             row block of its own -- the row with the smallest id, so the one that belongs in the answer, reaches its
             wave when the threshold already EQUALS its distance.
  ties       every row has a twin in the other half of the index; and an index with one centroid, where all rows tie
  nonfinite  NaN and inf codebook entries, NaN, inf and overflowing queries: the thresholds are compared as unsigned bits
"""
import ctypes as C

import numpy as np
import pytest

import merge_ref as mr
import scan_ref as R
from conftest import bits
from test_gpu_filter import _check_nonfinite, tune          # noqa: F401  (tune: the filter's small stage settings)
from test_gpu_query import _check, _make, _same_up_to_ties

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
PLANT = 64                        # rows planted per query and chunk: K + 1 at the largest K of one scan
COMPUTE_UNITS = 256               # of an MI355X


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


class World:
    """One index and its queries: cents, idx [m][n], Q [B][d], and what is known about them."""
    finite = True
    note = None


def _set(ix, **knobs):
    from gulon_amd import native as N
    for key, v in knobs.items():
        N.check(N.lib().gulon_index_tuning(ix._h, key.encode(), int(v)))


def _filter_tiles(ix):
    from gulon_amd import native as N
    t, r = C.c_int32(-1), C.c_int32(-1)
    N.check(N.lib().gulon_index_filter_stats(ix._h, C.byref(t), C.byref(r)))
    return t.value


def _index(g, w):
    pq = g.ProductQuantizer.from_flat(w.k, w.d, w.m, w.cents)
    coder = pq.coder_factory(w.n)
    enc = g.EncodedMatrix(coder, [coder.build_code(np.ascontiguousarray(w.idx[j])) for j in range(w.m)])
    return g.PQIndex(pq, enc)


def _decode(w, code):
    from gulon_amd.vectors import subvector_bounds
    fr, un = subvector_bounds(w.d, w.m)
    out = np.zeros(w.d, np.float32)
    for j in range(w.m):
        s = un[j] - fr[j]
        out[fr[j]:un[j]] = w.cents[w.k * fr[j] + code[j] * s: w.k * fr[j] + (code[j] + 1) * s]
    return out


def _all_distances(oracle, w, Q):
    """The distance of every row to every query from the ORACLE's tables, summed as Index.scala does: quantizer by
    quantizer in binary32.  [B][n]."""
    T = oracle.prepare_query(w.cents, w.d, w.m, w.k, Q)
    out = np.zeros((len(Q), w.n), np.float32)
    for q in range(len(Q)):
        acc = np.zeros(w.n, np.float32)
        for j in range(w.m):
            acc = acc + T[q, j][w.idx[j]]
        out[q] = acc
    return out


def _shape_of(w, B, frm, until, blocks):
    lay = R.layout(w.m)
    return R.scan_shape(frm, until, B, lay.w, lay.nsub, blocks)


def _blocks_value(w, B, spec):
    kind, v = spec
    return v if kind == "abs" else v * -(-B // R.layout(w.m).qt)


# ---- worlds -------------------------------------------------------------------------------------------------------------

def _start(name, seed):
    w = World()
    w.name = name
    w.d, w.m, w.k, w.n, w.mult = R.THRESHOLD_CASES[name]
    w.qt = R.layout(w.m).qt
    w.B1, w.B = w.qt + 1, 2 * w.qt + 3                    # a ragged second tile; three tiles, the last one ragged
    w.rng = np.random.default_rng(seed)
    w.cents = w.rng.standard_normal(w.k * w.d).astype(np.float32)
    w.idx = w.rng.integers(0, w.k, (w.m, w.n)).astype(np.int32)
    return w


def _mixed_queries(w, near_codes, first_near=0):
    """Even queries (and the first `first_near`): decoded code rows, whose nearest distance is 0 or close to it; the
    others far away, scaled by four.  w.near says which is which."""
    Q = (4.0 * w.rng.standard_normal((w.B, w.d))).astype(np.float32)
    w.near = np.array([q % 2 == 0 or q < first_near for q in range(w.B)])
    for q in np.flatnonzero(w.near):
        Q[q] = _decode(w, near_codes[q])
    return Q


def planted_world(oracle, name):
    """See the module's docstring.  The positions come from scan_ref for the launch at GULON_SCAN_BLOCKS = mult * ntiles."""
    w = _start(name, 20261021)
    shape = _shape_of(w, w.B1, 0, w.n, w.mult * 2)
    nch = shape.nchunks
    assert nch == w.mult and all(R.exchanges_of_chunk(shape, c) >= 1 for c in range(nch))
    # the queries that share the tie query's table entries (its sub-table) are near ones: none of them keeps the tie
    # row's block alive at a pruning checkpoint
    w.Q = _mixed_queries(w, w.rng.integers(0, w.k, (w.B, w.m)), first_near=R.layout(w.m).w)
    w.tie_query = 0
    T = oracle.prepare_query(w.cents, w.d, w.m, w.k, w.Q).astype(np.float64)
    nb = min(4, w.m)               # bytes below the first pruning checkpoint: the partial sum there is the whole distance
    # the rows behind the first exchange of every chunk, last row first; the very last one of chunk 0 is behind every
    # exchange of chunk 0
    pools = [list(R.rows_of_blocks(R.blocks_after_exchange(shape, c), 0, w.n)[::-1]) for c in range(nch)]
    last0 = R.rows_of_blocks(R.blocks_after_exchange(shape, 0, R.exchanges_of_chunk(shape, 0)), 0, w.n)
    w.tie_row = int(pools[0][0])
    assert w.tie_row == last0[-1] and w.tie_row % 64 == 63
    del pools[0][:64]              # the tie row's block holds nothing else that was planted
    w.late = {}
    for q in range(w.B):
        best = T[q].argmin(axis=1)
        cost = T[q, :nb, :] - T[q, np.arange(nb), best[:nb]][:, None]
        cost[np.arange(nb), best[:nb]] = np.inf
        fam = [(int(o) // w.k, int(o) % w.k) for o in np.argsort(cost.reshape(-1), kind="stable")[:nb * (w.k - 1)]]

        def put(rows, members):
            assert len(rows) == len(members)
            for r, (j, c) in zip(rows, members):
                w.idx[:, r] = best
                w.idx[j, r] = c

        slots = [R.rows_of_blocks(R.wave_slot_blocks(shape, c, q, 2), 0, w.n) for c in range(nch)]
        assert all(len(s) == 128 for s in slots)
        if q == w.tie_query:
            # 63 rows and two copies of the 64th in the blocks one wave of the LAST chunk walks first; a third copy of
            # the 64th at the very end of chunk 0; farther codes everywhere else
            put(slots[nch - 1], fam[:PLANT] + fam[PLANT - 1:PLANT] + fam[PLANT:2 * PLANT - 1])
            put([w.tie_row], fam[PLANT - 1:PLANT])
            rest = fam[2 * PLANT - 1:]
            for c in range(nch - 1):
                put(slots[c], rest[c * 128:(c + 1) * 128])
            continue
        true, decoys = fam[:PLANT * nch], fam[PLANT * nch:(PLANT + 128) * nch]
        assert len(decoys) == 128 * nch
        w.late[q] = []
        for c in range(nch):
            rows = [int(pools[c].pop(0)) for _ in range(PLANT)]
            put(rows, true[c::nch])
            put(slots[c], decoys[c::nch])
            w.late[q] += rows
    return w


def check_planted(w, dist):
    """The construction did what it was meant to: every query's 64 nearest rows sit behind an exchange, spread over all
    chunks; the tie query's 64th, 65th and 66th distances are equal and the row that wins the tie is the planted one."""
    for q in range(w.B):
        first = mr.order(dist[q], np.arange(w.n))[:PLANT + 2]
        if q == w.tie_query:
            assert first[PLANT - 1] == w.tie_row
            assert dist[q, first[PLANT - 2]] < dist[q, first[PLANT - 1]] == dist[q, first[PLANT]] == dist[q, first[PLANT + 1]]
            assert (first[:PLANT - 1] > w.tie_row).all() and (first[PLANT:] > w.tie_row).all()
        else:
            assert set(first[:PLANT].tolist()) <= set(w.late[q]), q
    near, far = dist[w.near].min(axis=1), dist[~w.near].min(axis=1)
    assert w.near[w.tie_query] and len(far) >= 1
    assert near.max() * 16 < far.min(), (near.max(), far.min())      # two scales inside one tile


def mixed_world(oracle, name):
    """Random codes (with five centroids per quantizer every code occurs about a hundred times: ties everywhere), queries
    of two scales inside one tile."""
    w = _start(name, 20261022)
    w.Q = _mixed_queries(w, w.idx[:, w.rng.integers(0, w.n, w.B)].T)
    return w


def ties_world(oracle, name):
    """Every row of the first half has a twin in the second half, which another chunk scans: the K-th and (K+1)-th
    distances are equal for every odd K.  Even queries are decoded rows (two rows at distance exactly 0)."""
    w = _start(name, 20261023)
    w.idx[:, w.n - w.n // 2:] = w.idx[:, :w.n // 2]
    w.Q = _mixed_queries(w, w.idx[:, w.rng.integers(0, w.n, w.B)].T)
    w.Q[1::2] *= np.float32(0.25)
    return w


def nonfinite_world(oracle, name):
    w = _start(name, 20261024)
    from gulon_amd.vectors import subvector_bounds
    fr, un = subvector_bounds(w.d, w.m)
    w.cents[w.k * fr[0] + 1 * (un[0] - fr[0])] = np.nan                     # quantizer 0, centroid 1
    w.cents[w.k * fr[2] + 3 * (un[2] - fr[2]) + (un[2] - fr[2] - 1)] = np.inf   # quantizer 2, centroid 3
    w.Q = w.rng.standard_normal((w.B, w.d)).astype(np.float32)
    w.Q[1, min(3, w.d - 1)] = np.nan            # every distance NaN
    w.Q[w.B - 1, :] = 1e30                      # every distance overflows to +inf
    w.Q[w.B - 2, w.d - 1] = np.inf              # inf - c = inf
    w.Q[w.B - 3, 0] = -np.inf
    w.finite = False
    return w


# ---- query forms --------------------------------------------------------------------------------------------------------

class Form:
    def __init__(self, label, kind, K, B, ranges):
        self.label, self.kind, self.K, self.B, self.ranges = label, kind, K, B, ranges

    def run(self, ix, w, dev):
        if self.kind == "query":
            (frm, until), = self.ranges
            return tuple(np.array(a) for a in ix.batch_query_raw(self.K, w.Q[:self.B], frm, until))
        return tuple(dev.partial(ix, self.B, self.K, frm, until) for frm, until in self.ranges)


def forms_of(w):
    n = w.n
    whole, cut = [(0, n)], [(37, n - 29)]                       # the cut goes through the first and the last 64-row block
    f = [Form("K=1", "query", 1, w.B1, whole), Form("K=10", "query", 10, w.B1, whole),
         Form("K=63", "query", 63, w.B1, whole), Form("cut range", "query", 10, w.B1, cut),
         Form("three tiles", "query", 10, w.B, whole)]
    if w.finite:
        split = 100032 if n == 200000 else 66048                # two halves; or 1032 row blocks and a short rest
        f += [Form("K=64", "query", 64, w.B1, whole), Form("K=200", "query", 200, w.B1, whole),
              Form("partial lists", "partial", 63, w.B1, [(0, split), (split, n)])]
    return f


class Dev:
    """Device buffers for the partial lists of one world."""

    def __init__(self, w):
        from gulon_amd import native as N
        self.N, self.L = N, N.lib()
        self.q, self.v, self.i = C.c_void_p(), C.c_void_p(), C.c_void_p()
        N.check(self.L.gulon_dev_malloc(C.byref(self.q), w.Q.nbytes))
        N.check(self.L.gulon_dev_malloc(C.byref(self.v), w.B * 64 * 4))
        N.check(self.L.gulon_dev_malloc(C.byref(self.i), w.B * 64 * 4))
        N.check(self.L.gulon_memcpy_h2d(self.q, w.Q.ctypes.data_as(C.c_void_p), w.Q.nbytes))

    def partial(self, ix, B, K, frm, until):
        N, L = self.N, self.L
        N.check(L.gulon_index_scan_partial_dev(ix._h, self.q, B, K, frm, until, self.v, self.i, None))
        N.check(L.gulon_device_synchronize())
        v, i = np.zeros((B, K + 1), np.float32), np.zeros((B, K + 1), np.int32)
        N.check(L.gulon_memcpy_d2h(v.ctypes.data_as(C.c_void_p), self.v, v.nbytes))
        N.check(L.gulon_memcpy_d2h(i.ctypes.data_as(C.c_void_p), self.i, i.nbytes))
        return v, i

    def close(self):
        for p in (self.q, self.v, self.i):
            self.N.check(self.L.gulon_dev_free(p))


def _same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def assert_identical(form, got, ref, what):
    if form.kind == "partial":
        for (gv, gi), (rv, ri) in zip(got, ref):
            assert np.array_equal(gi, ri) and _same_bits(gv, rv), (form.label, what)
        return
    gi, gd, gc, gf = got
    ri, rd, rc, rf = ref
    assert np.array_equal(gc, rc) and np.array_equal(gf, rf), (form.label, what)
    for q in range(len(rc)):
        assert np.array_equal(gi[q, :rc[q]], ri[q, :rc[q]]), (form.label, what, q)
        assert _same_bits(gd[q, :rc[q]], rd[q, :rc[q]]), (form.label, what, q)


def _nearest(dq, frm, until, count):
    """The rows of [frm, until) that can be among the `count` first in (distance, row id) order: (distances, rows)."""
    seg, rows = dq[frm:until], np.arange(frm, until)
    if len(seg) <= count:
        return seg, rows
    keep = seg <= np.partition(seg, count)[count]
    return seg[keep], rows[keep]


def check_against_oracle(oracle, g, w, form, got, dist):
    """The answer at the default knobs against the oracle: PQIndex.batchQuery up to 63 neighbours (rows where there is no
    tie or the tie was replayed), the (distance, row id) order of the oracle's distances beyond that and for partial
    lists, which get no replay."""
    Q, K = w.Q[:form.B], form.K
    if form.kind == "partial":
        for (v, i), (frm, until) in zip(got, form.ranges):
            for q in range(form.B):
                dd, rows = _nearest(dist[q], frm, until, K + 1)
                o = mr.order(dd, rows)[:K + 1]
                assert np.array_equal(i[q], rows[o]) and np.array_equal(bits(v[q]), bits(dd[o])), (frm, q)
        from gulon_amd.topk import merge_partials
        mi, md, mc, mf = merge_partials(np.stack([v for v, i in got]), np.stack([i for v, i in got]), K)
        oi, od, oc = oracle.pq_batch_query(w.idx, w.d, w.k, w.cents, Q, K)
        assert np.array_equal(mc, oc) and np.array_equal(bits(md), bits(od))
        for q in range(form.B):
            if mf[q] == 0:
                assert mi[q].tolist() == oi[q].tolist()
            else:
                _same_up_to_ties(mi[q], md[q], oi[q])
        return
    (frm, until), = form.ranges
    oi, od, oc = oracle.pq_batch_query(w.idx, w.d, w.k, w.cents, Q, K, frm, until)
    gi, gd, gc, gf = got
    res = [g.index.Result(gi[q, :gc[q]], gd[q, :gc[q]], int(gf[q])) for q in range(form.B)]
    if not w.finite:
        _check_nonfinite(res, oi, od, oc)
        return
    if K <= 63:
        _check(oracle, res, oi, od, oc)
        return
    for q in range(form.B):            # no replay beyond 63: exactly the (distance, row id) order
        ids, dd = mr.peeled_rounds(*_nearest(dist[q], frm, until, K + 65), K)
        ei, ed, ec, ef = mr.peel_final(ids, dd, K)
        assert gc[q] == ec == oc[q] and gf[q] == ef, q
        assert np.array_equal(gi[q], ei) and np.array_equal(bits(gd[q]), bits(ed)), q
        assert np.array_equal(bits(gd[q]), bits(od[q])), q
        if gf[q] == 0:
            assert gi[q].tolist() == oi[q].tolist(), q


def knob_settings(w, full):
    m_pad = R.layout(w.m).m_pad
    blocks = list(dict.fromkeys([("abs", 1), ("tiles", 1), ("tiles", w.mult), ("tiles", 3), ("abs", 4096)]))
    froms = list(dict.fromkeys([-1, 0, 4, 8, m_pad - 4, m_pad, m_pad + 100]))
    if full:
        return [(b, p, f) for b in blocks for p in (0, 1) for f in froms]
    return R.pairwise_cover(blocks, [0, 1], froms)


def run_world(oracle, g, w, settings):
    dist = _all_distances(oracle, w, w.Q) if w.finite else None
    if w.note == "planted":
        check_planted(w, dist)
    ix = _index(g, w)
    dev = Dev(w)
    try:
        _set(ix, GULON_SCAN_FILTER=0)
        forms = forms_of(w)
        for f in forms:        # the launch at the adversarial setting reaches the exchange, or the case is void
            frm, until = f.ranges[0]
            s = _shape_of(w, f.B, frm, until, _blocks_value(w, f.B, ("tiles", w.mult)))
            assert s.nchunks >= 2 and s.exchanges_per_wave >= 1, (f.label, s)
        ref = {}
        for f in forms:
            ref[f.label] = f.run(ix, w, dev)
            check_against_oracle(oracle, g, w, f, ref[f.label], dist)
        for blocks, prune, prune_from in settings:
            for f in forms:
                _set(ix, GULON_SCAN_BLOCKS=_blocks_value(w, f.B, blocks), GULON_SCAN_PRUNE=prune,
                     GULON_SCAN_PRUNE_FROM=prune_from)
                assert_identical(f, f.run(ix, w, dev), ref[f.label], (blocks, prune, prune_from))
        assert _filter_tiles(ix) == 0
    finally:
        dev.close()
        ix.close()


FULL_GRID = "one_word"             # the full cross product of the knobs here, a pairwise cover on the other layouts


@pytest.mark.parametrize("name", list(R.THRESHOLD_CASES))
def test_late_neighbours_and_mixed_scales(oracle, g, name):
    if R.THRESHOLD_CASES[name][2] < 256:
        w = mixed_world(oracle, name)          # 4-bit codes: 625 distinct codes, nothing to plant
    else:
        w = planted_world(oracle, name)
        w.note = "planted"
    run_world(oracle, g, w, knob_settings(w, name == FULL_GRID))


@pytest.mark.parametrize("name", list(R.THRESHOLD_CASES))
def test_ties_at_the_cut(oracle, g, name):
    w = ties_world(oracle, name)
    run_world(oracle, g, w, knob_settings(w, name == FULL_GRID))


def test_one_centroid_every_distance_equal(oracle, g):
    """k = 1: every row has the same distance to a query.  m = 8 takes two 4-byte words per row, 16 queries per tile."""
    w = World()
    w.name, w.d, w.m, w.k, w.n, w.mult = "one centroid", 8, 8, 1, 70000, 2
    w.qt = R.layout(w.m).qt
    w.B1, w.B = w.qt + 1, 2 * w.qt + 3
    w.rng = np.random.default_rng(5)
    w.cents = w.rng.standard_normal(w.k * w.d).astype(np.float32)
    w.idx = np.zeros((w.m, w.n), np.int32)
    w.Q = w.rng.standard_normal((w.B, w.d)).astype(np.float32)
    w.Q[0] = w.cents[:w.d]              # distance 0 to every row
    run_world(oracle, g, w, knob_settings(w, False))


@pytest.mark.parametrize("name", list(R.THRESHOLD_CASES))
def test_nonfinite_distances(oracle, g, name):
    """GULON_SCAN_BLOCKS = 1 and 3 * ntiles are in the grid of every layout (and with them the other values).  These
    queries end in the literal heaps over all rows, which makes them the slowest: the pairwise cover on every layout."""
    w = nonfinite_world(oracle, name)
    settings = knob_settings(w, False)
    assert {("abs", 1), ("tiles", 3)} <= {b for b, p, f in settings}
    run_world(oracle, g, w, settings)


def test_workgroups_that_start_from_published_thresholds(oracle, g):
    """More workgroups than the chip holds at once (each needs 128 KiB of a compute unit's LDS): the late ones load the
    thresholds the finished ones left (the first lines of scan_body).  That they start late rests on residency, which is
    not measured here.  Tile 0 holds near queries only, the other tiles alternate near and far ones."""
    d, m, k, n, B = R.RESIDENCY_CASE
    w = World()
    w.d, w.m, w.k, w.n, w.B = d, m, k, n, B
    w.rng = np.random.default_rng(77)
    w.cents = w.rng.standard_normal(k * d).astype(np.float32)
    w.idx = w.rng.integers(0, k, (m, n)).astype(np.int32)
    w.Q = _mixed_queries(w, w.idx[:, w.rng.integers(0, n, B)].T)
    for q in range(1, 8, 2):
        w.Q[q] = _decode(w, w.idx[:, 1000 + q])
    s = _shape_of(w, B, 0, n, 4096)
    assert s.nchunks >= 2 and s.ntiles * s.nchunks > 4 * COMPUTE_UNITS
    ix = _index(g, w)
    try:
        _set(ix, GULON_SCAN_FILTER=0)
        for K in (1, 10, 63):
            got = ix.batch_query(K, w.Q)
            oi, od, oc = oracle.pq_batch_query(w.idx, d, k, w.cents, w.Q, K)
            _check(oracle, got, oi, od, oc)
            _set(ix, GULON_SCAN_BLOCKS=s.ntiles)                   # one chunk per tile: nothing is published
            one = ix.batch_query(K, w.Q)
            _set(ix, GULON_SCAN_BLOCKS=4096)
            for a, b in zip(got, one):
                assert a.rows.tolist() == b.rows.tolist() and np.array_equal(bits(a.distances), bits(b.distances))
                assert a.flags == b.flags
        assert _filter_tiles(ix) == 0
    finally:
        ix.close()


@pytest.mark.parametrize("n,d,m,k,B", [(100000, 128, 16, 256, 37), (40000, 64, 32, 256, 20)])
def test_filter_blocks(oracle, g, tune, n, d, m, k, B):
    """GULON_FILTER_BLOCKS, the workgroups a filter launch aims for: one, few, the default -- the same answers, the
    oracle's, and the filter ran."""
    K = 10
    cents, idx, pq, enc = _make(oracle, g, n, d, m, k, seed=n + m)
    Q = np.random.default_rng(3).standard_normal((B, d)).astype(np.float32)
    oi, od, oc = oracle.pq_batch_query(idx, d, k, cents, Q, K)
    ix = g.PQIndex(pq, enc)
    try:
        for blocks in (1, 64, 4096):
            _set(ix, GULON_FILTER_BLOCKS=blocks)
            _check(oracle, ix.batch_query(K, Q), oi, od, oc)
            assert _filter_tiles(ix) > 0, blocks
    finally:
        ix.close()
