"""The key-sorted code copy of the flat filter (conflict_order.hip, GULON_FILTER_SORT).

The filter stages of a query over every row of an index read a copy whose rows are in stable ascending order of
(code 15 << 8) | code 14, dealt to lanes inside 256-row windows, with a 32-bit row id per lane position.  Which lane
holds which row is invisible outside the kernel: ids, distances, counts and flags equal the unsorted path's and the
oracle's bit for bit.  Shapes: 625 row blocks (just above filter_min_rb = 512), a ragged last block and last window,
two full 16-query tiles and a partial one."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import bits
from test_gpu_query import _check, _make
from test_gpu_subset import _filter_stats, _oracle_view

pytestmark = pytest.mark.gpu

D, M, KC, B, K = 32, 16, 256, 40, 10
KNOBS = {"GULON_FILTER_SORT": 1, "GULON_FILTER_CAP": 32768, "GULON_SCAN_FILTER": 1}


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


@pytest.fixture
def tune(g):
    before = {k: os.environ.get(k) for k in KNOBS}
    yield g.tune_live
    g.tune_live(**KNOBS)
    for k, v in before.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _same(x, y):
    """Raw answers (ids, distances, counts, flags), bit for bit."""
    assert np.array_equal(x[0], y[0]) and np.array_equal(bits(x[1]), bits(y[1]))
    assert np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3])


def _results(g, raw):
    from gulon_amd.index import Result
    oi, od, oc, of = raw
    return [Result(oi[i, :oc[i]].copy(), od[i, :oc[i]].copy(), int(of[i])) for i in range(len(oc))]


def _on_off(g, tune, ix, Q, frm=0, until=None):
    """The handle's answer with the sorted copy, without it, and with it again."""
    tune(GULON_FILTER_SORT=1)
    on = ix.batch_query_raw(K, Q, frm, until)
    tune(GULON_FILTER_SORT=0)
    off = ix.batch_query_raw(K, Q, frm, until)
    tune(GULON_FILTER_SORT=1)
    again = ix.batch_query_raw(K, Q, frm, until)
    _same(on, off)
    _same(on, again)
    return on


# ---- the copy itself ----------------------------------------------------------------------------------------------
def _sorted_copy(g, codes, rounds):
    """gulon_selftest_filter_sort of the test-hook library: codes [n][16] -> (copy [npad][16], ids [npad])."""
    from gulon_amd import native as N
    L = C.CDLL(N.HOOKS_LIB_PATH)
    fn = L.gulon_selftest_filter_sort
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    n = len(codes)
    src = np.zeros(((n + 63) // 64 * 64, 16), np.uint8)
    src[:n] = codes
    npad = (n + 255) // 256 * 256
    out, ids = np.full((npad, 16), 0xAA, np.uint8), np.full(npad, -7, np.int32)
    assert 0 == fn(src.ctypes.data, n, rounds, out.ctypes.data, ids.ctypes.data)
    return out, ids


def _codes(name):
    rng = np.random.default_rng(len(name))
    if name == "uniform":
        return rng.integers(0, 256, (40001, 16), dtype=np.uint8)
    if name == "one_cell":                               # every row in one (c15, c14) cell
        c = rng.integers(0, 256, (40000, 16), dtype=np.uint8)
        c[:, 14], c[:, 15] = 9, 200
        return c
    if name == "k4":
        return rng.integers(0, 4, (40001, 16), dtype=np.uint8)
    if name == "n32768":                                 # 64 * 512 rows exactly: no padding
        return rng.integers(0, 256, (64 * 512, 16), dtype=np.uint8)
    return rng.integers(0, 256, (int(name[1:]), 16), dtype=np.uint8)     # "n<rows>"


@pytest.mark.parametrize("rounds", [0, 1])
@pytest.mark.parametrize("name", ["uniform", "one_cell", "k4", "n32768", "n1", "n63", "n64", "n65", "n257"])
def test_sorted_copy(g, name, rounds):
    codes = _codes(name)
    n = len(codes)
    out, ids = _sorted_copy(g, codes, rounds)
    npad = len(ids)
    real = ids >= 0
    # the ids are a bijection onto the rows; the padding is marked, holds no code, and sits in the last window only
    assert np.array_equal(np.sort(ids[real]), np.arange(n))
    assert (ids[~real] == -1).all() and (~real).sum() == npad - n and not (~real)[:npad - 256].any()
    assert not out[~real].any()
    assert np.array_equal(out[real], codes[ids[real]])
    # window w holds exactly rows order[256 w .. 256 w + 255] of THE stable ascending order of the key
    key = codes[:, 15].astype(np.int64) * 256 + codes[:, 14]
    order = np.argsort(key, kind="stable")
    for w in range(npad // 256):
        have = ids[w * 256:(w + 1) * 256]
        assert np.array_equal(np.sort(have[have >= 0]), np.sort(order[w * 256:(w + 1) * 256])), w
    kw = np.where(real, key[np.maximum(ids, 0)], -1).reshape(-1, 256)
    hi = kw.max(axis=1)
    lo = np.where(kw >= 0, kw, 1 << 20).min(axis=1)
    assert (hi[:-1] <= lo[1:]).all()
    if rounds == 0 and n % 256 == 0:                     # no dealing: the copy is the sorted order itself
        assert np.array_equal(ids, order)


# ---- queries ------------------------------------------------------------------------------------------------------
_TRAINED = {}


def _trained(g, kind, n):
    """Synthetic rows of the benchmark's generator, a trained quantizer, the codes on the host, queries = dataset rows."""
    if (kind, n) not in _TRAINED:
        dm = g.DeviceMatrix.synthetic(n, D, kind, 77 + kind, 1000)
        pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(KC, M, 3))
        enc = pq.encode(dm)
        Q = dm.get_rows(np.arange(0, n, n // B, dtype=np.int32)[:B])
        dm.close()
        _TRAINED[(kind, n)] = (pq, enc, np.ascontiguousarray(enc.indices()), pq.flat_centroids(), Q)
    return _TRAINED[(kind, n)]


@pytest.mark.parametrize("n", [40000, 40001])
@pytest.mark.parametrize("kind", [3, 0, 1])
def test_sorted_equals_unsorted_and_oracle(oracle, g, tune, kind, n):
    """The benchmark's data kinds; the queries are dataset rows."""
    pq, enc, idx, cents, Q = _trained(g, kind, n)
    tune(GULON_FILTER_SORT=1)
    ix = g.PQIndex(pq, enc)
    on = _on_off(g, tune, ix, Q)
    assert _filter_stats(ix)[0] > 0                      # the batch went through the filter
    _check(oracle, _results(g, on), *oracle.pq_batch_query(idx, D, KC, cents, Q, K))
    ix.close()


def test_ties_run_the_replay(oracle, g, tune):
    """Half of the rows are copies of the other half: the answers hold exact ties, which the replay resolves in the
    reference's insertion order -- whatever order the sorted copy's lanes reported them in."""
    n = 40001
    cents, idx, pq, enc = _make(oracle, g, n, D, M, KC, seed=3, dup=20000)
    Q = np.random.default_rng(2).standard_normal((B, D)).astype(np.float32)
    tune(GULON_FILTER_SORT=1)
    ix = g.PQIndex(pq, enc)
    on = _on_off(g, tune, ix, Q)
    assert (on[3] != 0).any()
    _check(oracle, _results(g, on), *oracle.pq_batch_query(idx, D, KC, cents, Q, K))
    ix.close()


def test_nan_and_huge_queries(oracle, g, tune):
    n = 40001
    cents, idx, pq, enc = _make(oracle, g, n, D, M, KC, seed=13)
    Q = np.random.default_rng(5).standard_normal((B, D)).astype(np.float32)
    Q[1, 3] = np.nan
    Q[20, :] = 1e30
    Q[39, 30] = np.inf
    tune(GULON_FILTER_SORT=1)
    ix = g.PQIndex(pq, enc)
    on = _on_off(g, tune, ix, Q)
    oi, od, oc = oracle.pq_batch_query(idx, D, KC, cents, Q, K)
    for q in range(B):
        assert on[2][q] == oc[q] and on[0][q, :oc[q]].tolist() == oi[q, :oc[q]].tolist(), q
        e, v = od[q, :oc[q]], on[1][q, :oc[q]]
        assert np.array_equal(np.isnan(v), np.isnan(e)) and np.array_equal(bits(v[~np.isnan(e)]), bits(e[~np.isnan(e)]))
    assert on[3][1] & 8 and on[3][20] & 8 and not on[3][0] & 8
    ix.close()


def test_survivor_queue_overflow(oracle, g, tune):
    """Uniform codes, random queries and 64-entry sub-queues: query tiles overflow or give up and are redone exactly."""
    n = 40001
    cents, idx, pq, enc = _make(oracle, g, n, D, M, KC, seed=9)
    Q = np.random.default_rng(4).standard_normal((B, D)).astype(np.float32)
    tune(GULON_FILTER_SORT=1, GULON_FILTER_CAP=64)
    ix = g.PQIndex(pq, enc)
    on = _on_off(g, tune, ix, Q)
    tiles, redone = _filter_stats(ix)
    assert tiles > 0 and redone > 0
    _check(oracle, _results(g, on), *oracle.pq_batch_query(idx, D, KC, cents, Q, K))
    ix.close()


def test_sub_range_keeps_the_window_ordered_copy(oracle, g, tune):
    """[from, until) cuts blocks and windows: such a query never reads the sorted copy."""
    pq, enc, idx, cents, Q = _trained(g, 3, 40001)
    tune(GULON_FILTER_SORT=1)
    ix = g.PQIndex(pq, enc)
    for frm, until in ((123, 39999), (0, 40000), (1, 40001)):
        on = _on_off(g, tune, ix, Q, frm, until)
        _check(oracle, _results(g, on), *oracle.pq_batch_query(idx, D, KC, cents, Q, K, frm, until))
    ix.close()


# ---- handles ------------------------------------------------------------------------------------------------------
def _native(g, pq, idx):
    coder = pq.coder_factory(idx.shape[1])
    return g.PQIndex(pq, g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(idx.shape[0])]))


def test_view_answers_like_a_fresh_index(oracle, g, tune):
    pq, enc, idx, cents, Q = _trained(g, 3, 40001)
    tune(GULON_FILTER_SORT=1)
    ix = g.PQIndex(pq, enc)
    rows = np.flatnonzero(np.random.default_rng(1).random(40001) < 0.9)      # ~36 000 rows: above filter_min_rb
    view = ix.select(rows=rows)
    on = _on_off(g, tune, view, Q)
    assert _filter_stats(view)[0] > 0
    _check(oracle, _results(g, on), *_oracle_view(oracle, idx, rows, D, KC, cents, Q, K))
    fresh = _native(g, pq, np.ascontiguousarray(idx[:, rows]))
    raw = fresh.batch_query_raw(K, Q)
    mapped = np.where(raw[0] >= 0, rows[np.maximum(raw[0], 0)], raw[0])
    _same(on, (mapped.astype(np.int32), raw[1], raw[2], raw[3]))
    for h in (fresh, view, ix):
        h.close()


def test_updated_index_answers_like_a_fresh_index(oracle, g, tune):
    """add / replace / remove: rows of a second index among, instead of and without rows of the first."""
    pq, enc, idx, cents, Q = _trained(g, 3, 40001)
    tune(GULON_FILTER_SORT=1)
    a = g.PQIndex(pq, enc)
    rng = np.random.default_rng(2)
    idx_b = rng.integers(0, KC, (M, 500)).astype(np.int32)
    b = _native(g, pq, idx_b)
    take = np.arange(40001)
    take = np.delete(take, rng.choice(40001, 300, replace=False))            # remove
    take[rng.choice(len(take), 200, replace=False)] = -1 - np.arange(200)    # replace
    take = np.insert(take, rng.choice(len(take), 300), -1 - np.arange(200, 500))   # add
    merged = a.merged(b, take)
    want = np.where(take >= 0, idx[:, np.maximum(take, 0)], idx_b[:, np.maximum(-1 - take, 0)])
    on = _on_off(g, tune, merged, Q)
    assert _filter_stats(merged)[0] > 0
    fresh = _native(g, pq, np.ascontiguousarray(want))
    _same(on, fresh.batch_query_raw(K, Q))
    _check(oracle, _results(g, on), *oracle.pq_batch_query(np.ascontiguousarray(want), D, KC, cents, Q, K))
    for h in (fresh, merged, b, a):
        h.close()


def test_context_answers_like_its_parent_and_the_switch_flips_per_handle(oracle, g, tune):
    from gulon_amd import native as N
    pq, enc, idx, cents, Q = _trained(g, 0, 40000)
    tune(GULON_FILTER_SORT=1)
    ix = g.PQIndex(pq, enc)
    ctx = ix.context()
    ref = ix.batch_query_raw(K, Q)
    _same(ref, ctx.batch_query_raw(K, Q))
    for v in (0, 1, 0, 1):                               # the context alone, between two batches
        N.check(N.lib().gulon_index_tuning(ctx._h, b"GULON_FILTER_SORT", v))
        _same(ref, ctx.batch_query_raw(K, Q))
        _same(ref, ix.batch_query_raw(K, Q))
    _check(oracle, _results(g, ref), *oracle.pq_batch_query(idx, D, KC, cents, Q, K))
    ctx.close()
    ix.close()
