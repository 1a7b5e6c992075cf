"""Expressions over the true vectors (csrc/dataset_compose.hip, gulon_exact_index_query_terms in csrc/exact.hip):
the composed vectors bit for bit against expressions.compose_reference, and the expression query against its contract --
the handle's own answer to the composed vector at k + E, the operands dropped, the first k kept.

Tie-free data: standard-normal float32 distances collide now and then, and a tie would be compared through its flags
only.  SEED was searched on the CPU with `tie_free` below -- the distances restated in numpy in the kernels' order of
operations (unfused binary32, coordinates ascending), the DEPTHS[-1] + 1 nearest of every query compared -- for the first
seed whose queries have no two equal among them; the tests assert that no tie flag comes back."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

N_ROWS, D_QUERY, B_QUERY = 1500, 16, 12
DEPTHS = (5, 63, 64, 65, 200)          # k + E: the single pass, its last depth, the first of the one-pass path, ...
SEED = 1
TIES = 3                               # GULON_FLAG_BOUNDARY_TIE | GULON_FLAG_INTERIOR_TIE
WEIGHTS = (1.0, -1.0, 0.3, -1.7)


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def normal(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def three_term_expressions(seed, n=N_ROWS, b=B_QUERY):
    """b expressions of three distinct rows: b - a + c mostly, fractional weights among them."""
    rng = np.random.default_rng(seed)
    out = []
    for q in range(b):
        rows = rng.choice(n, 3, replace=False).tolist()
        w = (1.0, -1.0, 1.0) if q % 3 else tuple(WEIGHTS[int(i)] for i in rng.integers(0, len(WEIGHTS), 3))
        out.append(list(zip(rows, w)))
    return out


def reference_vectors(X, exprs, normalize_terms=False, normalize_query=False):
    from gulon_amd.expressions import compose_reference
    return np.stack([compose_reference(X[[r for r, _ in e]], [w for _, w in e], normalize_terms, normalize_query)
                     for e in exprs])


def tie_free(X, Q, depth):
    """CPU: no two equal among the depth + 1 smallest distances of any query, summed as the kernels sum them."""
    for q in Q:
        acc = np.zeros(len(X), np.float32)
        for e in range(X.shape[1]):
            dx = (q[e] - X[:, e]).astype(np.float32)
            acc = (acc + (dx * dx).astype(np.float32)).astype(np.float32)
        head = np.sort(acc)[:depth + 1]
        if (head[1:] == head[:-1]).any():
            return False
    return True


_WORLD = {}


def world(g):
    """X, its device copy, the expressions, an l2 ExactIndex over all rows: made once."""
    if not _WORLD:
        X = normal(2 * SEED, N_ROWS, D_QUERY)
        dm = g.DeviceMatrix.from_host(X)
        _WORLD.update(X=X, dm=dm, exprs=three_term_expressions(2 * SEED + 1), ix=g.ExactIndex(dm))
    return _WORLD


def compose(g, dm, exprs, nt, nq):
    """gulon_dataset_compose_rows with the flags given (ExactIndex.compose_rows passes its metric's)."""
    from gulon_amd.expressions import to_csr
    N = g.native
    off, rows, w = to_csr(exprs)
    b = len(off) - 1
    out = np.zeros((b, dm.cols), np.float32)
    one_i, one_f = np.zeros(1, np.int32), np.zeros(1, np.float32)
    N.check(N.lib().gulon_dataset_compose_rows(dm._h, off, rows if b else one_i, w if b else one_f, b, int(nt), int(nq),
                                               out.reshape(-1) if out.size else one_f))
    return out


def dropped(raw, exprs, k):
    """The contract on the host: an answer at depth k + E with the term rows removed, the first k kept, padded."""
    oi, od, oc, of = raw
    b = len(exprs)
    ri, rd, rc = np.full((b, k), -1, np.int32), np.full((b, k), np.inf, np.float32), np.zeros(b, np.int32)
    for q, e in enumerate(exprs):
        terms = {r for r, _ in e}
        keep = [p for p in range(oc[q]) if int(oi[q, p]) not in terms][:k]
        rc[q] = len(keep)
        ri[q, :len(keep)], rd[q, :len(keep)] = oi[q, keep], od[q, keep]
    return ri, rd, rc, of


def same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1]))
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])


# ---- compose ---------------------------------------------------------------------------------------------------------

def _mixed_expressions(n, rng):
    """1, 2, 3 and 7 terms; a repeated operand; weights other than +-1."""
    out = []
    for t in (1, 2, 3, 7, 3, 7, 2, 1):
        rows = rng.integers(0, n, t).tolist()
        out.append(list(zip(rows, [WEIGHTS[int(i)] for i in rng.integers(0, len(WEIGHTS), t)])))
    out[4][2] = (out[4][0][0], -1.0)                 # a + b - a
    out[5][6] = (out[5][1][0], 0.3)
    out.append([(n - 1, 1.0), (0, -1.0), (n - 1, 1.0)])
    return out


@pytest.mark.parametrize("d", [1, 3, 128, 256, 257, 300])
def test_compose_equals_the_reference_bit_for_bit(g, d):
    """d straddles the 256-thread coordinate stride (one, then four coordinates per thread); every combination of the
    two normalise flags; ExactIndex.compose_rows passes both for cosine and neither for l2."""
    X = normal(100 + d, N_ROWS, d)
    dm = g.DeviceMatrix.from_host(X)
    exprs = _mixed_expressions(N_ROWS, np.random.default_rng(d))
    assert sorted({len(e) for e in exprs}) == [1, 2, 3, 7]
    for nt in (False, True):
        for nq in (False, True):
            got = compose(g, dm, exprs, nt, nq)
            want = reference_vectors(X, exprs, nt, nq)
            nan = np.isnan(want)               # d = 1: w * (x / |x|) sums to exactly 0, which normalises to NaN
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan])), (nt, nq)
    for metric, flag in (("l2", False), ("cosine", True)):
        ix = g.ExactIndex(dm, metric)
        got, want = ix.compose_rows(exprs), reference_vectors(X, exprs, flag, flag)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))
        assert ix.compose_rows([]).shape == (0, d)                                       # b = 0
        ix.close()
    assert compose(g, dm, [], True, True).shape == (0, d)
    dm.close()


def test_compose_refuses_a_bad_row_on_the_host(g):
    w = world(g)
    for bad in (N_ROWS, -1):
        with pytest.raises(ValueError, match=rf"term 4: row {bad} outside \[0, {N_ROWS}\)"):
            compose(g, w["dm"], [[(1, 1.0), (2, 1.0)], [(3, 1.0), (4, -1.0), (bad, 1.0)], [(N_ROWS + 7, 1.0)]], False, False)
    N = g.native
    one_f = np.zeros(4 * D_QUERY, np.float32)
    rc = N.lib().gulon_dataset_compose_rows(w["dm"]._h, np.array([0, 1, 1], np.int32), np.array([5], np.int32),
                                            np.ones(1, np.float32), 2, 0, 0, one_f)
    assert rc == N.ERR_INVALID_ARGUMENT and "expression 1 is empty" in N.last_error()


def test_compose_dev_answers_a_bad_expression_with_nan_and_the_error_word(g):
    import torch
    w = world(g)
    N, X = g.native, w["X"]
    off = torch.tensor([0, 2, 3, 3, 6], dtype=torch.int32, device="cuda")           # expression 2 has no terms
    rows = torch.tensor([10, 11, N_ROWS, 7, 8, 9], dtype=torch.int32, device="cuda")   # expression 1: a row past the end
    wts = torch.tensor([1, -1, 1, 1, -1, 0.3], dtype=torch.float32, device="cuda")
    out = torch.zeros((4, D_QUERY), dtype=torch.float32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    call = N.lib().gulon_dataset_compose_rows_dev
    N.check(call(w["dm"]._h, off.data_ptr(), rows.data_ptr(), wts.data_ptr(), 4, 0, 0, out.data_ptr(), err.data_ptr(),
                 None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all() and err.item() == 1
    want = reference_vectors(X, [[(10, 1.0), (11, -1.0)], [(7, 1.0), (8, -1.0), (9, 0.3)]])
    assert np.array_equal(bits(got[[0, 3]]), bits(want))
    # good expressions leave the word alone; a null word is allowed
    err.zero_()
    good_off = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    N.check(call(w["dm"]._h, good_off.data_ptr(), rows.data_ptr(), wts.data_ptr(), 1, 1, 1, out.data_ptr(),
                 err.data_ptr(), None))
    N.check(call(w["dm"]._h, off.data_ptr(), rows.data_ptr(), wts.data_ptr(), 4, 0, 0, out.data_ptr(), None, None))
    torch.cuda.synchronize()
    assert err.item() == 0 and np.isnan(out.cpu().numpy()[1]).all()


# ---- query_terms: the contract ---------------------------------------------------------------------------------------

def test_the_seed_is_tie_free_on_the_cpu(g):
    w = world(g)
    assert tie_free(w["X"], reference_vectors(w["X"], w["exprs"]), DEPTHS[-1])


@pytest.mark.parametrize("depth", DEPTHS)
def test_query_terms_is_the_own_answer_with_the_operands_dropped(g, depth):
    w = world(g)
    ix, exprs, k = w["ix"], w["exprs"], depth - 3
    composed = ix.compose_rows(exprs)
    assert np.array_equal(bits(composed), bits(reference_vectors(w["X"], exprs)))
    raw = ix.batch_query_raw(depth, composed)
    assert not (raw[3] & TIES).any() and (raw[2] == depth).all()
    got = ix.batch_query_terms_raw(k, exprs, 3)
    stats = ix.stats()
    same(got, dropped(raw, exprs, k))
    assert (got[2] == k).all()
    for q, e in enumerate(exprs):                              # every operand is near its own expression: dropped
        assert not {r for r, _ in e} & set(got[0][q].tolist())
    if depth > 63:
        assert stats["one_pass"] == len(exprs) and stats["fallback"] == 0 and stats["nonfinite"] == 0
    same(ix.batch_query_expressions_raw(k, exprs), got)         # the partitioned form: all of these have E = 3
    results = ix.batch_query_expressions(k, exprs)
    assert [r.rows.tolist() for r in results] == got[0].tolist()


def test_query_terms_dev_and_cosine_flags(g):
    """The device form on torch's buffers; and both normalise flags: the handle carries no metric, so an l2 handle over
    the same rows answers the normalised composition as it is."""
    import torch
    from gulon_amd.expressions import to_csr
    w = world(g)
    N, ix, exprs, depth = g.native, w["ix"], w["exprs"], 65
    k, b = depth - 3, len(w["exprs"])
    off, rows, wts = (torch.from_numpy(a).cuda() for a in to_csr(exprs))
    oi = torch.full((b, k), 7, dtype=torch.int32, device="cuda")
    od = torch.zeros((b, k), dtype=torch.float32, device="cuda")
    oc, of = torch.zeros(b, dtype=torch.int32, device="cuda"), torch.zeros(b, dtype=torch.int32, device="cuda")
    for flag in (0, 1):
        N.check(N.lib().gulon_exact_index_query_terms_dev(ix._h, off.data_ptr(), rows.data_ptr(), wts.data_ptr(), b, k, 3,
                                                          flag, flag, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                                          of.data_ptr(), None))
        torch.cuda.synchronize()
        composed = compose(g, w["dm"], exprs, flag, flag)
        want = dropped(ix.batch_query_raw(depth, composed), exprs, k)
        same((oi.cpu().numpy(), od.cpu().numpy(), oc.cpu().numpy(), of.cpu().numpy()), want)
    cosine = g.ExactIndex(w["dm"], "cosine")
    same(cosine.batch_query_terms_raw(k, exprs, 3), want)
    cosine.close()


# ---- query_terms: edges ----------------------------------------------------------------------------------------------

def test_a_range_shorter_than_the_depth(g):
    w = world(g)
    frm, until, k = 100, 120, 30
    ix = g.ExactIndex(w["dm"], frm=frm, until=until)
    inside = [[(101, 1.0), (105, -1.0), (119, 1.0)], [(100, 1.0), (110, -1.0), (111, 0.3)]]
    got = ix.batch_query_terms_raw(k, inside, 3)
    raw = ix.batch_query_raw(k + 3, ix.compose_rows(inside))
    assert raw[2].tolist() == [20, 20]
    same(got, dropped(raw, inside, k))
    assert got[2].tolist() == [17, 17] and (got[0][:, 17:] == -1).all() and np.isposinf(got[1][:, 17:]).all()
    assert ((got[0][:, :17] >= frm) & (got[0][:, :17] < until)).all()
    # operands outside the range (rows of the dataset all the same): nothing is dropped
    outside = [[(5, 1.0), (700, -1.0), (1499, 1.0)], [(99, 1.0), (120, -1.0), (121, 1.0)]]
    got = ix.batch_query_terms_raw(5, outside, 3)
    raw = ix.batch_query_raw(8, ix.compose_rows(outside))
    assert np.array_equal(got[0], raw[0][:, :5]) and np.array_equal(bits(got[1]), bits(raw[1][:, :5]))
    assert got[2].tolist() == [5, 5]
    ix.close()


def test_k_zero_and_an_empty_batch(g):
    w = world(g)
    oi, od, oc, of = w["ix"].batch_query_terms_raw(0, w["exprs"], 3)
    assert oi.shape == (B_QUERY, 0) and od.shape == (B_QUERY, 0) and oc.tolist() == [0] * B_QUERY
    oi, od, oc, of = w["ix"].batch_query_expressions_raw(4, [])
    assert oi.shape == (0, 4) and oc.shape == (0,)
    assert w["ix"].batch_query_expressions(4, []) == []


def test_a_depth_above_the_peeled_limit_is_unsupported(g):
    w = world(g)
    assert g.native.MAX_K_PEELED == 8191
    with pytest.raises(NotImplementedError, match="8192 > 8191"):
        w["ix"].batch_query_terms_raw(8189, w["exprs"], 3)
    with pytest.raises(NotImplementedError):
        w["ix"].batch_query_expressions(8190, [[(1, 1.0), (2, -1.0)]])
    assert len(w["ix"].batch_query_expressions(8190, [[(1, 1.0)]])[0].rows) == N_ROWS - 1     # 8191: the last depth


def test_an_answer_does_not_depend_on_the_batch(g):
    """Expressions of one, two and three distinct operands in one batch (a repeated operand counts once): each answer
    equals the one it gets alone."""
    w = world(g)
    ix, k = w["ix"], 70
    mixed = [[(3, 1.0)], [(4, 1.0), (9, -1.0)], [(4, 1.0), (9, -1.0), (4, 0.3)], w["exprs"][0], [(8, -1.7)],
             w["exprs"][1], [(1400, 1.0), (2, 1.0)]]
    oi, od, oc, of = ix.batch_query_expressions_raw(k, mixed)
    assert (oc == k).all()
    for q, e in enumerate(mixed):
        alone = ix.batch_query_expressions_raw(k, [e])
        same(alone, (oi[q:q + 1], od[q:q + 1], oc[q:q + 1], of[q:q + 1]))
        extra = len({r for r, _ in e})
        raw = ix.batch_query_raw(k + extra, ix.compose_rows([e]))
        same(alone, dropped(raw, [e], k))
