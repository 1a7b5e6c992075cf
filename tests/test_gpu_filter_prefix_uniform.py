"""The prefix test of the flat filter's main stage on copies whose windows are uniform in code 15 -- and on ones that are not.

In the key-sorted copy a 256-row window usually holds ONE value of code 15: the shape every change to the prefix block
that treats that quantizer apart has to get right (a form that took its entry from scalar registers in such windows was
built, measured and dropped: DESIGN.md 3.1, round 6), and the shape in which the vector L1 serves all 64 lanes of a
look-up from one line.  ONE main stage run through the stage hook (gulon_selftest_filter_stage: copy = 2,
main_stage = 1) must queue

    exactly the rows whose sixteen levels -- the 8-bit levels the hook reports -- sum to qmax - 1 or less,

the set filter_stage_ref.model_stage computes, with every sub-queue within `cap` and no tile flagged; the levels
themselves are held against float64 (check_levels), and every row with D <= tau must be in the set (soundness, no slack).

Shapes: m = 16, d = 32, the codes of quantizers 0-14 random, code 15 laid out per case so that the copy holds uniform
windows, windows in which the value changes, blocks in which it changes, padding inside an otherwise uniform window, and
no uniform window at all.  Queries are decoded rows plus noise; tau rotates as in filter_stage_ref (the (K+1)-th smallest
D, the smallest, the float below it, the 64th) unless the case sets it."""
import numpy as np
import pytest

import filter_stage_ref as fs
import value_regimes as vr
from test_gpu_filter_stage import SORTED, Hooks

pytestmark = pytest.mark.gpu

D_, M_ = 32, 16
N_RUNS = 40960                       # 640 row blocks, 160 windows


class _Ref(fs.Ref):
    """filter_stage_ref.Ref over data made here (its own constructor takes the shape from a named form)"""

    def __init__(self, oracle, k, cents, idx, Q):
        self.form, self.regime, self.n, self.b = "m16", "uniform-windows", idx.shape[1], Q.shape[0]
        self.d, self.m, self.k, self.m_pad = D_, M_, k, fs.m_pad_of(M_, k)
        self.cents, self.idx, self.Q = cents, idx, Q
        self.T = oracle.prepare_query(cents, self.d, self.m, self.k, Q)
        D = np.zeros((self.b, self.n), np.float32)
        R = np.zeros((self.b, self.n), np.float64)
        for j in range(self.m):
            t = self.T[:, j, :][:, idx[j]]
            D = (D + t).astype(np.float32)
            R += t
        self.D, self.R = D, R
        self.mins = np.fmin.reduce(self.T, axis=2).astype(np.float64)
        self.sum_min = np.zeros(self.b, np.float64)
        for j in range(self.m):
            self.sum_min += self.mins[:, j]


def _case(oracle, n, b, k, code15, seed, near_rows=True):
    """code15: (value, rows) pairs, the rows summing to n -- dealt to the rows at random (the copy sorts them);
    near_rows=False: the queries are random vectors instead of noisy decoded rows"""
    rng = np.random.default_rng(seed)
    cents = vr.rows_as_cents(rng.standard_normal((k, D_)).astype(np.float32), D_, M_, k)
    idx = rng.integers(0, k, (M_, n)).astype(np.int32)
    assert sum(c for _, c in code15) == n and all(0 <= v < k for v, _ in code15)
    idx[M_ - 1] = rng.permutation(np.repeat([v for v, _ in code15], [c for _, c in code15])).astype(np.int32)
    idx = np.ascontiguousarray(idx)
    Q = vr.decode(cents, idx[:, rng.choice(n, b, replace=False)], D_, M_, k) if near_rows else np.zeros((b, D_), np.float32)
    Q = np.ascontiguousarray(Q + (0.1 if near_rows else 1.0) * rng.standard_normal(Q.shape).astype(np.float32), np.float32)
    return _Ref(oracle, k, cents, idx, Q)


def _windows(ref):
    """(uniform windows, windows) of the key-sorted copy: 256 consecutive rows in ascending (code 15, code 14) order,
    the last window padded with zero code words"""
    c15 = np.sort(ref.idx[M_ - 1])
    c15 = np.concatenate([c15, np.zeros(-len(c15) % 256, c15.dtype)]).reshape(-1, 256)
    return int((c15 == c15[:, :1]).all(axis=1).sum()), len(c15)


@pytest.fixture(scope="module")
def hooks():
    return Hooks()


def _run(hooks, ref, tau=None, cap=fs.CAP):
    tau = ref.taus(0, ref.n) if tau is None else np.ascontiguousarray(tau, np.float32)
    rows, counts, flagged, levels, info = hooks.flat(ref, 0, ref.n, tau, SORTED, 4, cap, 1)
    qmax = int(info[0])
    assert (info[3], info[4]) == (16, 1)                                   # the one-word form: 16 queries per entry
    assert (counts >= 0).all() and (counts <= cap).all(), "a sub-queue beyond cap"
    assert not flagged.any(), "a tile was flagged"
    fs.check_levels(ref, tau, qmax, levels)
    total = np.zeros((ref.b, ref.n), np.int64)
    for j in range(ref.m):
        total += levels[:, j, :][:, ref.idx[j]]
    sizes = []
    for q in range(ref.b):
        got = rows[q][rows[q] >= 0]
        want = np.flatnonzero(total[q] <= qmax - 1)
        assert counts[q].sum() == len(got) and (np.diff(got) > 0).all(), (q, "counts, order or duplicates")
        assert np.array_equal(got, want), (q, len(got), len(want), np.setxor1d(got, want)[:8].tolist())
        with np.errstate(invalid="ignore"):
            must = np.flatnonzero(ref.D[q] <= tau[q])
        assert len(np.setdiff1d(must, got)) == 0, (q, "dropped rows with D <= tau")
        sizes.append(len(got))
    return np.array(sizes), tau


@pytest.mark.parametrize("b", [16, 40])
def test_value_changes_inside_runs_and_blocks(oracle, hooks, b):
    """Three values of code 15 over 13 001, 14 003 and 13 956 rows: the value changes at sorted positions 13 001 and
    27 004 -- inside a window, and inside a 64-row block of it -- and every other window is uniform.  b = 40: a partial
    last query tile."""
    ref = _case(oracle, N_RUNS, b, 256, ((3, 13001), (77, 14003), (250, 13956)), seed=1)
    assert _windows(ref) == (158, 160)
    sizes, _ = _run(hooks, ref)
    assert sizes[0::4].min() >= fs.K + 1


def test_one_value_for_the_whole_index(oracle, hooks):
    ref = _case(oracle, N_RUNS, 16, 256, ((141, N_RUNS),), seed=2)
    assert _windows(ref) == (160, 160)
    sizes, _ = _run(hooks, ref)
    assert sizes[0::4].min() >= fs.K + 1


def test_no_uniform_window(oracle, hooks):
    """256 values over 4 096 rows, sixteen rows each: every window holds sixteen values"""
    ref = _case(oracle, 4096, 16, 256, tuple((v, 16) for v in range(256)), seed=3)
    assert _windows(ref) == (0, 16)
    sizes, _ = _run(hooks, ref)
    assert sizes[0::4].min() >= fs.K + 1


@pytest.mark.parametrize("values,uniform", [((0,), 160), ((9,), 159), ((0, 5, 9), 157)])
def test_padding_rows_in_the_last_window(oracle, hooks, values, uniform):
    """n = 40 960 - 37: the last window ends in 37 padding places (zero code word, row id -1).  With 0 as the one value
    the window is uniform, padding included -- its padding lanes may pass the test and must not be queued; with 9 the
    padding breaks the window's uniformity."""
    n = N_RUNS - 37
    counts = [n // len(values)] * len(values)
    counts[-1] += n - sum(counts)
    ref = _case(oracle, n, 16, 256, tuple(zip(values, counts)), seed=4 + len(values) + values[0])
    assert _windows(ref) == (uniform, 160)
    sizes, _ = _run(hooks, ref)
    assert sizes[0::4].min() >= fs.K + 1


def test_a_code_book_of_100(oracle, hooks):
    """k = 100: code values below 100, table entries 100-255 of every quantizer unused (level qmax)"""
    ref = _case(oracle, N_RUNS, 16, 100, ((0, 13001), (42, 14003), (99, 13956)), seed=8)
    assert _windows(ref) == (158, 160)
    sizes, _ = _run(hooks, ref)
    assert sizes[0::4].min() >= fs.K + 1


@pytest.mark.parametrize("n", [N_RUNS, 127 * 64])
def test_bounds_so_loose_that_waves_take_whole_blocks(oracle, hooks, n):
    """tau = the distance below which 30 % of the rows lie: far more than a quarter of the rows pass the prefix test,
    so a wave that draws a ninth block takes it whole, in the middle of a uniform window.
    (n = 8 128: one chunk of 127 blocks, 32 runs for sixteen waves, so that waves do draw a third run.)"""
    ref = _case(oracle, n, 16, 256, ((3, n // 3), (77, n // 3 + 5), (250, n - 2 * (n // 3) - 5)), seed=9)
    tau = np.sort(ref.D, axis=1)[:, (3 * n) // 10].copy()
    sizes, _ = _run(hooks, ref, tau, cap=16384)
    assert (sizes * 4 > n).all()


def test_bounds_so_tight_that_nothing_passes(oracle, hooks):
    """Random queries and tau = a quarter of the smallest distance.  A queued row has R <= sum_min + delta (qmax - 1 +
    m_pad) (filter_stage_ref: `not too many`), which is below 78 / 62 tau' < D_min where the budget is positive, and
    where it is not only a row made of every table's minimum could pass: there is none."""
    ref = _case(oracle, N_RUNS, 16, 256, ((3, 13001), (77, 14003), (250, 13956)), seed=10, near_rows=False)
    tau = (ref.D.min(axis=1) * np.float32(0.25)).astype(np.float32)
    assert (ref.R.min(axis=1) > ref.sum_min * (1 + 1e-6)).all()
    sizes, _ = _run(hooks, ref, tau)
    assert (sizes == 0).all()
