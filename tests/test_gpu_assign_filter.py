"""The matrix-core filter in front of KMeans.assign (kmeans_mfma.hip), run as a stage of its own
(gulon_selftest_assign_filter: the library's pack_slice_if_filtered + assign_stage1) on rows that sit inside its error
band without being exact ties, in every kernel form the dispatch can choose and on grids whose persistent loops take
more than one step.

Per case, every expectation from the CPU oracle or the float64 restatement in assign_filter_ref.py:
  teeth       the near-tie rows do disagree between the float64 scan and the reference's binary32 chain, and the ordinary
              rows are not all near-ties: a filter that flags nothing fails soundness, one that flags everything fails
              the over-flagging bound
  soundness   a row the filter did not flag holds the reference's answer; a flagged row still holds its pre-filled value
  no over-flagging   a flagged finite row has a scan margin <= 2 band in float64 (the band plus twice the proven error
              E <= band / 2.1; (s + 8) 2^-23 of slack for the kernel's binary32 evaluation of the band: s + 5 roundings)
  end to end  KMeans.assign / par_assign equal the oracle: the flagged rows go through the exact kernels with a row list
"""
import ctypes as C

import numpy as np
import pytest

import assign_filter_ref as R

pytestmark = pytest.mark.gpu

N = 4096 + 64 * 5 + 37      # a ragged last tile, an odd number of tiles, a partial last group of four waves
FRM = 1


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def _stage(g, X, s, Cn, pre):
    """The filter stage alone -> (assignments as it left them, flagged rows, (kind, width))."""
    n, ld = X.shape
    a = pre.copy()
    rows = np.full(n, -1, np.int32)
    nf = C.c_int32(-1)
    form = np.full(2, -1, np.int32)
    rc = g.native.hooks_lib().gulon_selftest_assign_filter(X, n, ld, FRM, s, np.ascontiguousarray(Cn.reshape(-1)),
                                                           Cn.shape[0], a, rows, C.byref(nf), form)
    assert rc == 0, g.native.hooks_lib().gulon_last_error()
    assert 0 <= nf.value <= n
    return a, rows[:nf.value], (int(form[0]), int(form[1]))


def _end_to_end(oracle, g, X, s, Cn, pre=None):
    v = g.Vectors(g.DeviceMatrix.from_host(X), FRM, FRM + s)
    km = g.KMeans(s, Cn)
    if pre is None:
        assert np.array_equal(km.assign(v), oracle.kmeans_assign(X, FRM, s, Cn, 0))
    else:
        assert np.array_equal(km.assign(v, pre.copy()), oracle.kmeans_assign(X, FRM, s, Cn, 0, pre.copy()))
    assert np.array_equal(km.par_assign(v), oracle.kmeans_assign(X, FRM, s, Cn, 25000))


def _check_stage(oracle, g, X, s, Cn, expected_form, pre):
    """Soundness and the over-flagging bound of one run of the stage; returns the flagged rows."""
    n = X.shape[0]
    a, rows, form = _stage(g, X, s, Cn, pre)
    assert form == expected_form
    kind = form[0]
    exp = oracle.kmeans_assign(X, FRM, s, Cn, 0, pre.copy())
    assert rows.size == np.unique(rows).size and (rows.size == 0 or (rows.min() >= 0 and rows.max() < n))
    flagged = np.zeros(n, bool)
    flagged[rows] = True
    bad = np.flatnonzero(~flagged & (a != exp))
    print(f"s={s} k={Cn.shape[0]} n={n} form={form}: flagged {rows.size}, unflagged rows with a wrong answer {bad.size}")
    assert bad.size == 0, (bad[:10], a[bad[:10]], exp[bad[:10]])
    assert np.array_equal(a[rows], pre[rows])
    _, gap = R.scan64(X, FRM, s, Cn, rows=rows)
    bnd = R.band(X, FRM, s, Cn, kind, rows=rows)
    finite = np.isfinite(gap) & np.isfinite(bnd)
    lim = 2.0 * bnd * (1.0 + (s + 8) * 2.0 ** -23)
    over = rows[finite][gap[finite] > lim[finite]]
    print(f"    flagged finite rows {int(finite.sum())}, of them outside 2 band {over.size}")
    assert over.size == 0, over[:10]
    return rows


def _check_teeth(oracle, X, s, Cn, kind, near, rows):
    """From the reference alone, over `rows`: the near-tie rows split the two evaluations, the ordinary rows are not
    all in the band."""
    arg, gap = R.scan64(X, FRM, s, Cn, rows=rows)
    exp = oracle.kmeans_assign(X, FRM, s, Cn, 0)[rows]
    bnd = R.band(X, FRM, s, Cn, kind, rows=rows)
    nr = near[rows]
    disagree = float((arg[nr] != exp[nr]).mean())
    outside = float((gap[~nr] > 2.0 * bnd[~nr]).mean())
    print(f"    teeth: near-tie rows where float64 and the reference disagree {disagree:.3f}, "
          f"ordinary rows outside 2 band {outside:.3f}")
    assert disagree >= 0.05
    assert outside >= 0.10


def _case(oracle, g, s, k, n=N, head=0, outliers=0.0):
    kind, width = R.EXPECTED_FORM[(s, k)]
    X, Cn, near = R.mixed_data(1000 * s + k, n, s + 2, FRM, s, k, head, outliers)
    pre = np.random.default_rng(k).integers(0, k, n).astype(np.int32)
    if kind == R.NO_FILTER:
        _, rows, form = _stage(g, X, s, Cn, pre)
        assert form == (kind, width) and rows.size == 0
    else:
        # (the long cases: the first tiles of the all-ordinary head and everything behind it)
        sub = np.arange(n) if head == 0 else np.concatenate([np.arange(4096), np.arange(head, n)])
        _check_teeth(oracle, X, s, Cn, kind, near, sub)
        _check_stage(oracle, g, X, s, Cn, (kind, width), pre)
    _end_to_end(oracle, g, X, s, Cn)


@pytest.mark.parametrize("s,k", [
    # assign_bf16, compact words: 3 (nkb = 1, 2, 3, k on and off a block edge, the last k that fits LDS), 4, 5
    (1, 3), (4, 16), (8, 32), (8, 33), (8, 64), (8, 65), (8, 576), (9, 448), (10, 40), (11, 352), (13, 100),
    # assign_bf16, three pieces
    (14, 576), (16, 33),
    # assign_mfma<T>: T = 1 (LDS exactly full), 2 (even nkb), 3, 4, 5, 6, 7 (odd nkb), 8
    (2, 3840), (3, 640), (5, 1100), (8, 1536), (9, 449), (11, 353), (14, 577), (16, 832),
    # assign_mfma_stream<T>: T = 16 (the first k past resident; many blocks; s alone decides), 32 (nkb = 1), 64
    (16, 833), (8, 3000), (32, 33), (33, 7), (64, 33), (65, 40), (128, 300),
    # no filter
    (130, 5)])
def test_filter_stage_on_near_tie_rows(oracle, g, s, k):
    _case(oracle, g, s, k)


def test_filter_stage_where_the_centroids_stand_closer_than_the_band(oracle, g):
    """assign_mfma<1> at s = 1, k = 577: between 577 centroids on a line every row is a genuine near-tie; a quarter of
    the ordinary rows lie outside the centroids' hull instead."""
    _case(oracle, g, 1, 577, outliers=0.25)


@pytest.mark.parametrize("s,k,n,head", [
    (2, 5, 524288 + 357, 524288),        # assign_bf16: 2048 workgroups x 4 pairs x 64 rows, then a second grid step
    (2, 577, 524288 + 357, 524288),      # assign_mfma<1>, the same grid
    (33, 7, 131072 + 357, 131072)])      # assign_mfma_stream<32>: 512 workgroups x 4 pairs x 64 rows
def test_filter_stage_on_grids_that_loop(oracle, g, s, k, n, head):
    """The persistent loops' second step: ordinary rows only in the first step (a fault of the second cannot hide among
    rows that are flagged anyway), the near-tie mix behind it."""
    _case(oracle, g, s, k, n=n, head=head)


SHAPES = [(8, 64), (5, 1100), (33, 7)]     # one bf16, one resident, one streaming shape


@pytest.mark.parametrize("s,k", SHAPES)
def test_non_finite_rows_are_flagged_and_leave_their_tiles_alone(oracle, g, s, k):
    form = R.EXPECTED_FORM[(s, k)]
    X, Cn, _ = R.mixed_data(1000 * s + k, N, s + 2, FRM, s, k, head=256)
    special = np.array([5, 70, 150])       # inside tiles of ordinary rows
    X[5, FRM] = np.nan
    X[70, FRM + s - 1] = np.inf
    X[150, FRM + s // 2] = -np.inf
    pre = np.random.default_rng(k).integers(0, k, N).astype(np.int32)
    rows = _check_stage(oracle, g, X, s, Cn, form, pre)
    assert np.isin(special, rows).all()
    # their neighbours: decided rows hold the reference's answer (soundness above), and no more of them are flagged than
    # have a near-tie of their own (the over-flagging bound above) -- in particular not the whole tile
    tile_mates = np.setdiff1d(np.concatenate([np.arange(64 * (r // 64), 64 * (r // 64) + 64) for r in special]), special)
    assert not np.isin(tile_mates, rows).all()
    _end_to_end(oracle, g, X, s, Cn, pre)    # the three rows end as the reference leaves them: untouched or not


@pytest.mark.parametrize("s,k", SHAPES)
def test_infinite_centroid_coordinate_flags_every_row(oracle, g, s, k):
    form = R.EXPECTED_FORM[(s, k)]
    X, Cn, _ = R.mixed_data(1000 * s + k, N, s + 2, FRM, s, k)
    Cn[k // 2 + 1, s // 2] = np.inf          # its offset is infinite: no finite band covers that centroid's distances
    pre = np.random.default_rng(k).integers(0, k, N).astype(np.int32)
    rows = _check_stage(oracle, g, X, s, Cn, form, pre)
    assert rows.size == N
    _end_to_end(oracle, g, X, s, Cn, pre)


@pytest.mark.parametrize("scale", [1e-20, 1e19])
@pytest.mark.parametrize("s,k", SHAPES)
def test_products_that_underflow_and_squares_that_overflow(oracle, g, s, k, scale):
    form = R.EXPECTED_FORM[(s, k)]
    X, Cn, _ = R.mixed_data(1000 * s + k, N, s + 2, FRM, s, k)
    with np.errstate(all="ignore"):
        X = X * np.float32(scale)
        Cn = Cn * np.float32(scale)
    pre = np.random.default_rng(k).integers(0, k, N).astype(np.int32)
    _check_stage(oracle, g, X, s, Cn, form, pre)
    _end_to_end(oracle, g, X, s, Cn, pre)
