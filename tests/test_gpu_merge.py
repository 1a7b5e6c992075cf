"""gulon_topk_merge_dev and gulon_topk_merge on constructed lists (tests/merge_ref.py): every answer of the library
leaves through merge.hip, and a scan of random data never hands it an odd list count, a tie across lists, a list that is
all padding, a real +inf entry next to the padding, a list stride with a gap, more than 64 queries above K = 63, or K at
the limit.  Every comparison is bit for bit: idx, count and flags as ints, dist through `bits`; guard words behind
every output."""
import ctypes as C

import numpy as np
import pytest

import merge_ref as mr
from conftest import bits

pytestmark = pytest.mark.gpu

GUARD_I = 0x5A5A5A5A
GUARD_F = 0x7FC12345                  # a NaN pattern no kernel produces
GAP = 37                              # words between two lists in the "gap" stride
GAP_V, GAP_I = -1.0, 7                # what the gap holds: it would win every merge if it were read


@pytest.fixture(scope="module")
def N():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd.native


class Dev:
    """Device words from gulon_dev_malloc, filled from / read back into numpy arrays of 4-byte items."""

    def __init__(self, N, host):
        self.N, self.nbytes = N, host.nbytes
        self.p = C.c_void_p()
        N.check(N.lib().gulon_dev_malloc(C.byref(self.p), max(host.nbytes, 4)))
        if host.nbytes:
            N.check(N.lib().gulon_memcpy_h2d(self.p, host.ctypes.data_as(C.c_void_p), host.nbytes))

    def read(self, dtype):
        out = np.zeros(self.nbytes // 4, dtype)
        if self.nbytes:
            self.N.check(self.N.lib().gulon_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.p, self.nbytes))
        return out

    def free(self):
        self.N.check(self.N.lib().gulon_dev_free(self.p))


def merge_dev(N, pv, pi, K, stride="dense", with_count_flags=True):
    """gulon_topk_merge_dev on [lists][B][K+1] lists laid out by `stride`: "dense" (list_stride = 0), "exact"
    (b * (K + 1)) or "gap" (GAP more words per list, holding (GAP_V, GAP_I)).  Every output starts as guard words and
    has more of them behind it.  -> (rc, idx[B][K], dist bits[B][K], count[B] | None, flags[B] | None); the guards
    behind the outputs are asserted here."""
    lists, B, keff = pv.shape
    per = B * keff
    step = per + (GAP if stride == "gap" else 0)
    hv = np.full(lists * step, GAP_V, np.float32)
    hi = np.full(lists * step, GAP_I, np.int32)
    for l in range(lists):
        hv[l * step:l * step + per] = pv[l].reshape(-1)
        hi[l * step:l * step + per] = pi[l].reshape(-1)
    bufs = [Dev(N, hv), Dev(N, hi),
            Dev(N, np.full((B + 1) * K, GUARD_I, np.uint32)), Dev(N, np.full((B + 1) * K, GUARD_F, np.uint32)),
            Dev(N, np.full(B + 2, GUARD_I, np.uint32)), Dev(N, np.full(B + 2, GUARD_I, np.uint32))]
    dv, di, oi, od, oc, of = bufs
    rc = N.lib().gulon_topk_merge_dev(dv.p, di.p, lists, {"dense": 0, "exact": per, "gap": step}[stride], B, K, oi.p,
                                      od.p, oc.p if with_count_flags else None, of.p if with_count_flags else None,
                                      None)
    N.check(N.lib().gulon_device_synchronize())
    ri, rd, rc_, rf = oi.read(np.uint32), od.read(np.uint32), oc.read(np.uint32), of.read(np.uint32)
    for b in bufs:
        b.free()
    assert (ri[B * K:] == GUARD_I).all() and (rd[B * K:] == GUARD_F).all()
    assert (rc_[B:] == GUARD_I).all() and (rf[B:] == GUARD_I).all()
    if not with_count_flags:
        assert (rc_ == GUARD_I).all() and (rf == GUARD_I).all()
    return (rc, ri[:B * K].view(np.int32).reshape(B, K), rd[:B * K].reshape(B, K),
            rc_[:B].view(np.int32) if with_count_flags else None, rf[:B].view(np.int32) if with_count_flags else None)


def _assert_ties_occur(pv, pi, K, ef):
    assert (ef & mr.FLAG_INTERIOR_TIE).any() and (ef & mr.FLAG_BOUNDARY_TIE).any(), ef
    assert (ef == 0).any() and (ef == mr.FLAG_INTERIOR_TIE).any(), ef         # ... and a cut that falls between two values
    assert mr.cross_list_ties(pv, pi, K).max() >= 1


# K, lists, B, regime, stride.  K <= 63: merge_lists<true>; above: the pairwise tree (an odd width copies a list
# through; 17 lists: five levels, 64 lists: six; one list: straight to peel_finalize, whose second block B = 70 needs).
CASES = [
    (1, 1, 1, "distinct", "dense"),
    (1, 8, 3, "short", "exact"),
    (2, 3, 3, "ties", "gap"),
    (31, 5, 3, "inf", "dense"),
    (31, 2, 70, "zeros", "gap"),
    (62, 17, 3, "ties", "dense"),
    (62, 2, 1, "short", "exact"),
    (63, 64, 3, "distinct", "gap"),
    (63, 8, 70, "ties", "exact"),
    (63, 3, 3, "short", "dense"),
    (63, 5, 3, "inf", "gap"),
    (63, 1, 3, "zeros", "dense"),
    (64, 1, 3, "short", "dense"),
    (64, 3, 3, "ties", "gap"),
    (64, 64, 3, "distinct", "exact"),
    (65, 5, 70, "ties", "dense"),
    (65, 2, 1, "zeros", "gap"),
    (127, 17, 3, "inf", "exact"),
    (128, 8, 3, "short", "gap"),
    (128, 3, 70, "zeros", "dense"),
    (200, 5, 3, "distinct", "gap"),
    (200, 17, 3, "ties", "exact"),
    (1000, 3, 1, "inf", "dense"),
    (1000, 1, 3, "distinct", "exact"),
    (8190, 3, 3, "ties", "dense"),
    (8190, 5, 1, "short", "gap"),
]


def test_case_table_covers_what_it_names():
    small = [c for c in CASES if c[0] <= 63]
    large = [c for c in CASES if c[0] > 63]
    assert {c[0] for c in small} == {1, 2, 31, 62, 63} and {c[0] for c in large} == {64, 65, 127, 128, 200, 1000, 8190}
    assert {c[1] for c in CASES} == {1, 2, 3, 5, 8, 17, 64} and {1, 3, 5, 17} <= {c[1] for c in large}
    assert {c[2] for c in CASES} == {1, 3, 70} and 70 in {c[2] for c in large}
    for side in (small, large):
        assert {c[3] for c in side} == set(mr.REGIMES)
        assert {c[4] for c in side} == {"dense", "exact", "gap"}


@pytest.mark.parametrize("K,lists,B,regime,stride", CASES)
def test_merge_dev_equals_the_sorted_union(N, K, lists, B, regime, stride):
    pv, pi = mr.make_lists(np.random.default_rng(1000 * K + lists), lists, B, K, regime)
    mr.check_precondition(pv, pi)
    ei, ed, ec, ef = mr.merge_final(pv, pi, K)
    if regime == "ties":
        _assert_ties_occur(pv, pi, K, ef)
    if regime == "short":
        assert (ec < K).any() and ((pi != mr.INT_MAX).sum(axis=2) == 0).any()
    if regime == "inf":
        assert (np.isposinf(ed) & (ei >= 0)).any()
    rc, oi, od, oc, of = merge_dev(N, pv, pi, K, stride)
    assert rc == 0, N.last_error()
    assert np.array_equal(oi, ei)
    assert np.array_equal(od, bits(ed))
    assert np.array_equal(oc, ec)
    assert np.array_equal(of, ef)


@pytest.mark.parametrize("K", [63, 200])
def test_merge_dev_without_count_and_flags(N, K):
    pv, pi = mr.make_lists(np.random.default_rng(K), 3, 3, K, "ties")
    ei, ed, ec, ef = mr.merge_final(pv, pi, K)
    _assert_ties_occur(pv, pi, K, ef)
    rc, oi, od, oc, of = merge_dev(N, pv, pi, K, "exact", with_count_flags=False)
    assert rc == 0, N.last_error()
    assert np.array_equal(oi, ei) and np.array_equal(od, bits(ed))


def test_merge_dev_refuses_k_8191_and_writes_nothing(N):
    K = N.MAX_K_PEELED
    pv, pi = mr.make_lists(np.random.default_rng(1), 1, 1, K, "distinct")
    rc, oi, od, oc, of = merge_dev(N, pv, pi, K, "dense")
    assert rc == N.ERR_UNSUPPORTED
    assert (oi.view(np.uint32) == GUARD_I).all() and (od == GUARD_F).all()
    assert (oc.view(np.uint32) == GUARD_I).all() and (of.view(np.uint32) == GUARD_I).all()


# ---- the host form ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("regime", ["ties", "short"])
@pytest.mark.parametrize("lists", [1, 3])
@pytest.mark.parametrize("K", [1, 63])
def test_merge_partials_equals_the_sorted_union(N, K, lists, regime):
    from gulon_amd.topk import merge_partials
    pv, pi = mr.make_lists(np.random.default_rng(10 * K + lists), lists, 3, K, regime)
    ei, ed, ec, ef = mr.merge_final(pv, pi, K)
    if regime == "ties" and lists > 1 and K > 1:
        _assert_ties_occur(pv, pi, K, ef)
    oi, od, oc, of = merge_partials(pv, pi, K)
    assert np.array_equal(oi, ei) and np.array_equal(bits(od), bits(ed))
    assert np.array_equal(oc, ec) and np.array_equal(of, ef)


def test_merge_partials_refuses_k_64(N):
    from gulon_amd.topk import merge_partials
    pv, pi = mr.make_lists(np.random.default_rng(64), 2, 1, 64, "distinct")
    with pytest.raises(NotImplementedError):
        merge_partials(pv, pi, 64)
