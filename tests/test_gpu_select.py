"""block_radix_select (gulon_amd/csrc/select.hpp) on its own: the `want`-th smallest of a workgroup's keys.

The threshold it finds only decides which rows or groups are looked at again, so an off-by-one in it still ends in the
reference's answers -- through more fallbacks to the literal kernels -- and no end-to-end test sees it.  Here one
workgroup selects from keys chosen to break a single counting pass, in the three forms its callers take
(gulon_selftest_block_select): 0 = 256 threads, keys in registers (gf_quant, gq_select_groups<8 / 40>), 1 = 1024 threads,
keys in registers (the shape of gf_survivors, which keeps a copy of its own: DESIGN.md 9n), 2 = 256 threads, keys
streamed from memory (gq_select_groups<0>)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THREADS = {0: 256, 1: 1024, 2: 256}
LARGEST = {0: 2048, 1: 16384, 2: 3001}


@pytest.fixture(scope="module")
def select():
    import gulon_amd
    from gulon_amd import native as N
    assert gulon_amd.native.device_count() >= 1
    fn = C.CDLL(N.HOOKS_LIB_PATH).gulon_selftest_block_select
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]

    def run(keys, want, form):
        keys = np.ascontiguousarray(keys, np.uint32)
        thr, cnt = np.full(1, 0xDEADBEEF, np.uint32), np.full(1, -7, np.int64)
        assert 0 == fn(keys.ctypes.data, len(keys), want, form, thr.ctypes.data, cnt.ctypes.data)
        return int(thr[0]), int(cnt[0])
    return run


def _check(select, keys, want, form):
    thr, cnt = select(keys, want, form)
    assert thr == int(np.sort(keys)[want - 1]), (form, len(keys), want)
    assert cnt == int((keys <= np.uint32(thr)).sum()), (form, len(keys), want)


def _cases(form):
    """(name, keys, wants): keys below 0xFFFFFFFF (the register forms' "no entry" marker)."""
    rng = np.random.default_rng(100 + form)
    nt, big = THREADS[form], LARGEST[form]
    rand = lambda n: rng.integers(0, 0xFFFFFFFF, n, dtype=np.uint64).astype(np.uint32)
    ends = lambda n: sorted({1, 2, (n + 1) // 2, n - 1, n} & set(range(1, n + 1)))
    out = [("n1", rand(1), [1])]
    for n in (nt - 1, nt + 1, big):                       # one short of / one past the thread count; the form's largest
        out.append(("rand%d" % n, rand(n), ends(n) + [min(n, 64)]))
    out.append(("all_equal", np.full(nt + 1, 0x3F800000, np.uint32), ends(nt + 1)))
    n = 700
    for name, shift in (("low_byte", 0), ("byte1", 8), ("byte2", 16), ("high_byte", 24)):   # one pass decides everything
        k = np.uint32(0x40302010 & ~(0xFF << shift)) | (rng.integers(0, 256, n).astype(np.uint32) << np.uint32(shift))
        out.append((name, k, ends(n) + [64, 255, 256, 257]))
    k = rand(600)
    k[7], k[301] = 0, 0xFFFFFFFE                          # the two ends of the key range
    out.append(("extremes", k, ends(600)))
    k = rand(900)                                         # a run of 300 equal keys across the want-th position
    k[:300] = np.sort(k)[400]
    below = int((k < k[0]).sum())
    out.append(("run300", rng.permutation(k), [below + 1, below + 150, below + 300, min(900, below + 301)]))
    return out


@pytest.mark.parametrize("form", [0, 1, 2])
def test_block_select_finds_the_wanted_key(select, form):
    for name, keys, wants in _cases(form):
        assert len(keys) <= LARGEST[form] or form == 2, name
        for want in wants:
            _check(select, keys, want, form)


# ---- the rest of select.hpp (gulon_selftest_select_parts): keys, the packed subtract, the 64-lane networks, the queues ----
@pytest.fixture(scope="module")
def parts():
    import gulon_amd
    from gulon_amd import native as N
    assert gulon_amd.native.device_count() >= 1
    fn = C.CDLL(N.HOOKS_LIB_PATH).gulon_selftest_select_parts
    fn.restype = C.c_int32
    fn.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64]

    def run(what, a, b, n, out, cap=0):
        a = np.ascontiguousarray(a)
        b = None if b is None else np.ascontiguousarray(b)
        assert 0 == fn(what, a.ctypes.data, a.nbytes, None if b is None else b.ctypes.data, 0 if b is None else b.nbytes, n, cap,
                       out.ctypes.data, out.nbytes)
        return out
    return run


def _pad64(x, fill):
    n = -(-len(x) // 64) * 64
    return np.concatenate([x, np.full(n - len(x), fill, x.dtype)])


def test_ordered_key_round_trip_and_order(parts):
    """ordered_key is a bijection whose unsigned order is the float order: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN"""
    rng = np.random.default_rng(7)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                        0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF,
                        0x3F800000, 0xBF800000], np.uint32)
    bits_in = _pad64(np.concatenate([special, rng.integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)]), np.uint32(0))
    n = len(bits_in)
    out = parts(0, bits_in, None, n, np.zeros(2 * n, np.uint32))
    keys, back = out[:n], out[n:]
    assert np.array_equal(back, bits_in)                                 # the round trip, bit for bit (NaN payloads too)
    mag = (bits_in & 0x7FFFFFFF).astype(np.int64)                        # sign-magnitude order of the bit patterns =
    rank = np.where(bits_in >> 31, -mag - 1, mag)                        # float order, -0 below +0, NaNs at the two ends
    order = np.argsort(rank, kind="stable")
    assert (np.diff(keys[order].astype(np.int64)) >= 0).all()
    assert (np.diff(keys[order].astype(np.int64))[np.diff(rank[order]) > 0] > 0).all()
    f = bits_in.view(np.float32)
    fin = ~np.isnan(f)
    a, b = np.meshgrid(np.flatnonzero(fin)[:200], np.flatnonzero(fin)[:200])
    assert ((f[a] < f[b]) <= (keys[a] < keys[b])).all()                 # a < b as floats  =>  key(a) < key(b)


def test_pk_sub_sat_u16(parts):
    """per 16-bit half max(a - b, 0): the four corner combinations of each half and random words"""
    rng = np.random.default_rng(8)
    corners = np.array([0, 1, 0x7FFF, 0x8000, 0xFFFF, 62, 63, 64, 126, 127, 128], np.uint32)
    lo_a, lo_b, hi_a, hi_b = [x.reshape(-1) for x in np.meshgrid(corners, corners, corners[:5], corners[:5])]
    a = np.concatenate([lo_a | (hi_a << 16), rng.integers(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32)])
    b = np.concatenate([lo_b | (hi_b << 16), rng.integers(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32)])
    a, b = _pad64(a, np.uint32(0)), _pad64(b, np.uint32(0))
    got = parts(1, a, b, len(a), np.zeros(len(a), np.uint32))
    half = lambda x, y: np.maximum(x.astype(np.int64) - y.astype(np.int64), 0).astype(np.uint32)
    assert np.array_equal(got, half(a & 0xFFFF, b & 0xFFFF) | (half(a >> 16, b >> 16) << 16))


def _net_sort(x, lo, hi):
    """sort64 of select.hpp in numpy: rows of 64, pick = lo / hi"""
    lane = np.arange(64)
    for k in (2, 4, 8, 16, 32, 64):
        j = k >> 1
        while j >= 1:
            y = x[:, lane ^ j]
            x = np.where(((lane & k) == 0) == ((lane & j) == 0), lo(x, y), hi(x, y))
            j >>= 1
    return x


def _net_merge(a, b, lo, hi):
    lane = np.arange(64)
    a = lo(a, b[:, 63 - lane])
    for j in (32, 16, 8, 4, 2, 1):
        y = a[:, lane ^ j]
        a = np.where((lane & j) == 0, lo(a, y), hi(a, y))
    return a


def _sort_inputs(rng, dtype):
    draw = (lambda n: rng.standard_normal(n).astype(np.float32)) if dtype == np.float32 else \
        (lambda n: rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64))
    rows = [draw(64) for _ in range(6)]
    rows.append(np.sort(draw(64))[::-1].copy())                           # already descending
    rows.append(np.sort(draw(64)))                                        # already ascending
    rows.append(np.repeat(draw(8), 8))                                    # equal keys
    rows.append(np.full(64, draw(1)[0]))                                  # all equal
    rows.append(rng.permutation(np.repeat(draw(3), [30, 30, 4])))
    return np.stack(rows).astype(dtype)


def test_sort64_and_merge64_float(parts):
    """sort64_asc / merge64_asc against np.sort; with NaNs the expectation is the network's own, step by step, under what
    fminf / fmaxf define (the non-NaN operand of the two): a NaN that meets a number is REPLACED by that number, so the
    result need not be a permutation -- bound_tables relies on NaN distances never reaching a list."""
    rng = np.random.default_rng(9)
    x = _sort_inputs(rng, np.float32)
    n = x.size
    got = parts(2, x, None, n, np.zeros(n, np.float32)).reshape(x.shape)
    assert np.array_equal(got, np.sort(x, axis=1)) and np.array_equal(got, _net_sort(x, np.fmin, np.fmax))
    a, b = np.sort(x, axis=1), np.sort(x[::-1], axis=1)
    got = parts(3, a, b, n, np.zeros(n, np.float32)).reshape(x.shape)
    assert np.array_equal(got, np.sort(np.concatenate([a, b], axis=1), axis=1)[:, :64])
    xn = x.copy()
    xn[0, 5], xn[1, ::7], xn[2, :] = np.nan, np.nan, np.nan
    xn[3, 1::2] = -np.nan
    want = _net_sort(xn, np.fmin, np.fmax)
    got = parts(2, xn, None, n, np.zeros(n, np.float32)).reshape(x.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    assert np.isnan(want[2]).all() and not np.isnan(want[[0, 1, 3]]).any()      # NaNs survive only among themselves
    an = a.copy()
    an[0, 60:], an[1, :] = np.nan, np.nan                                      # (NaNs at a sorted list's end, as a sort leaves none)
    want = _net_merge(an, b, np.fmin, np.fmax)
    got = parts(3, an, b, n, np.zeros(n, np.float32)).reshape(x.shape)
    assert not np.isnan(want).any() and np.array_equal(got, want)


def test_sort64_and_merge64_u64(parts):
    rng = np.random.default_rng(10)
    x = _sort_inputs(rng, np.uint64)
    n = x.size
    got = parts(4, x, None, n, np.zeros(n, np.uint64)).reshape(x.shape)
    assert np.array_equal(got, np.sort(x, axis=1))
    a, b = np.sort(x, axis=1), np.sort(x[::-1], axis=1)
    got = parts(5, a, b, n, np.zeros(n, np.uint64)).reshape(x.shape)
    assert np.array_equal(got, np.sort(np.concatenate([a, b], axis=1), axis=1)[:, :64])


def test_survivor_queues_flat_numbering(parts):
    """SurvivorQueues::count / entry: the sub-queues of a query read as one list, in sub-queue order, over ragged fill
    levels -- empty ones, full ones and counters beyond the capacity (clamped; the overflow is reported)"""
    rng = np.random.default_rng(11)
    cap, nq = 37, 9
    cnt = rng.integers(0, cap + 1, (nq, 16)).astype(np.int32)
    cnt[0] = 0                                                            # nothing queued
    cnt[1] = cap                                                          # every sub-queue full
    cnt[2] = 0
    cnt[2, 15] = 5                                                        # only the last
    cnt[3, ::2] = 0                                                       # every other one empty
    cnt[4, 3], cnt[4, 9] = cap + 1, 100 * cap                             # counters beyond the capacity
    cnt[5, 0] = 1
    cnt[5, 1:] = 0
    queue = rng.integers(0, 1 << 30, (nq, 16, cap)).astype(np.int32)
    out = parts(6, cnt, queue, nq, np.zeros((nq, 2 + 16 * cap), np.int32), cap=cap)
    for q in range(nq):
        kept = np.minimum(cnt[q], cap)
        want = np.concatenate([queue[q, s, :kept[s]] for s in range(16)])
        assert out[q, 0] == len(want) and out[q, 1] == int((cnt[q] > cap).any()), q
        assert np.array_equal(out[q, 2:2 + len(want)], want), q
