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
