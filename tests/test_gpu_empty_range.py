"""Queries over an empty row range, or for no neighbours, through the device-pointer entry points: final lists of
(-1, +inf) with zero counts and flags, partial lists of K + 1 entries of (+inf, INT32_MAX) -- also above 63 neighbours,
where a scan round is 64 entries long but a shard's list is not --, nothing written outside them, and all of it in the
order of the caller's stream."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ROWS, D, M, B = 200, 16, 4, 3
GUARD, PAD = 0x5A5A5A5A, 256          # guard words on either side of every output
INT_MAX = np.iinfo(np.int32).max
INF_BITS = 0x7F800000


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


@pytest.fixture(scope="module")
def indexes(g):
    """name -> (index, from == until): a flat (k = 16) and a wide (k = 300) index of 200 rows asked for rows [64, 64),
    and the same two shapes with no rows at all asked for [0, 0)"""
    rng = np.random.default_rng(5)
    made = {}
    for name, k, n in (("flat", 16, N_ROWS), ("flat_no_rows", 16, 0), ("wide", 300, N_ROWS), ("wide_no_rows", 300, 0)):
        cents = rng.standard_normal(k * D).astype(np.float32)
        idx = rng.integers(0, k, (M, n)).astype(np.int32)
        pq = g.ProductQuantizer.from_flat(k, D, M, cents)
        coder = pq.coder_factory(n)
        enc = g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(M)])
        made[name] = (g.PQIndex(pq, enc), 64 if n else 0)
    assert made["wide"][0].length == N_ROWS and made["wide_no_rows"][0].length == 0
    yield made
    for ix, _ in made.values():
        ix.close()


class Guarded:
    """`words` 32-bit words on the device between two runs of guard words, all of it GUARD to begin with"""

    def __init__(self, words):
        import torch
        self.words = words
        self.t = torch.full((PAD + words + PAD,), GUARD, dtype=torch.int32, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * PAD

    def body(self):
        return self.t[PAD:PAD + self.words].cpu().numpy()

    def intact(self):
        a = self.t.cpu().numpy()
        return bool((a[:PAD] == GUARD).all() and (a[PAD + self.words:] == GUARD).all())


def _final(g, ix, at, K, stream=None):
    import torch
    N = g.native
    q = torch.zeros((B, D), dtype=torch.float32, device="cuda")
    out = [Guarded(B * K), Guarded(B * K), Guarded(B), Guarded(B)]
    st = None if stream is None else C.c_void_p(stream.cuda_stream)
    N.check(N.lib().gulon_index_batch_query_dev(ix._h, q.data_ptr(), B, K, at, at, out[0].ptr, out[1].ptr, out[2].ptr,
                                                out[3].ptr, st))
    return q, out


def _partial(g, ix, at, K, stream=None):
    import torch
    N = g.native
    q = torch.zeros((B, D), dtype=torch.float32, device="cuda")
    out = [Guarded(B * (K + 1)), Guarded(B * (K + 1))]
    st = None if stream is None else C.c_void_p(stream.cuda_stream)
    N.check(N.lib().gulon_index_scan_partial_dev(ix._h, q.data_ptr(), B, K, at, at, out[0].ptr, out[1].ptr, st))
    return q, out


def _check_final(out):
    oi, od, oc, of = out
    assert (oi.body() == -1).all()
    assert (od.body().view(np.uint32) == INF_BITS).all()
    assert (oc.body() == 0).all() and (of.body() == 0).all()
    assert all(o.intact() for o in out)


def _check_partial(out):
    pv, pi = out
    assert (pv.body().view(np.uint32) == INF_BITS).all()        # every one of the K + 1 entries, not a round's 64
    assert (pi.body() == INT_MAX).all()
    assert pv.intact() and pi.intact()                          # ... and not 128 of them either


CASES = [("flat", 0), ("flat", 5), ("flat", 100), ("flat_no_rows", 0), ("flat_no_rows", 5), ("flat_no_rows", 100),
         ("wide", 5), ("wide", 100), ("wide_no_rows", 5), ("wide_no_rows", 100)]


@pytest.mark.parametrize("name,K", CASES)
def test_final_lists_of_an_empty_range(g, indexes, name, K):
    import torch
    ix, at = indexes[name]
    _, out = _final(g, ix, at, K)
    torch.cuda.synchronize()
    _check_final(out)


@pytest.mark.parametrize("name,K", [c for c in CASES if c[1] > 0])
def test_partial_lists_of_an_empty_range(g, indexes, name, K):
    import torch
    ix, at = indexes[name]
    _, out = _partial(g, ix, at, K)
    torch.cuda.synchronize()
    _check_partial(out)


@pytest.mark.parametrize("name", ["flat", "wide"])
def test_empty_range_calls_run_in_stream_order(g, indexes, name):
    """The outputs are filled with guard words ON the side stream, behind a long matrix product: a call that wrote them
    from anywhere but that stream would be overwritten.  After stream.synchronize() they hold the empty answer."""
    import torch
    ix, at = indexes[name]
    stream = torch.cuda.Stream()
    a = torch.ones((4096, 4096), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(4):
            a = (a @ a).clamp_(0, 1)
        _, fin = _final(g, ix, at, 5, stream)
        _, big = _final(g, ix, at, 100, stream)
        _, part = _partial(g, ix, at, 5, stream)
        _, part_big = _partial(g, ix, at, 100, stream)
    stream.synchronize()
    _check_final(fin)
    _check_final(big)
    _check_partial(part)
    _check_partial(part_big)
