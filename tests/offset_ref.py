"""What the offset-query tests share: the oracle for the distances -- the handle's own ordinary query at
k = the rows of its range, scattered back by row id -- offsets drawn so that equal keys occur, the _dev call, and the
bit-for-bit comparison with csls.offset_query_reference."""
import numpy as np

from conftest import bits

LEVELS = np.array([0.0, 0.125, 0.25, 0.3, 0.5, 0.75, 1.0, 1.5], np.float32)     # the eight offsets in use


def distances_by_row(raw, ids):
    """(rows, distances, counts, flags) of an ordinary query at k = len(ids) -> [b][len(ids)] float32, column j the
    distance to row ids[j] (ids ascending, contiguous)."""
    oi, od, oc = raw[0], raw[1], raw[2]
    assert (oc == len(ids)).all(), oc
    out = np.zeros((len(oi), len(ids)), np.float32)
    for q in range(len(oi)):
        out[q, oi[q] - ids[0]] = od[q]
    return out


def draw_offsets(seed, n, twins=(), inf_share=0.1, keep=None):
    """n offsets from LEVELS, a share of them +inf; twins: (row, copy) pairs that get one offset (their rows are equal, so
    their keys tie); keep: all but these rows are +inf."""
    rng = np.random.default_rng(seed)
    off = LEVELS[rng.integers(0, len(LEVELS), n)]
    off[rng.random(n) < inf_share] = np.inf
    for a, b in twins:
        off[b] = off[a]
    if keep is not None:
        masked = np.full(n, np.inf, np.float32)
        masked[list(keep)] = LEVELS[rng.integers(0, len(LEVELS), len(keep))]
        off = masked
    return off.astype(np.float32)


def same(got, want):
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1]))


def padded(got):
    """-1 and +inf after every query's last entry."""
    oi, ok, oc = got
    return all((oi[q, c:] == -1).all() and np.isposinf(ok[q, c:]).all() for q, c in enumerate(oc))


def run_dev(g, call, q, k, offsets, exclude):
    """A *_query_offset_dev call on device copies: call(d_q, b, k, d_offsets, d_exclude, d_oi, d_ok, d_oc) ->
    (rows [b][k], keys [b][k], counts [b])."""
    from gulon_amd.refine import _DeviceArray
    q = np.ascontiguousarray(q, np.float32)
    b = len(q)
    dev = {name: _DeviceArray() for name in ("q", "off", "ex", "oi", "ok", "oc")}
    try:
        dev["q"].upload(q), dev["off"].upload(np.ascontiguousarray(offsets, np.float32))
        if exclude is not None:
            dev["ex"].upload(np.ascontiguousarray(exclude, np.int32))
        for name, nbytes in (("oi", b * k * 4), ("ok", b * k * 4), ("oc", b * 4)):
            dev[name].ensure(nbytes)
        g.native.check(call(dev["q"].ptr, b, k, dev["off"].ptr, dev["ex"].ptr if exclude is not None else None,
                            dev["oi"].ptr, dev["ok"].ptr, dev["oc"].ptr))
        g.native.check(g.native.lib().gulon_device_synchronize())
        oi = dev["oi"].download(np.zeros((b, k), np.int32))
        ok = dev["ok"].download(np.zeros((b, k), np.float32))
        oc = dev["oc"].download(np.zeros(b, np.int32))
    finally:
        for a in dev.values():
            a.free()
    return oi, ok, oc
