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


def draw_offsets(seed, n, twins=(), inf_share=0.1, keep=None, levels=LEVELS):
    """n offsets from `levels`, a share of them +inf; twins: (row, copy) pairs that get one offset (their rows are equal,
    so their keys tie); keep: all but these rows are +inf."""
    rng = np.random.default_rng(seed)
    off = levels[rng.integers(0, len(levels), n)]
    off[rng.random(n) < inf_share] = np.inf
    for a, b in twins:
        off[b] = off[a]
    if keep is not None:
        masked = np.full(n, np.inf, np.float32)
        masked[list(keep)] = LEVELS[rng.integers(0, len(LEVELS), len(keep))]
        off = masked
    return off.astype(np.float32)


# ---- what test_gpu_offset_paths.py adds: signed offsets, non-finite queries, the flat launcher's arithmetic ---------------

SIGNED_LEVELS = np.concatenate([np.array([-1.5, -0.75, -0.125, -0.0], np.float32), LEVELS])
HUGE = np.float32(3e38)                      # a finite offset that a finite distance of 1e38 or more overflows

LDS_BUDGET = 144 * 1024                      # TABLE_LDS_BUDGET (table_scan.hpp)
FLAT_TABLE_BYTES = 256 << 20                 # the tables of one pass (table_scan.hpp)


def ceil_div(a, b):
    return -(-a // b)


def flat_slots(m, b):
    """offset.hip's choice of query slots for m quantizers and a batch of b, restated: vec = 16 if 16 divides m, else 4;
    ng = ceil(m / vec); m_pad = ng * vec; a slot is max(m_pad * 1024, 16 * 64 * 8) bytes; fit = 144 KiB // slot and
    E_lds = the largest of 8, 4, 2, 1 that is <= fit (0: refused); E = E_lds halved while E > 1 and E / 2 >= b.
    -> (vec, ng, m_pad, E_lds, E)."""
    vec = 16 if m % 16 == 0 else 4
    ng = ceil_div(m, vec)
    m_pad = ng * vec
    fit = LDS_BUDGET // max(m_pad * 256 * 4, 16 * 64 * 8)
    e_lds = 8 if fit >= 8 else 4 if fit >= 4 else 2 if fit >= 2 else fit
    e = e_lds
    while e > 1 and e // 2 >= b:
        e //= 2
    return vec, ng, m_pad, e_lds, e


def flat_chunks(frm, until, b, m):
    """offset_flat_shape restated for rows [frm, until) and b queries: (queries per pass, row chunks of the first pass,
    64-row code blocks per chunk)."""
    _, _, m_pad, _, e = flat_slots(m, b)
    sub = max(1, FLAT_TABLE_BYTES // (m_pad * 256 * 4))
    sub = max(sub // e * e, e)
    groups = ceil_div(min(sub, b), e)
    blocks = ceil_div(until, 64) - frm // 64
    per_chunk = max(1, ceil_div(blocks, min(max(1, ceil_div(2048, groups)), max(1, blocks // 32))))
    return sub, max(1, ceil_div(blocks, per_chunk)), per_chunk


def noisy_queries(seed, X, b, lo, hi):
    """b noisy copies of rows of X[lo:hi] and the row every other one excludes (the one it was made from), else -1."""
    rng = np.random.default_rng(seed)
    made_from = rng.integers(lo, hi, b)
    Q = (X[made_from] + rng.standard_normal((b, X.shape[1])).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    return Q, np.where(np.arange(b) % 2 == 1, made_from, -1).astype(np.int32)


def plant_nearest(offsets, dist, ids, exclude, value):
    """A copy of `offsets` with `value` at every query's nearest candidate row: dist [b][len(ids)], ids the row of every
    column (= its index into offsets), exclude [b]."""
    out = offsets.copy()
    for q in range(len(dist)):
        out[ids[np.argmin(np.where(ids == exclude[q], np.inf, dist[q]))]] = value
    return out


def sign_change_inside(want):
    """Every list is full, starts with a negative key and ends with a positive one: negative keys occur and the step
    from negative to non-negative lies inside the first k."""
    _, keys, counts = want
    return bool((counts == keys.shape[1]).all() and (keys[:, 0] < 0).all() and (keys[:, -1] > 0).all())


NONFINITE_KINDS = ("nan", "inf", "far", "edge")


def nonfinite_queries(Q, at):
    """A copy of Q with the queries at = (nan, inf, far, edge) replaced: one component NaN; one component +inf; every
    component of magnitude 1e19 with the query's signs (d >= 32: every distance sums past the largest float32, 3.4e38);
    every component of magnitude 3e18 (32 <= d <= 37: every distance is finite, about d * 9e36, and adding HUGE
    overflows)."""
    out = np.array(Q, np.float32)
    nan, inf, far, edge = at
    out[nan, 1] = np.nan
    out[inf, 2] = np.inf
    out[far] = np.copysign(np.float32(1e19), Q[far])
    out[edge] = np.copysign(np.float32(3e18), Q[edge])
    return out


def distances_in_steps(query, frm, until, whole):
    """The distances [b][until - frm] of a flat handle's ordinary query whose batch holds non-finite queries.  At k above
    63 a query with NaN distances comes back empty; at k <= 63 it is answered as the reference's heap answers it, with
    the first k rows of the range and their NaN.  So query(k, f, u) -> (rows, distances, counts, ...) is asked over
    steps of 63 rows at k = the rows of the step.  whole: the same query over [frm, until) at k = until - frm; the
    queries it answers in full must have the same distance bits in both."""
    cuts = list(range(frm, until, 63)) + [until]
    steps = [distances_by_row(query(u - f, f, u), np.arange(f, u)) for f, u in zip(cuts, cuts[1:])]
    out = np.concatenate(steps, axis=1)
    full = np.flatnonzero(whole[2] == until - frm)
    assert len(full) >= 2
    at_once = distances_by_row(tuple(a[full] for a in whole[:3]), np.arange(frm, until))
    assert not np.isnan(at_once).any() and np.array_equal(bits(at_once), bits(out[full]))
    return out


def own_or_nan(raw, ids, restated):
    """distances_by_row for an exact handle whose batch holds a NaN query.  The exact index orders by (distance, row), so
    a query whose every distance is NaN is answered with no row at any k, and its distances cannot be read off the
    handle.  restated [b][len(ids)]: the distances restated in numpy (cosmul_ref.exact_distances).  The queries answered
    in full take the handle's distances, which must be restated's bit for bit; the others must be NaN throughout in
    restated and take that row."""
    full = raw[2] == len(ids)
    assert full.sum() >= 2 and np.isnan(restated[~full]).all() and not np.isnan(restated[full]).any()
    out = np.array(restated, np.float32)
    out[full] = distances_by_row(tuple(a[full] for a in raw[:3]), ids)
    assert np.array_equal(bits(out[full]), bits(restated[full]))
    return out


def huge_offsets(seed, n, keepers):
    """HUGE everywhere but at `keepers`, which draw from LEVELS, every eighth of them +inf."""
    rng = np.random.default_rng(seed)
    off = np.full(n, HUGE, np.float32)
    keepers = np.asarray(keepers)
    off[keepers] = LEVELS[rng.integers(0, len(LEVELS), len(keepers))]
    off[keepers[::8]] = np.inf
    return off


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
