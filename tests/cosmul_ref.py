"""What the cosmul tests share: the per-term distances restated in the kernels' order of operations, the
answer lists by expressions.cosmul_reference and np.lexsort, term-list patterns, and the comparison."""
import numpy as np

from conftest import bits

PATTERNS = {"+": (1,), "+-": (1, -1), "+-+": (1, -1, 1), "-+++-": (-1, 1, 1, 1, -1),
            "8": (1, -1, 1, 1, -1, 1, -1, 1)}


def expression(rng, n, signs, repeat=False, lo=0):
    """Distinct rows of [lo, n) under `signs`; repeat: the last term names the first row again."""
    rows = (lo + rng.choice(n - lo, len(signs), replace=False)).tolist()
    if repeat and len(rows) > 1:
        rows[-1] = rows[0]
    return [(int(r), float(s)) for r, s in zip(rows, signs)]


def mixed_batch(seed, n, b, patterns=("+", "+-", "+-+", "-+++-", "8"), lo=0):
    """b expressions cycling through `patterns`, every fourth with a repeated row."""
    rng = np.random.default_rng(seed)
    return [expression(rng, n, PATTERNS[patterns[q % len(patterns)]], repeat=q % 4 == 3, lo=lo) for q in range(b)]


def unit_rows(seed, n, d):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def exact_distances(X, Q):
    """[len(Q)][len(X)]: acc = 0; acc += (q[e] - x[e]) * (q[e] - x[e]), e ascending, unfused -- knn_kernel's order."""
    X, Q = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(Q, np.float32)
    acc = np.zeros((len(Q), len(X)), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(X.shape[1]):
            dx = (Q[:, e, None] - X[None, :, e]).astype(np.float32)
            acc = (acc + (dx * dx).astype(np.float32)).astype(np.float32)
    return acc


def adc_distances(tables, codes):
    """[T][n]: tables [T][m][k] (Index.prepareQuery of every term vector), codes [n][m]; acc = 0; acc += T[j][code_j],
    j ascending -- the order of scan.hip's exact scan."""
    tables = np.ascontiguousarray(tables, np.float32)
    T, m, _ = tables.shape
    acc = np.zeros((T, len(codes)), np.float32)
    for j in range(m):
        acc = (acc + tables[:, j, :][:, codes[:, j]]).astype(np.float32)
    return acc


def reference_lists(distances, exprs, row_ids, k):
    """distances: per expression [E][n] over the rows `row_ids` (ascending ids) -> (rows [b][k] padded with -1, scores
    [b][k] padded with -inf, counts [b]): the rows that are no term rows by (score descending, row id ascending)."""
    from gulon_amd.expressions import cosmul_reference
    b = len(exprs)
    ri, rs, rc = np.full((b, k), -1, np.int32), np.full((b, k), -np.inf, np.float32), np.zeros(b, np.int32)
    row_ids = np.asarray(row_ids, np.int64)
    for q, (D, e) in enumerate(zip(distances, exprs)):
        score = cosmul_reference(D, [w for _, w in e])
        keep = ~np.isin(row_ids, [r for r, _ in e])
        order = np.lexsort((row_ids[keep], -score[keep]))[:k]
        rc[q] = len(order)
        ri[q, :rc[q]], rs[q, :rc[q]] = row_ids[keep][order], score[keep][order]
    return ri, rs, rc


def per_expression(term_distances, exprs):
    """term_distances [T][n] in the order of the batch's terms -> the list of [E][n] blocks."""
    out, t = [], 0
    for e in exprs:
        out.append(term_distances[t:t + len(e)])
        t += len(e)
    return out


def same(got, want):
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1]))


def zero_factors(D):
    """[E][n] bool: where a term's factor s_t is 0 (a distance of 4 or more, or a NaN).  A one-term expression scores
    s_t / 1.001, so cosmul_reference itself says it."""
    from gulon_amd.expressions import cosmul_reference
    return np.stack([cosmul_reference(D[t:t + 1], [1.0]) == 0 for t in range(len(D))])


def equal_neighbours(lists):
    """Per answer list of (rows, scores, counts): the (row, next row) pairs of adjacent entries with equal scores."""
    ri, rs, rc = lists
    return [[(int(ri[q, e]), int(ri[q, e + 1])) for e in range(rc[q] - 1) if rs[q, e] == rs[q, e + 1]]
            for q in range(len(rc))]


def native_index(g, pq, idx, row_base=0):
    """The flat index gulon_index_create makes of the planted codes idx [m][n]: no training."""
    coder = pq.coder_factory(idx.shape[1])
    return g.PQIndex(pq, g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(idx.shape[0])]), row_base)


def flat_term_distances(oracle, vi, codes, cents, exprs, normalize):
    """[T][n] over the PQIndex `vi` with codes [n][m]: every term's vector by the handle's own compose_rows, the oracle's
    Index.prepareQuery tables of it, adc_distances."""
    d, m = vi.dimension, codes.shape[1]
    Q = vi.compose_rows([[(r, 1.0)] for e in exprs for r, _ in e], normalize, normalize)
    return adc_distances(oracle.prepare_query(cents, d, m, vi.product_quantizer.num_clusters, Q), codes)


def run_dev(g, call, exprs, k, with_err):
    """A *_query_cosmul_dev call on device copies of the term lists: call(off, rows, w, b, oi, os, oc, err) with device
    addresses (err: a zeroed word, None unless with_err) -> (rows [b][k], scores [b][k], counts [b]), *err or None."""
    from gulon_amd.expressions import to_csr
    from gulon_amd.refine import _DeviceArray
    off, rows, w = to_csr(exprs)
    b = len(exprs)
    dev = {name: _DeviceArray() for name in ("off", "rows", "w", "oi", "os", "oc", "err")}
    try:
        dev["off"].upload(off), dev["rows"].upload(rows), dev["w"].upload(w)
        dev["err"].upload(np.zeros(1, np.int32))
        for name, nbytes in (("oi", b * k * 4), ("os", b * k * 4), ("oc", b * 4)):
            dev[name].ensure(nbytes)
        g.native.check(call(dev["off"].ptr, dev["rows"].ptr, dev["w"].ptr, b, dev["oi"].ptr, dev["os"].ptr,
                            dev["oc"].ptr, dev["err"].ptr if with_err else None))
        g.native.check(g.native.lib().gulon_device_synchronize())
        oi = dev["oi"].download(np.zeros((b, k), np.int32))
        os_ = dev["os"].download(np.zeros((b, k), np.float32))
        oc = dev["oc"].download(np.zeros(b, np.int32))
        err = int(dev["err"].download(np.zeros(1, np.int32))[0]) if with_err else None
    finally:
        for a in dev.values():
            a.free()
    return (oi, os_, oc), err
