"""What the grouped offset-query tests share: the build of a small grouped index by test_gpu_grouped.py's
recipe, and the reference -- the handle's own ordinary query deep enough to return every searched row, scattered by row
id into [b][n] filled with +inf (so the rows of unsearched groups drop out on their own), fed to
csls.offset_query_reference."""
import numpy as np
import pytest


def scale_of(d):
    """Rows of variance 3 / d per component: two rows of one cluster lie about 6 apart and a row about 1 from its own
    code, so offsets between -1.5 and 1.5 change the order and a few keys, not all, turn negative."""
    return np.float32(np.sqrt(3.0 / d))


def build(g, n, d, groups, m, k, seed, twins=0, iters=3, metric="l2", row0_outside=False):
    """Coarse k-means, group, ProductQuantizer.apply on the residuals.  twins: the last `twins` rows repeat the first
    ones.  row0_outside: rows are swapped so that row 0 is not in the lowest-numbered non-empty cluster, which gives the
    reference's leading empty group.  -> dict with the vectors in grouped order (Xg), the grouped vectors, the quantizer
    and the grouped row positions of the twins [(a, b), ...]."""
    rng = np.random.default_rng(seed)
    X = ((rng.standard_normal((n, d)) + 3.0 * rng.integers(0, 4, (n, 1))) * scale_of(d)).astype(np.float32)
    if twins:
        X[-twins:] = X[:twins]
    dm = g.DeviceMatrix.from_host(X)
    coarse = g.KMeans.compute_clusters(g.Vectors(dm), g.KMeansConfig(groups, iters))
    gv = g.group(dm, coarse)
    if row0_outside and gv.offsets[0] != 0:
        assign = np.empty(n, np.int64)
        assign[gv.perm] = np.searchsorted(gv.offsets, np.arange(n), side="right")
        other = int(np.argmax(assign != assign[0]))           # a row of a later group than row 0's ...
        X[[0, other]] = X[[other, 0]]                         # ... becomes row 0
        dm.close()
        dm = g.DeviceMatrix.from_host(X)
        gv = g.group(dm, coarse)
    pq = g.ProductQuantizer.apply(gv.residuals, g.ProductQuantizerConfig(k, m, iters))
    pos = np.empty(n, np.int64)
    pos[gv.perm] = np.arange(n)
    return {"X": X, "Xg": X[gv.perm], "gv": gv, "pq": pq, "n": n, "d": d, "metric": metric, "dm": dm,
            "twins": [(int(pos[i]), int(pos[n - twins + i])) for i in range(twins)]}


def group_of_rows(gv, n):
    """The group whose row range holds every grouped row position (GroupedVectors.cluster_of)."""
    return np.searchsorted(gv.offsets, np.arange(n), side="right")


def scattered_distances(index, Q, depth=None, oracle=None):
    """The handle's ordinary query at K = n, which the literal kernels answer with every searched row, scattered by row id
    into [b][n] filled with +inf.  depth: for an index whose tables leave LDS for `depth` heap entries only (the handle
    refuses K = n): the CPU oracle's GroupedIndex.query at K = n takes the handle's place, after the handle's answer at
    K = depth has been found equal to the oracle's at that depth, bit for bit."""
    n = index.size
    if depth is None:
        oi, od, oc = index.batch_query_raw(n, Q)
    else:
        with pytest.raises(NotImplementedError, match="LDS"):
            index.batch_query_raw(n, Q)
        s, limit = index._strategy()
        args = (index.data.indices(), index.dimension, index.quantizer.num_clusters, index.quantizer.flat_centroids(),
                index.centroids, index.offsets, Q)
        hi, hd, hc = index.batch_query_raw(depth, Q)
        ei, ed, ec = oracle.grouped_query(*args, depth, s, limit)
        assert np.array_equal(hc, ec)
        for q in range(len(Q)):
            assert np.array_equal(hi[q, :hc[q]], ei[q, :ec[q]])
            assert np.array_equal(hd[q, :hc[q]].view(np.uint32), ed[q, :ec[q]].view(np.uint32))
        oi, od, oc = oracle.grouped_query(*args, n, s, limit)
    out = np.full((len(oi), n), np.inf, np.float32)
    for q in range(len(oi)):
        out[q, oi[q, :oc[q]]] = od[q, :oc[q]]
    return out


def reference(g, dist, offsets, k, exclude=None):
    return g.offset_query_reference(dist, offsets, k, exclude, rows=np.arange(dist.shape[1]))


def queries_from(seed, Xg, b, first=()):
    """b noisy copies of rows of Xg -- `first` names the rows the first queries are made from, the others are drawn --
    and the row every other query excludes (the one it was made from), else -1."""
    rng = np.random.default_rng(seed)
    made_from = rng.integers(0, len(Xg), b)
    made_from[:min(b, len(first))] = list(first)[:b]
    noise = rng.standard_normal((b, Xg.shape[1])).astype(np.float32) * np.float32(0.05) * scale_of(Xg.shape[1])
    return (Xg[made_from] + noise).astype(np.float32), np.where(np.arange(b) % 2 == 1, made_from, -1).astype(np.int32)
