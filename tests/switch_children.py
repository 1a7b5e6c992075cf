"""What the child processes of test_gpu_switches_off.py run: the process-wide switches of the library are read once per
process, so each gets a fresh interpreter with the switch in its environment.  A child loads its inputs from an .npz
the parent wrote, asks the GPU, and writes the raw answers to another .npz; the parent compares them with the oracle.
The builders of the inputs are here as well, so that parent and child agree on them.  Nothing here imports the library at
module level: the parent only uses the builders."""
import sys
import threading

import numpy as np


# ---- inputs (parent side) --------------------------------------------------------------------------------------------

def random_index(n, d, m, k, seed, dup=0):
    """test_gpu_query._make's data: (cents, idx [m][n])."""
    rng = np.random.default_rng(seed)
    cents = rng.standard_normal(k * d).astype(np.float32)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    if dup:
        idx[:, -dup:] = idx[:, :dup]
    return cents, idx


def decode(cents, k, code, bounds):
    """ProductQuantizer.decode of one code row; bounds = the sub-vectors' (from, until) (oracle.subvectors)."""
    fr, un = bounds
    out = np.zeros(int(un[-1]), np.float32)
    for j in range(len(fr)):
        s = un[j] - fr[j]
        out[fr[j]:un[j]] = cents[k * fr[j] + code[j] * s: k * fr[j] + (code[j] + 1) * s]
    return out


def many_flagged_index(n, d, m, k, K, B, nbase, bounds):
    """test_exact_heap_replay_many_flagged_long_range's data: half of the rows are copies of a few hundred code rows, a few
    rows have one far copy each; the queries are decoded copies.  -> (cents, idx, Q)."""
    rng = np.random.default_rng(n + K)
    cents = rng.standard_normal(k * d).astype(np.float32)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    base = rng.integers(0, k, (m, nbase)).astype(np.int32)
    copies = rng.permutation(n)[:n // 2]
    idx[:, copies] = base[:, rng.integers(0, nbase, n // 2)]
    lone = np.setdiff1d(np.arange(2000, 4000), copies)[:8]
    far = np.setdiff1d(np.arange(n - 3000, n - 1000), copies)[:8]
    idx[:, far] = idx[:, lone]
    Q = np.stack([decode(cents, k, idx[:, int(r)], bounds) for r in list(copies[:B - 8]) + list(lone)]).astype(np.float32)
    return cents, idx, Q


def grouped_data(n, d, seed, dup):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, d)) + 3.0 * rng.integers(0, 4, (n, 1))).astype(np.float32)
    if dup:
        X[-dup:] = X[:dup]
    return X


# ---- the GPU side (child) --------------------------------------------------------------------------------------------

def _index(g, cents, idx, d, k):
    m, n = idx.shape
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    coder = pq.coder_factory(n)
    enc = g.EncodedMatrix(coder, [coder.build_code(np.ascontiguousarray(idx[j])) for j in range(m)])
    return g.PQIndex(pq, enc)


def _set(ix, **knobs):
    from gulon_amd import native as N
    for key, v in knobs.items():
        N.check(N.lib().gulon_index_tuning(ix._h, key.encode(), int(v)))


def _filter_tiles(ix):
    import ctypes as C
    from gulon_amd import native as N
    t, r = C.c_int32(-1), C.c_int32(-1)
    N.check(N.lib().gulon_index_filter_stats(ix._h, C.byref(t), C.byref(r)))
    return t.value


def _put(out, label, raw):
    for name, a in zip(("i", "d", "c", "f"), raw):
        out[label + "/" + name] = np.array(a)


def _partial(ix, Q, K, frm, until):
    import ctypes as C
    from gulon_amd import native as N
    L, B = N.lib(), len(Q)
    dq, dv, di = C.c_void_p(), C.c_void_p(), C.c_void_p()
    N.check(L.gulon_dev_malloc(C.byref(dq), Q.nbytes))
    N.check(L.gulon_dev_malloc(C.byref(dv), B * (K + 1) * 4))
    N.check(L.gulon_dev_malloc(C.byref(di), B * (K + 1) * 4))
    N.check(L.gulon_memcpy_h2d(dq, Q.ctypes.data_as(C.c_void_p), Q.nbytes))
    N.check(L.gulon_index_scan_partial_dev(ix._h, dq, B, K, frm, until, dv, di, None))
    N.check(L.gulon_device_synchronize())
    v, i = np.zeros((B, K + 1), np.float32), np.zeros((B, K + 1), np.int32)
    N.check(L.gulon_memcpy_d2h(v.ctypes.data_as(C.c_void_p), dv, v.nbytes))
    N.check(L.gulon_memcpy_d2h(i.ctypes.data_as(C.c_void_p), di, i.nbytes))
    for p in (dq, dv, di):
        N.check(L.gulon_dev_free(p))
    return v, i


def order_window_ranges(n):
    """(label, from, until): the whole index, cuts through the first and the last block, a range inside one block."""
    return [("whole", 0, n), ("cut", 777, n - 333), ("cut blocks", 37, n - 29), ("one block", 130, 180)]


ORDER_WINDOW_SPLIT = 35000


def order_window_answers(ix, Q, n, out, prefix):
    """Everything the GULON_FILTER_ORDER_WINDOW=0 child asks of one handle, under `prefix`."""
    _set(ix, GULON_SCAN_FILTER=1)
    for label, frm, until in order_window_ranges(n)[:2]:                      # (a) filtered
        _put(out, f"{prefix}/filtered/{label}", ix.batch_query_raw(10, Q, frm, until))
        out[f"{prefix}/filtered/{label}/tiles"] = np.array(_filter_tiles(ix))
    _set(ix, GULON_SCAN_FILTER=0)
    for blocks in (1, 4096):                                                  # (b) the exact scan
        _set(ix, GULON_SCAN_BLOCKS=blocks)
        for K in (1, 10, 63):
            for label, frm, until in order_window_ranges(n):
                _put(out, f"{prefix}/exact/{blocks}/{K}/{label}", ix.batch_query_raw(K, Q, frm, until))
    for K in (100, 200):                                                      # (c) peeled rounds
        for label, frm, until in order_window_ranges(n)[:2]:
            _put(out, f"{prefix}/peeled/{K}/{label}", ix.batch_query_raw(K, Q, frm, until))
    for label, frm, until in (("low", 0, ORDER_WINDOW_SPLIT), ("high", ORDER_WINDOW_SPLIT, n)):   # (d) partial lists
        v, i = _partial(ix, Q, 10, frm, until)
        out[f"{prefix}/partial/{label}/v"], out[f"{prefix}/partial/{label}/i"] = v, i
    out[f"{prefix}/exact_tiles"] = np.array(_filter_tiles(ix))


def child_order_window(inp, out):
    import gulon_amd as g
    for name in ("plainidx", "dupidx", "control"):
        cents, idx, Q = inp[name + "_cents"], inp[name + "_idx"], inp[name + "_Q"]
        d, k = int(inp[name + "_dk"][0]), int(inp[name + "_dk"][1])
        ix = _index(g, cents, idx, d, k)
        order_window_answers(ix, Q, idx.shape[1], out, name + "/ordered")
        _set(ix, GULON_FILTER_ORDER=0)                                        # (e) back on the plain copy
        order_window_answers(ix, Q, idx.shape[1], out, name + "/plain")
        ix.close()


def child_flat_queries(inp, out):
    """Cases `c<i>`: cents, idx, Q, params = (d, k, K, from, until, repeats): batch_query_raw of each, `repeats` times."""
    import gulon_amd as g
    for c in range(int(inp["cases"])):
        d, k, K, frm, until, reps = (int(v) for v in inp[f"c{c}_params"])
        ix = _index(g, inp[f"c{c}_cents"], inp[f"c{c}_idx"], d, k)
        for r in range(reps):
            _put(out, f"c{c}/r{r}", ix.batch_query_raw(K, inp[f"c{c}_Q"], frm, until))
        ix.close()


def _grouped(g, X, groups, m, k, iters, limit, Q, K, out, label):
    dm = g.DeviceMatrix.from_host(X)
    coarse = g.KMeans.compute_clusters(g.Vectors(dm), g.KMeansConfig(groups, iters))
    gv = g.group(dm, coarse)
    pq = g.ProductQuantizer.apply(gv.residuals, g.ProductQuantizerConfig(k, m, iters))
    index = g.Index.grouped(gv, pq, g.LimitGroups(limit))
    oi, od, oc = index.batch_query_raw(K, Q)
    out[label + "/i"], out[label + "/d"], out[label + "/c"] = np.array(oi), np.array(od), np.array(oc)
    out[label + "/codes"] = np.array(index.data.indices())
    out[label + "/pq"] = np.array(pq.flat_centroids())
    out[label + "/gcents"] = np.array(gv.centroids)
    out[label + "/offsets"] = np.array(gv.offsets)
    index.close()


def child_grouped(inp, out):
    import gulon_amd as g
    for c in range(int(inp["cases"])):
        groups, m, k, iters, limit, K = (int(v) for v in inp[f"c{c}_params"])
        _grouped(g, inp[f"c{c}_X"], groups, m, k, iters, limit, inp[f"c{c}_Q"], K, out, f"c{c}")


def _train(g, X, m, k, iters, out, label):
    dm = g.DeviceMatrix.from_host(X)
    pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(k, m, iters))
    out[label + "/cents"] = np.array(pq.flat_centroids())
    out[label + "/codes"] = np.array(pq.encode(dm).indices())


def child_kmeans(inp, out):
    import gulon_amd as g
    for c in range(int(inp["cases"])):
        m, k, iters = (int(v) for v in inp[f"c{c}_params"])
        _train(g, inp[f"c{c}_X"], m, k, iters, out, f"c{c}")


def child_host_contexts(inp, out):
    """Eight threads, host-pointer queries on one handle, three rounds each (test_concurrent_host_queries_from_threads)."""
    import gulon_amd as g
    d, k, K = (int(v) for v in inp["params"])
    ix = _index(g, inp["cents"], inp["idx"], d, k)
    Qs = [inp[f"Q{t}"] for t in range(8)]
    res, err = [None] * 8, []

    def run(t):
        try:
            for _ in range(3):
                res[t] = ix.batch_query_raw(K, Qs[t])
        except Exception as e:      # pragma: no cover
            err.append(repr(e))

    ts = [threading.Thread(target=run, args=(t,)) for t in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not err, err
    for t in range(8):
        _put(out, f"t{t}", res[t])
    ix.close()


def child_stats(inp, out):
    """One filtered query, one tie query, one grouped query and one small k-means with every statistics switch set."""
    import gulon_amd as g
    for name in ("filtered", "ties"):
        d, k, K = (int(v) for v in inp[name + "_params"])
        ix = _index(g, inp[name + "_cents"], inp[name + "_idx"], d, k)
        _put(out, name, ix.batch_query_raw(K, inp[name + "_Q"]))
        out[name + "/tiles"] = np.array(_filter_tiles(ix))
        ix.close()
    groups, m, k, iters, limit, K = (int(v) for v in inp["grouped_params"])
    _grouped(g, inp["grouped_X"], groups, m, k, iters, limit, inp["grouped_Q"], K, out, "grouped")
    m, k, iters = (int(v) for v in inp["kmeans_params"])
    _train(g, inp["kmeans_X"], m, k, iters, out, "kmeans")


CHILDREN = {"order_window": child_order_window, "flat": child_flat_queries, "grouped": child_grouped,
            "kmeans": child_kmeans, "host_contexts": child_host_contexts, "stats": child_stats}


def main(argv):
    what, src, dst = argv
    out = {}
    with np.load(src) as inp:
        CHILDREN[what](inp, out)
    np.savez(dst, **out)


if __name__ == "__main__":
    main(sys.argv[1:])
