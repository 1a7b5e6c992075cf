"""Decode and query-by-row measurements (decode.hip); prints one JSON line.

  decode   ProductQuantizer.decode(EncodedMatrix) of N x D rows, M quantizers of 256 centroids, into a new device dataset
           (gulon_index_decode_dataset): the call's wall time around a device synchronisation, which includes the
           allocation of the output.  The kernel's own time: run under `rocprofv3 --kernel-trace --stats` (kernel
           decode_range_kernel) with --only-decode.  Bytes moved = n*d*4 written + n*m code bytes read.
  query    1 024 rows queried by row on the device (batch_query_rows) against batch_query on the same rows decoded on
           the host (PQIndex.decode per row: its time reported on its own), for a sorted and a grouped index.

Every timing: warm-up, then the median of --blocks blocks."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29     # measured device-to-device copy rate of the MI355X (TB/s)


def median_ms(fn, blocks, reps):
    fn()
    times = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        times.append((time.perf_counter() - t0) * 1e3 / reps)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--b", type=int, default=1024)
    ap.add_argument("--k-nn", type=int, default=10)
    ap.add_argument("--groups", type=int, default=10_000)
    ap.add_argument("--limit", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--only-decode", action="store_true")
    a = ap.parse_args()

    import gulon_amd as g
    n, d, m, k, B, K = a.n, a.d, a.m, 256, a.b, a.k_nn
    rng = np.random.default_rng(1)
    cents = rng.standard_normal(k * d).astype(np.float32)
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    coder = pq.coder_factory(n)
    codes = [rng.integers(0, k, n, dtype=np.uint8) for _ in range(m)]      # width 8: the packed code is the byte
    assert coder.width == 8 and coder.bytes_per_code == n
    enc = g.EncodedMatrix(coder, codes)
    ix = g.PQIndex(pq, enc)
    out = {"shape": {"n": n, "d": d, "m": m, "k": k}}

    def decode_once():
        ix.decode_matrix().close()

    reps = 3 if n >= 1_000_000 else 20
    med, lo, hi = median_ms(decode_once, 1 if a.only_decode else a.blocks, 1 if a.only_decode else reps)
    nbytes = n * d * 4 + n * m
    out["decode_call_ms"] = {"median": med, "min": lo, "max": hi}
    out["decode_bytes"] = nbytes
    out["decode_call_tbs"] = nbytes / (med * 1e-3) / 1e12
    out["decode_floor_ms"] = nbytes / (COPY_TBS * 1e12) * 1e3
    if a.only_decode:
        print(json.dumps(out))
        return

    rows = rng.integers(0, n, B).astype(np.int32)

    def host_decode():         # ProductQuantizer.decode's numpy gather, for the requested rows only
        Q = np.zeros((B, d), np.float32)
        for j, q in enumerate(pq.quantizers):
            Q[:, q.frm:q.frm + q.dimension] = q.clusters.centroids[codes[j][rows]]
        return Q

    Q = host_decode()
    out["host_decode_ms"] = median_ms(host_decode, a.blocks, 5)[0]
    # the two paths must agree
    r1 = ix.batch_query_rows_raw(K, rows)
    r2 = ix.batch_query_raw(K, Q)
    assert all(np.array_equal(x, y) for x, y in zip(r1, r2)), "query by row differs from the host-decoded query"
    q_rows = median_ms(lambda: ix.batch_query_rows_raw(K, rows), a.blocks, 5)
    q_vecs = median_ms(lambda: ix.batch_query_raw(K, Q), a.blocks, 5)
    out["sorted"] = {"query_rows_ms": q_rows[0], "query_vectors_ms": q_vecs[0],
                     "decode_overhead_pct": 100 * (q_rows[0] - q_vecs[0]) / q_vecs[0]}
    ix.close()

    # grouped: the same codes as residuals, `groups` groups of equal size
    G = a.groups
    gc = rng.standard_normal((G, d)).astype(np.float32)
    offsets = (np.arange(1, G, dtype=np.int64) * n // G).astype(np.int32)
    gx = g.GroupedIndex(pq, enc, gc, offsets, g.LimitGroups(a.limit))
    look = gx.lookup_rows(rows)
    r1 = gx.batch_query_rows_raw(K, rows)
    r2 = gx.batch_query_raw(K, look)
    assert all(np.array_equal(x, y) for x, y in zip(r1, r2)), "grouped query by row differs"
    q_rows = median_ms(lambda: gx.batch_query_rows_raw(K, rows), a.blocks, 2)
    q_vecs = median_ms(lambda: gx.batch_query_raw(K, look), a.blocks, 2)
    out["grouped"] = {"groups": G, "limit_groups": a.limit, "query_rows_ms": q_rows[0], "query_vectors_ms": q_vecs[0],
                      "decode_overhead_pct": 100 * (q_rows[0] - q_vecs[0]) / q_vecs[0]}
    gx.close()
    out["b"], out["k_nn"] = B, K
    print(json.dumps(out))


if __name__ == "__main__":
    main()
