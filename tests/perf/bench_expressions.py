"""Expression-query benchmark (1 M x 128, m = 16, k = 256, 1024 three-term expressions, k_nn = 10): the device route
(csrc/compose.hip: compose, query at k + 3, drop, one call) against the host route on the same build -- lookup_rows to
the host, numpy composition, batch_query at k + 3, the operands dropped on the host -- and a plain batch_query_rows at
k + 3 as the floor.  Checks that both routes give identical results.  Timed, not gated.
   python tests/perf/bench_expressions.py [rows] [dim] [k_nn]
Every time is the median of BLOCKS blocks of STEPS back-to-back steps, after warm-up, the device idle before a block."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import gulon_amd as g
from gulon_amd import native as N
from gulon_amd.expressions import compose_reference

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 128
K = int(sys.argv[3]) if len(sys.argv) > 3 else 10
m, k, B, iters, E = 16, 256, 1024, 10, 3
WARMUP, BLOCKS, STEPS = 3, 7, 10
dm = g.DeviceMatrix.synthetic(n, d, 3, 1234, 1000)
pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(k, m, iters))
index = g.Index.sorted(dm, pq)
vi = index.vector_index
rng = np.random.default_rng(0)
rows = np.stack([rng.choice(n, E, replace=False) for _ in range(B)]).astype(np.int32)      # king - man + woman
weights = np.asarray([1.0, -1.0, 1.0], np.float32)
exprs = [[(int(r), float(w)) for r, w in zip(rows[q], weights)] for q in range(B)]


def device_route():
    return vi.batch_query_terms_raw(K, exprs, E)


def host_route():
    vectors = vi.decode_rows(rows.reshape(-1)).reshape(B, E, d)
    acc = (weights[0] * vectors[:, 0]).astype(np.float32)                # the arithmetic of compose_reference, batched
    for t in range(1, E):
        acc = (acc + (weights[t] * vectors[:, t]).astype(np.float32)).astype(np.float32)
    oi, od, oc, of = vi.batch_query_raw(K + E, acc)
    ri, rd = np.full((B, K), -1, np.int32), np.full((B, K), np.inf, np.float32)
    rc = np.zeros(B, np.int32)
    for q in range(B):
        keep = [p for p in range(oc[q]) if oi[q, p] not in rows[q]][:K]
        ri[q, :len(keep)], rd[q, :len(keep)], rc[q] = oi[q, keep], od[q, keep], len(keep)
    return ri, rd, rc, of


def floor():
    return vi.batch_query_rows_raw(K + E, rows[:, 0])


def timed(step):
    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    blocks = []
    for _ in range(BLOCKS):
        t = time.perf_counter()
        for _ in range(STEPS):
            step()
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t) / STEPS * 1e3)
    return {"median_ms": statistics.median(blocks), "min_ms": min(blocks), "max_ms": max(blocks)}


a, b = device_route(), host_route()
identical = all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                               y.view(np.uint32) if y.dtype == np.float32 else y) for x, y in zip(a, b))
assert np.array_equal(vi.compose_rows(exprs[:4]).view(np.uint32),
                      np.stack([compose_reference(vi.decode_rows(rows[q]), weights) for q in range(4)]).view(np.uint32))
times = {"device_route": timed(device_route), "host_route": timed(host_route), "floor_query_rows": timed(floor)}
print(json.dumps({"metric": "expression_query_ms", "value": times["device_route"]["median_ms"], "unit": "ms",
                  "config": {"workload": f"SortedIndex {n}x{d}, PQ(m={m},k={k}), {B} expressions of {E} terms, K={K}",
                             "warmup": WARMUP, "blocks": BLOCKS, "steps_per_block": STEPS},
                  "times": times, "routes_identical": bool(identical)}), flush=True)
assert identical, "the device route and the host route differ"
