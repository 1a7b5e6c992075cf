"""Index-view benchmark at the headline shape (10 M x 128, m = 16, k = 256): what building a view on the device
(csrc/subset.hip) costs next to the host route it replaces, and that a batch on the view runs as fast as on an index
created natively from the same rows -- their code buffers are byte-identical.  Timed, not gated.
   python tests/perf/bench_subset.py [rows] [dim]
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
from gulon_amd.index import pack_mask
from gulon_amd.recall import sample_rows

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 128
m, k, B, K, iters = 16, 256, 1024, 10, 10
WARMUP, BLOCKS, STEPS = 3, 7, 10
dm = g.DeviceMatrix.synthetic(n, d, 3, 1234, 1000)
pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(k, m, iters))
parent = g.Index.sorted(dm, pq).vector_index
Q = dm.get_rows(sample_rows(n, B, 0))
# the same row count under a one-byte code: select on it is mask -> rows plus a 4-byte gather per row
thin_pq = g.ProductQuantizer.from_flat(1, 1, 1, np.zeros(1, np.float32))
thin = g.PQIndex(thin_pq, g.EncodedMatrix(thin_pq.coder_factory(n), [np.zeros(0, np.uint8)]))


def timed(step, sync=torch.cuda.synchronize):
    for _ in range(WARMUP):
        step()
    sync()
    blocks = []
    for _ in range(BLOCKS):
        t = time.perf_counter()
        for _ in range(STEPS):
            step()
        sync()
        blocks.append((time.perf_counter() - t) / STEPS * 1e3)
    return {"median_ms": statistics.median(blocks), "min_ms": min(blocks), "max_ms": max(blocks)}


out = {"rows": n, "dim": d, "m": m, "k": k}
for density in (0.5, 0.01):
    keep = np.random.default_rng(int(density * 100)).random(n) < density
    rows = np.flatnonzero(keep)
    mask = torch.from_numpy(pack_mask(keep, n).view(np.int64)).cuda()
    rec = {"selected": int(len(rows))}

    def select(index=parent):
        index.select(mask=mask).close()

    # 1. select alone: mask -> rows (+ a 4-byte gather), + the gather of the codes, + the conflict ordering of the copy
    g.tune_live(GULON_FILTER_ORDER=0)
    rec["select_mask_to_rows_thin_code"] = timed(lambda: select(thin))
    rec["select_without_ordering"] = timed(select)
    g.tune_live(GULON_FILTER_ORDER=1)
    rec["select_with_ordering"] = timed(select)

    # 2. the host route on the same build: codes on the host, numpy gather, gulon_index_create
    def host_route():
        idx = parent.data.indices()
        coder = pq.coder_factory(len(rows))
        return g.PQIndex(pq, g.EncodedMatrix(coder, [coder.build_code(idx[j, rows]) for j in range(m)]))

    rec["host_route"] = timed(lambda: host_route().close())

    # 3. one batch on the view and on the native index over the same rows
    view, native = parent.select(mask=mask), host_route()
    rec["batch_on_view"] = timed(lambda: view.batch_query_raw(K, Q))
    rec["batch_on_native"] = timed(lambda: native.batch_query_raw(K, Q))
    a, b = view.positions_raw(K, Q), native.batch_query_raw(K, Q)
    rec["view_equals_native"] = bool(all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b)))
    view.close(), native.close()
    out[f"density_{density}"] = rec
print(json.dumps(out))
