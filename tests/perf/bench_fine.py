"""Fine-code benchmark (csrc/fine.hip): what re-ranking an index's candidates against the two-level codes costs per
1024-query batch, next to re-ranking them against the original vectors (csrc/refine.hip) at the same shapes -- d = 128,
coarse PQ(m = 16, k = 256), fine PQ(m = 32, k = 256), k_nn = 10, c = 100 and c = 1000.  Timed, not gated: the two
kernels read different things (c x 512 bytes of vectors against c x 48 bytes of codes and their code-book entries).
   python tests/perf/bench_fine.py [rows] [baseline_lib]
baseline_lib: another build of libgulon_hip.so (e.g. the parent commit's) whose gulon_refine_topk_dev is timed beside
this build's over the same device buffers.
Every time is the median of BLOCKS blocks of STEPS back-to-back steps, after warm-up, the device idle before a block."""
import ctypes as C
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
from gulon_amd.fine import index_row_residuals
from gulon_amd.recall import sample_rows

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
baseline = sys.argv[2] if len(sys.argv) > 2 else None
d, m, m2, k, B, K, iters = 128, 16, 32, 256, 1024, 10, 5
CANDIDATES = (100, 1000)
WARMUP, BLOCKS, STEPS = 3, 15, 10
L = N.lib()
dm = g.DeviceMatrix.synthetic(n, d, 3, 1234, 1000)
pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(k, m, iters))
index = g.Index.sorted(dm, pq)
rows = np.arange(n, dtype=np.int32)
E = index_row_residuals(index, dm, rows, rows)
fine = g.Index.sorted(E, g.ProductQuantizer.apply(E, g.ProductQuantizerConfig(k, m2, iters)))
E.close()
h, fh = index.vector_index._h, fine.vector_index._h
Q = torch.from_numpy(dm.get_rows(sample_rows(n, B, 0))).cuda()

base_fn = None
if baseline:
    base = C.CDLL(baseline)
    base_fn = base.gulon_refine_topk_dev
    base_fn.restype, base_fn.argtypes = N.SIGNATURES["gulon_refine_topk_dev"]


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


times = {}
for c in CANDIDATES:
    ci = torch.empty((B, c), dtype=torch.int32, device="cuda")
    cd = torch.empty((B, c), dtype=torch.float32, device="cuda")
    cc, cf = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    oi = torch.empty((B, K), dtype=torch.int32, device="cuda")
    od = torch.empty((B, K), dtype=torch.float32, device="cuda")
    oc = torch.empty(B, dtype=torch.int32, device="cuda")
    N.check(L.gulon_index_batch_query_dev(h, Q.data_ptr(), B, c, 0, n, ci.data_ptr(), cd.data_ptr(), cc.data_ptr(),
                                          cf.data_ptr(), None))      # the index's own candidates
    torch.cuda.synchronize()

    def codes():
        N.check(L.gulon_index_refine_codes_topk_dev(h, fh, Q.data_ptr(), B, ci.data_ptr(), c, None, 0, K, oi.data_ptr(),
                                                    od.data_ptr(), oc.data_ptr(), None))

    def vectors(fn=L.gulon_refine_topk_dev):
        N.check(fn(dm._h, Q.data_ptr(), B, ci.data_ptr(), c, None, 0, K, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), None))

    times[f"c{c}_refine_codes_topk_dev"] = timed(codes)
    assert int(oc.min()) >= 0
    times[f"c{c}_refine_topk_dev"] = timed(vectors)
    if base_fn is not None:
        times[f"c{c}_refine_topk_dev_baseline_lib"] = timed(lambda: vectors(base_fn))

print(json.dumps({"metric": "refine_codes_stage_ms", "value": times["c100_refine_codes_topk_dev"]["median_ms"],
                  "unit": "ms",
                  "config": {"workload": f"SortedIndex {n}x{d}, PQ(m={m},k={k}), fine PQ(m={m2},k={k}), batch={B}, K={K}, "
                                         f"candidates={list(CANDIDATES)}", "baseline_lib": bool(baseline),
                             "warmup": WARMUP, "blocks": BLOCKS, "steps_per_block": STEPS},
                  "times": times}), flush=True)
