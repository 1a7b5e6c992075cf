"""More than 63 neighbours from a wide-code index (wide.hip's peeling rounds): what a round costs.

Per 1024-query batch at 1 M x 128, m = 16, random codes and code books (the exact wide scan prunes nothing, so its
time does not hang on the data):
  (i)   k = 1024, K = 63, filter off: one exact wide scan, the unit;
  (ii)  k = 1024, K = 100 (2 rounds) and K = 1000 (16 rounds);
  (iii) k = 4096 (the table in two slices), K = 63 filter off (its own full scan) and K = 1000;
  (iv)  k = 256 (byte codes, scan.hip's peeling), K = 63 filter off and K = 1000: what peeling costs there.
Warm-up, then the median of `blocks` timed blocks of `steps` batches each.
    python tests/perf/bench_wide_large_k.py [rows] [blocks] [steps]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import gulon_amd as g
from gulon_amd import native as N

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 5
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
d, m, B = 128, 16, 1024
L = N.lib()


def make(k, seed):
    rng = np.random.default_rng(seed)
    cents = rng.standard_normal(k * d).astype(np.float32)
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    coder = pq.coder_factory(n)
    enc = g.EncodedMatrix(coder, [coder.build_code(rng.integers(0, k, n).astype(np.int32)) for _ in range(m)])
    return g.PQIndex(pq, enc)


Q = torch.from_numpy(np.random.default_rng(0).standard_normal((B, d)).astype(np.float32)).cuda()


def measure(index, K, filter_on):
    """(median ms per batch, min, max over the blocks)"""
    N.check(L.gulon_index_tuning(index._h, b"GULON_SCAN_FILTER", 1 if filter_on else 0))
    oi = torch.empty((B, K), dtype=torch.int32, device="cuda")
    od = torch.empty((B, K), dtype=torch.float32, device="cuda")
    oc = torch.empty(B, dtype=torch.int32, device="cuda")
    of = torch.empty(B, dtype=torch.int32, device="cuda")

    def step():
        N.check(L.gulon_index_batch_query_dev(index._h, Q.data_ptr(), B, K, 0, n, oi.data_ptr(), od.data_ptr(),
                                              oc.data_ptr(), of.data_ptr(), None))

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        t = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) / steps * 1e3)
    assert int(oc.min()) == min(K, n)
    return {"ms": float(np.median(ms)), "min": min(ms), "max": max(ms)}


def rounds(K):
    return -(-(K + 1) // 64)


out = {"rows": n, "d": d, "m": m, "batch": B, "blocks": blocks, "steps": steps}
ix = make(1024, 1)
out["k1024_K63_exact"] = unit = measure(ix, 63, False)
for K in (100, 1000):
    r = measure(ix, K, True)
    r["rounds"] = rounds(K)
    r["over_rounds_x_unit"] = r["ms"] / (rounds(K) * unit["ms"])
    out[f"k1024_K{K}"] = r
ix.close()
ix = make(4096, 2)
out["k4096_K63_exact"] = full = measure(ix, 63, False)
r = measure(ix, 1000, True)
r["rounds"] = rounds(1000)
r["over_rounds_x_full_scan"] = r["ms"] / (rounds(1000) * full["ms"])
out["k4096_K1000"] = r
ix.close()
ix = make(256, 3)
out["k256_K63_exact"] = byte_unit = measure(ix, 63, False)
r = measure(ix, 1000, True)
r["rounds"] = rounds(1000)
r["over_rounds_x_unit"] = r["ms"] / (rounds(1000) * byte_unit["ms"])
out["k256_K1000"] = r
ix.close()
print(json.dumps(out))
