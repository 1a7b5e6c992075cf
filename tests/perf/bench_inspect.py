"""Index-diagnostics benchmark (csrc/inspect.hip, csrc/decode.hip): the calls of DESIGN.md §9j's timing table at its shape
-- 1 M x 128, PQ(m = 16, k = 256), random codes, synthetic vectors:
   gulon_index_code_histogram                         the whole index
   gulon_index_row_errors_dev, identity / shuffled    row errors, norms and quantizer errors against the vectors
   gulon_index_decode_dataset                         the decoded matrix to HBM (the two-step route's first step)
   python tests/perf/bench_inspect.py [rows]
§9j's method: HIP events on the null stream around the whole call (allocations, the histogram's download and the
synchronisations inside it included), one warm-up call, then REPEATS calls: the minimum is the table's figure, the
median and the maximum are printed beside it.  Timed, not gated.  Prints one JSON line."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import gulon_amd as g
from gulon_amd import native as N

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d, m, k = 128, 16, 256
REPEATS = 7
L = N.lib()
rng = np.random.default_rng(1)
pq = g.ProductQuantizer.from_flat(k, d, m, rng.standard_normal(k * d).astype(np.float32))
coder = pq.coder_factory(n)
index = g.PQIndex(pq, g.EncodedMatrix(coder, [rng.integers(0, k, n, dtype=np.uint8) for _ in range(m)]))
dm = g.DeviceMatrix.synthetic(n, d, 3, 1234, 1000)
shuffled = torch.from_numpy(rng.permutation(n).astype(np.int32)).cuda()
err = torch.empty(n, dtype=torch.float32, device="cuda")
nrm = torch.empty(n, dtype=torch.float32, device="cuda")
qerr = np.zeros(m, np.float64)
hist = np.zeros(m * k, np.int64)


def timed(call, after=lambda: None):
    """`after` runs outside the timed span (it frees what the call allocated)"""
    times = []
    for _ in range(1 + REPEATS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
        after()
    times = times[1:]
    return {"min_ms": min(times), "median_ms": statistics.median(times), "max_ms": max(times)}


def row_errors(row_map):
    N.check(L.gulon_index_row_errors_dev(index._h, dm._h, row_map, n if row_map else 0, 0, n, err.data_ptr(),
                                         nrm.data_ptr(), qerr, None))


decoded = C.c_void_p()


def decode():
    N.check(L.gulon_index_decode_dataset(index._h, 0, n, C.byref(decoded)))


times = {
    "code_histogram": timed(lambda: N.check(L.gulon_index_code_histogram(index._h, 0, n, hist))),
    "row_errors_dev_identity": timed(lambda: row_errors(None)),
    "row_errors_dev_shuffled": timed(lambda: row_errors(shuffled.data_ptr())),
    "decode_dataset": timed(decode, lambda: N.check(L.gulon_dataset_destroy(decoded))),
}
assert int(hist.sum()) == n * m and float(qerr.sum()) > 0

print(json.dumps({"metric": "row_errors_call_ms", "value": times["row_errors_dev_identity"]["min_ms"], "unit": "ms",
                  "config": {"workload": f"PQIndex {n}x{d}, PQ(m={m},k={k}), random codes, synthetic vectors",
                             "warmup": 1, "repeats": REPEATS, "timer": "HIP events on the null stream"},
                  "times": times}), flush=True)
