"""Word-pair similarity benchmark (csrc/pairs.hip): the calls of DESIGN.md §9w's timing table at its shapes --
   gulon_index_pair_distances_dev       3 000 and 100 000 random pairs over a flat index, 1 M x 300, PQ(m = 30, k = 256),
                                        random codes
   gulon_dataset_pair_distances_dev     the same pairs over a dataset, 1 M x 300, synthetic vectors
   gulon_rank_sums_dev                  n = 3 000 and 100 000 (scores with ties, ten interleaved sections), then the stream
                                        is synchronised
   python tests/perf/bench_similarity.py [rows]
§9j's method: HIP events on the null stream around the whole call (the allocation of the error word and the
synchronisation inside the pair distances included), one warm-up call, then REPEATS calls: the minimum is the table's
figure, the median and the maximum are printed beside it.  Timed, not gated.  Prints one JSON line."""
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
d, m, k = 300, 30, 256
PAIRS = (3_000, 100_000)
REPEATS = 7
L = N.lib()
rng = np.random.default_rng(1)
pq = g.ProductQuantizer.from_flat(k, d, m, rng.standard_normal(k * d).astype(np.float32))
coder = pq.coder_factory(n)
index = g.PQIndex(pq, g.EncodedMatrix(coder, [rng.integers(0, k, n, dtype=np.uint8) for _ in range(m)]))
dm = g.DeviceMatrix.synthetic(n, d, 3, 1234, 1000)


def timed(call):
    times = []
    for _ in range(1 + REPEATS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    times = times[1:]
    return {"min_ms": min(times), "median_ms": statistics.median(times), "max_ms": max(times)}


times = {}
for pairs in PAIRS:
    a = torch.from_numpy(rng.integers(0, n, pairs).astype(np.int32)).cuda()
    b = torch.from_numpy(rng.integers(0, n, pairs).astype(np.int32)).cuda()
    dist = torch.empty(pairs, dtype=torch.float32, device="cuda")
    score = torch.from_numpy(rng.integers(0, 41, pairs).astype(np.float32) / 4).cuda()
    section = torch.from_numpy(rng.integers(0, 10, pairs).astype(np.int32)).cuda()
    sums = torch.empty((10, 5), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    times[f"index_pair_distances_dev_{pairs}"] = timed(lambda: N.check(L.gulon_index_pair_distances_dev(
        index._h, a.data_ptr(), b.data_ptr(), pairs, dist.data_ptr(), None)))
    flat = dist.cpu().numpy()
    times[f"dataset_pair_distances_dev_{pairs}"] = timed(lambda: N.check(L.gulon_dataset_pair_distances_dev(
        dm._h, a.data_ptr(), b.data_ptr(), pairs, dist.data_ptr(), None)))
    assert np.isfinite(flat).all() and np.isfinite(dist.cpu().numpy()).all()

    def rank_sums():
        N.check(L.gulon_rank_sums_dev(dist.data_ptr(), score.data_ptr(), section.data_ptr(), pairs, 10, sums.data_ptr(),
                                      None))
        N.check(L.gulon_device_synchronize())
    times[f"rank_sums_dev_{pairs}"] = timed(rank_sums)
    assert int(sums.cpu().numpy()[:, 0].sum()) == pairs

print(json.dumps({"metric": "index_pair_distances_call_ms", "value": times["index_pair_distances_dev_3000"]["min_ms"],
                  "unit": "ms",
                  "config": {"workload": f"PQIndex {n}x{d}, PQ(m={m},k={k}), random codes; dataset {n}x{d}, synthetic vectors",
                             "warmup": 1, "repeats": REPEATS, "timer": "HIP events on the null stream"},
                  "times": times}), flush=True)
