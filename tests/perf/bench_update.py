"""Index-update benchmark at the headline shape (10 M x 128, m = 16, k = 256), adding 100 000 rows: what encoding
against the index's own code books and merging the code buffers on the device (csrc/update.hip) cost next to the host
route they replace, and that a batch on the merged index runs as fast as on an index created natively from the same
codes -- their buffers are byte-identical.  Timed, not gated.
   python tests/perf/bench_update.py [rows] [dim] [added]
Every time is the median of BLOCKS blocks of back-to-back steps, after warm-up, the device idle before a block.  Every
timed section runs under an alarm: a step that hangs ends the script instead of holding the device."""
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import gulon_amd as g
from gulon_amd.recall import sample_rows

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 128
n_add = int(sys.argv[3]) if len(sys.argv) > 3 else 100_000
m, k, B, K, iters = 16, 256, 1024, 10, 10
WARMUP, BLOCKS = 3, 7
SECTION_LIMIT_S = 400                           # per timed section (SIGALRM ends the process)


def timed(step, steps=10, sync=torch.cuda.synchronize):
    signal.alarm(SECTION_LIMIT_S)
    for _ in range(WARMUP):
        step()
    sync()
    blocks = []
    for _ in range(BLOCKS):
        t = time.perf_counter()
        for _ in range(steps):
            step()
        sync()
        blocks.append((time.perf_counter() - t) / steps * 1e3)
    signal.alarm(0)
    return {"median_ms": statistics.median(blocks), "min_ms": min(blocks), "max_ms": max(blocks), "steps": steps}


t_setup = time.perf_counter()
signal.alarm(SECTION_LIMIT_S)
dm = g.DeviceMatrix.synthetic(n, d, 3, 1234, 1000)
pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(k, m, iters))
parent = g.Index.sorted(dm, pq).vector_index
Q = dm.get_rows(sample_rows(n, B, 0))
dm.close()
add = g.DeviceMatrix.synthetic(n_add, d, 3, 4321, 1000)
signal.alarm(0)
# the added rows land at random places among the old ones, as words in String order do
slots = np.zeros(n + n_add, bool)
slots[np.random.default_rng(5).choice(n + n_add, n_add, replace=False)] = True
take = np.zeros(n + n_add, np.int32)
take[slots] = -1 - np.arange(n_add, dtype=np.int32)
take[~slots] = np.arange(n, dtype=np.int32)

out = {"rows": n, "dim": d, "m": m, "k": k, "added": n_add}


def record(key, value):
    """Into the result line, and to stderr as it arrives (a long run shows where it is)."""
    out[key] = value
    print(key, json.dumps(value), file=sys.stderr, flush=True)


record("setup_s", round(time.perf_counter() - t_setup, 1))

# (a) encode_dataset alone
record("encode_dataset", timed(lambda: parent.encode(add).close()))

# (b) merge alone, the conflict ordering of the filter's copy on and off
encoded = parent.encode(add)
g.tune_live(GULON_FILTER_ORDER=0)
record("merge_without_ordering", timed(lambda: parent.merged(encoded, take).close(), steps=3))
g.tune_live(GULON_FILTER_ORDER=1)
record("merge_with_ordering", timed(lambda: parent.merged(encoded, take).close(), steps=3))


# (c) the host route on the same build: gulon_pq_encode to host bytes, a numpy merge, gulon_index_create
def host_route():
    new = pq.encode(add).indices()
    both = np.concatenate([parent.data.indices(), new], axis=1)
    idx = both[:, np.where(take >= 0, take, n + (-1 - take))]
    coder = pq.coder_factory(idx.shape[1])
    return g.PQIndex(pq, g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(m)]))


record("host_route", timed(lambda: host_route().close(), steps=1))

# the query check: one batch on the merged index and on the native index over the same codes
merged, native = parent.merged(encoded, take), host_route()
record("batch_on_merged", timed(lambda: merged.batch_query_raw(K, Q)))
record("batch_on_native", timed(lambda: native.batch_query_raw(K, Q)))
a, b = merged.batch_query_raw(K, Q), native.batch_query_raw(K, Q)
record("merged_equals_native", bool(all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))))
merged.close(), native.close(), encoded.close(), parent.close(), add.close()
print(json.dumps(out))
