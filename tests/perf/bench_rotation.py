"""Rotation benchmark at the headline shape (10 M x 128, m = 16, k = 256): what rotating the data, taking its second
moment and one training round cost on the device (csrc/rotate.hip, gulon_amd/rotation.py), and what the query rotation
adds to a batch of 1024 queries.  Timed, not gated: it asserts no threshold.
   python tests/perf/bench_rotation.py [rows] [dim]
The rotate kernel's time is set next to its arithmetic: 2 n d^2 lane operations (one multiply and one add per term --
nothing is fused) at the fp32 vector rate, 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz, an fma counted as one operation there.
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
from gulon_amd import rotation
from gulon_amd.recall import sample_rows

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 128
m, k, B, K, iters = 16, 256, 1024, 10, 10
WARMUP, BLOCKS = 2, 5
SECTION_LIMIT_S = 400                           # per timed section (SIGALRM ends the process)
VECTOR_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9    # one fp32 operation per lane per clock


def timed(step, steps=5, warmup=WARMUP, blocks=BLOCKS, sync=torch.cuda.synchronize):
    signal.alarm(SECTION_LIMIT_S)
    for _ in range(warmup):
        step()
    sync()
    times = []
    for _ in range(blocks):
        t = time.perf_counter()
        for _ in range(steps):
            step()
        sync()
        times.append((time.perf_counter() - t) / steps * 1e3)
    signal.alarm(0)
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "steps": steps}


out = {"rows": n, "dim": d, "m": m, "k": k}


def record(key, value):
    """Into the result line, and to stderr as it arrives (a long run shows where it is)."""
    out[key] = value
    print(key, json.dumps(value), file=sys.stderr, flush=True)


t_setup = time.perf_counter()
signal.alarm(SECTION_LIMIT_S)
dm = g.DeviceMatrix.synthetic(n, d, 3, 1234, 1000)
config = g.ProductQuantizerConfig(k, m, iters)
q, _ = np.linalg.qr(np.random.default_rng(0).normal(size=(d, d)))
rot = rotation.Rotation(q)
Q = dm.get_rows(sample_rows(n, B, 0))
signal.alarm(0)
record("setup_s", round(time.perf_counter() - t_setup, 1))

# (a) gulon_dataset_rotate: upload of R, allocation of the output and the kernel
t = timed(lambda: rot.apply_device(dm).close())
t["lane_ops"] = 2.0 * n * d * d
t["ms_at_vector_rate"] = t["lane_ops"] / VECTOR_LANE_OPS_PER_S * 1e3
t["share_of_vector_rate"] = t["ms_at_vector_rate"] / t["median_ms"]
record("dataset_rotate", t)

# (b) gulon_dataset_moment of the matrix with itself
record("dataset_moment", timed(lambda: rotation.moment(dm, dm)))

# (c) one training round: rotate, train the quantizer, encode, row errors, decode, moment, Procrustes
def training_round():
    error, decoded = rotation.rotation_error(dm, rot, config, decode=True)
    rotation.procrustes(rotation.moment(dm, decoded))
    decoded.close()


record("training_round", timed(training_round, steps=1, warmup=1, blocks=3))

# (d) a batch of 1024 queries with and without the query rotation, on an index over the rotated rows
rotated = rot.apply_device(dm)
pq = g.ProductQuantizer.apply(rotated, config)
inner = g.Index.sorted(rotated, pq)
rotated.close()


class _Inner:
    """The two members RotatedWordIndex reads of its inner index here."""
    dimension = d

    def batch_query_raw(self, k_nn, vectors):
        return inner.vector_index.batch_query_raw(k_nn, vectors)


outer = rotation.RotatedWordIndex(_Inner(), rot)
RQ = rot.apply(Q)
record("batch_without_rotation", timed(lambda: inner.vector_index.batch_query_raw(K, RQ), steps=10))
record("batch_with_rotation", timed(lambda: outer.batch_query_raw(K, Q), steps=10))
record("query_rotation_alone", timed(lambda: rot.apply(Q), steps=10))
inner.vector_index.close(), dm.close()
print(json.dumps(out))
