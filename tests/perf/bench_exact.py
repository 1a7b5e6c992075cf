"""Exact-kNN benchmark: gulon_exact_knn (above 63 neighbours: 64 entries peeled per full pass over the rows) against
gulon_exact_index_batch_query (csrc/exact.hip: one pass behind a sample bound) on the same build, the dataset already in
HBM, host queries in and host results out for both.  Timed, not gated; it asserts that both return identical bits.
   python tests/perf/bench_exact.py [rows divisor]
Shapes: 1 M x 300 with 1 000 queries at k = 1 000 (the `test` command's), 10 M x 128 with 1 024 queries at k = 100 and
k = 1 000.  Every time is the median of BLOCKS blocks of back-to-back steps, after warm-up, the device idle before a
block.  Every timed section runs under an alarm: a step that hangs ends the script instead of holding the device."""
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gulon_amd as g
from gulon_amd import native as N
from gulon_amd.recall import sample_rows

DIV = int(sys.argv[1]) if len(sys.argv) > 1 else 1
SHAPES = [(1_000_000 // DIV, 300, 1000, 1000), (10_000_000 // DIV, 128, 1024, 100), (10_000_000 // DIV, 128, 1024, 1000)]
WARMUP, BLOCKS = 3, 7
SECTION_LIMIT_S = 400                           # per timed section (SIGALRM ends the process)


def sync():
    N.check(N.lib().gulon_device_synchronize())


def timed(step, steps):
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


def record(out, key, value):
    """Into the result, and to stderr as it arrives (a long run shows where it is)."""
    out[key] = value
    print(key, json.dumps(value), file=sys.stderr, flush=True)


results, dm, shape_of_dm = [], None, None
for n, d, b, k in SHAPES:
    out = {"rows": n, "dim": d, "queries": b, "k": k}
    if shape_of_dm != (n, d):
        if dm is not None:
            dm.close()
        signal.alarm(SECTION_LIMIT_S)
        dm, shape_of_dm = g.DeviceMatrix.synthetic(n, d, 3, 1234, 1000), (n, d)
        signal.alarm(0)
    Q = dm.get_rows(sample_rows(n, b, 0))
    oi, od = np.zeros((b, k), np.int32), np.zeros((b, k), np.float32)
    oc, of = np.zeros(b, np.int32), np.zeros(b, np.int32)
    ix = g.ExactIndex(dm)
    new = ix.batch_query_raw(k, Q)
    stats = ix.stats()
    record(out, "stats", stats)

    def peeled():
        N.check(N.lib().gulon_exact_knn(dm._h, 0, n, Q.reshape(-1), b, k, oi.reshape(-1), od.reshape(-1), oc, of))

    peeled()
    same = (np.array_equal(oi, new[0]) and np.array_equal(od.view(np.uint32), new[1].view(np.uint32))
            and np.array_equal(oc, new[2]) and np.array_equal(of, new[3]))
    record(out, "identical_bits", bool(same))
    assert same, "the exact index and gulon_exact_knn disagree"
    record(out, "gulon_exact_knn", timed(peeled, steps=1))
    record(out, "gulon_exact_index_batch_query", timed(lambda: ix.batch_query_raw(k, Q), steps=3))
    record(out, "speedup_of_medians", out["gulon_exact_knn"]["median_ms"] / out["gulon_exact_index_batch_query"]["median_ms"])
    record(out, "slowest_new_beats_fastest_old",
           out["gulon_exact_index_batch_query"]["max_ms"] < out["gulon_exact_knn"]["min_ms"])
    ix.close()
    results.append(out)
dm.close()
print(json.dumps(results))
