"""Offset queries on the grouped index (csrc/grouped_offset.hip): host time of three routes on one handle,

  offset    gulon_grouped_index_query_offset     the offset scan over every searched (query, group) pair
  query     gulon_grouped_index_batch_query      the ordinary query: pre-selection, re-rank, literal redo of what it flags
  literal   the same under GULON_GROUPED_LITERAL=1: every (query, group) pair through the literal heaps -- the yardstick,
            since it builds the same tables and walks the same rows as the offset scan

for `--queries` rows of the index at k = 10.  All three are host-pointer forms: a step is the call, which uploads the
queries (the offset route: the n row offsets too), runs on the null stream, downloads the answers and synchronises, timed
on the host.  WARMUP steps per route, then REPEATS timed steps, the routes alternating; median and range.

  python tests/perf/bench_grouped_offset.py [--rows 1000000] [--dim 128] [--partitions 1000] [--limit 50] [--queries 1024]

Prints progress lines and one JSON line.  A measurement needs the GPU: without one the library fails to start."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gulon_amd as g
from gulon_amd.recall import sample_rows

WARMUP, REPEATS, K = 3, 7, 10


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--partitions", type=int, default=1000)
    p.add_argument("--limit", type=int, default=50)
    p.add_argument("--queries", type=int, default=1024)
    p.add_argument("--quantizers", type=int, default=16)
    p.add_argument("--clusters", type=int, default=256)
    p.add_argument("--train-iters", type=int, default=3)
    args = p.parse_args()
    n, d, b = args.rows, args.dim, args.queries

    def note(text):
        print(f"[{time.strftime('%H:%M:%S')}] {text}", flush=True)

    t0 = time.perf_counter()
    dm = g.DeviceMatrix.synthetic(n, d, 3, 1234, 1000)
    coarse = g.KMeans.compute_clusters(g.Vectors(dm), g.KMeansConfig(args.partitions, args.train_iters))
    gv = g.group(dm, coarse)
    pq = g.ProductQuantizer.apply(gv.residuals, g.ProductQuantizerConfig(args.clusters, args.quantizers, args.train_iters))
    index = g.Index.grouped(gv, pq, g.LimitGroups(args.limit))
    note(f"{n} x {d}, {len(gv.centroids)} groups, LimitGroups({args.limit}), residual PQ m = {args.quantizers} / k = "
         f"{args.clusters} built in {time.perf_counter() - t0:.1f} s")
    Q = dm.get_rows(sample_rows(n, b, 0))
    offsets = np.random.default_rng(0).random(n).astype(np.float32)

    def literal():
        os.environ["GULON_GROUPED_LITERAL"] = "1"
        try:
            return index.batch_query_raw(K, Q)
        finally:
            del os.environ["GULON_GROUPED_LITERAL"]

    routes = {"offset": lambda: index.batch_query_offset_raw(K, Q, offsets),
              "query": lambda: index.batch_query_raw(K, Q),
              "literal": literal}

    def step(call):
        t = time.perf_counter()
        call()
        return time.perf_counter() - t

    times = {name: [] for name in routes}
    for s in range(WARMUP + REPEATS):
        last = {name: step(call) for name, call in routes.items()}
        if s >= WARMUP:
            for name, dt in last.items():
                times[name].append(dt)
        note(f"step {s}: " + ", ".join(f"{name} {dt * 1e3:.2f} ms" for name, dt in last.items())
             + (" (warm-up)" if s < WARMUP else ""))
    zero = index.batch_query_offset_raw(K, Q[:64], np.zeros(n, np.float32))
    plain = literal()
    agree = bool(np.array_equal(zero[1].view(np.uint32), plain[1][:64].view(np.uint32)))
    out = {"workload": f"{b} queries against a GroupedIndex of {n} x {d}, {len(gv.centroids)} groups, LimitGroups("
                       f"{args.limit}), residual PQ m = {args.quantizers} / k = {args.clusters}, k = {K}; host-pointer "
                       f"forms, transfers included; median and range of {REPEATS} steps after {WARMUP} warm-up steps",
           "routes": {name: {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}
                      for name, ts in times.items()},
           "zero_offsets_give_the_literal_distances": agree}
    print(json.dumps(out), flush=True)
    index.close()


if __name__ == "__main__":
    main()
