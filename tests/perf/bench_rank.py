"""Rank queries against the offset query they are the counting twin of (csrc/rank.hip, csrc/offset.hip):
time of the host-pointer calls

  exact_rank     gulon_exact_index_query_rank      one gold row per query, CSLS offsets, on an ExactIndex over the target
  exact_offset   gulon_exact_index_query_offset    the offset query at k = 10 on the same handle: the yardstick in the tree
  flat_rank      gulon_index_query_rank            the same on a flat byte-code index of the target (m = 25)
  flat_offset    gulon_index_query_offset

for `--queries` source words.  Both forms of a pair take the same queries and the same offsets from host memory, upload
them, run on the null stream and return when the answer has arrived, so a step is CALLS calls timed on the host.  WARMUP
steps per route, then REPEATS timed steps, the routes alternating; median and range per call.  The ranks are checked
against the offset query's lists before anything is timed: a rank below 10 must be the position of its row.

  python tests/perf/bench_rank.py [--rows 200000] [--dim 300] [--queries 1500] [--quantizers 25] [--train-iters 2]

Both sides are standard-normal rows normalised on the host, the source a perturbed copy of the target, and the gold row of
a source word is the target row it was made from.  Prints progress lines and one JSON line.  A measurement needs the GPU:
without one the library fails to start."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gulon_amd as g

WARMUP, REPEATS, CALLS, K = 3, 7, 5, 10


def unit_rows(n, d, seed, base=None, noise=0.0, chunk=1 << 16):
    rng = np.random.default_rng(seed)
    out = np.empty((n, d), np.float32)
    for s in range(0, n, chunk):
        x = rng.standard_normal((min(chunk, n - s), d), dtype=np.float32)
        if base is not None:
            x = base[s:s + chunk] + np.float32(noise) * x
        out[s:s + chunk] = x / np.linalg.norm(x, axis=1, keepdims=True)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=200_000)
    p.add_argument("--dim", type=int, default=300)
    p.add_argument("--queries", type=int, default=1500)
    p.add_argument("--quantizers", type=int, default=25)
    p.add_argument("--clusters", type=int, default=256)
    p.add_argument("--train-iters", type=int, default=2)
    p.add_argument("--neighbours", type=int, default=10)
    args = p.parse_args()
    n, d, b = args.rows, args.dim, args.queries

    def note(text):
        print(f"[{time.strftime('%H:%M:%S')}] {text}", flush=True)

    t0 = time.perf_counter()
    T = unit_rows(n, d, 1234)
    S = unit_rows(n, d, 99, base=T, noise=0.03)
    tdm, sdm = g.DeviceMatrix.from_host(T), g.DeviceMatrix.from_host(S)
    pq = g.ProductQuantizer.apply(tdm, g.ProductQuantizerConfig(args.clusters, args.quantizers, args.train_iters))
    flat = g.Index.sorted(tdm, pq, "cosine")
    exact, source = g.ExactIndex(tdm, "cosine"), g.ExactIndex(sdm, "cosine")
    note(f"{n} x {d} unit vectors on both sides, index m = {args.quantizers} / k = {args.clusters} built in "
         f"{time.perf_counter() - t0:.1f} s")

    rows = np.random.default_rng(0).choice(n, b, replace=False).astype(np.int32)
    Q = np.ascontiguousarray(S[rows])
    gold = [[int(r)] for r in rows]
    device = g.csls_offsets(exact, source, args.neighbours)
    offsets = device.numpy()
    device.free()

    # the C entry points on arrays laid out once: a step times the library, not the marshalling of the Python classes
    from gulon_amd import native as N
    from gulon_amd.ranks import gold_lists
    L, vi = N.lib(), flat.vector_index
    qe, qf = N.f32(exact._prepare(Q)).reshape(-1), N.f32(flat._prepare(Q)).reshape(-1)
    goff, grows = gold_lists(gold, b)
    rank, row, total = np.zeros(b, np.int32), np.zeros(b, np.int32), np.zeros(b, np.int32)
    key = np.zeros(b, np.float32)
    oi, od, oc = np.zeros(b * K, np.int32), np.zeros(b * K, np.float32), np.zeros(b, np.int32)
    off = offsets.ctypes.data
    routes = {
        "exact_rank": lambda: N.check(L.gulon_exact_index_query_rank(exact._h, qe, b, off, None, goff, grows, rank, row, key,
                                                                     total.ctypes.data)),
        "exact_offset": lambda: N.check(L.gulon_exact_index_query_offset(exact._h, qe, b, K, offsets, None, oi, od, oc)),
        "flat_rank": lambda: N.check(L.gulon_index_query_rank(vi._h, qf, b, 0, n, off, None, goff, grows, rank, row, key,
                                                              total.ctypes.data)),
        "flat_offset": lambda: N.check(L.gulon_index_query_offset(vi._h, qf, b, K, 0, n, offsets, None, oi, od, oc)),
    }
    for side in ("exact", "flat"):                               # the ranks are the positions in the lists
        routes[side + "_rank"]()
        routes[side + "_offset"]()
        near = np.flatnonzero((rank >= 0) & (rank < K))
        assert np.array_equal(oi.reshape(b, K)[near, rank[near]], row[near]) and (total == n).all(), side
        note(f"{side}: {len(near)} of {b} gold rows among the first {K}, mrr {np.mean(1.0 / (rank + 1.0)):.4f}")

    def step(call):
        t = time.perf_counter()
        for _ in range(CALLS):
            call()
        return (time.perf_counter() - t) / CALLS

    times = {name: [] for name in routes}
    for s in range(WARMUP + REPEATS):
        last = {name: step(call) for name, call in routes.items()}
        if s >= WARMUP:
            for name, dt in last.items():
                times[name].append(dt)
        note(f"step {s}: " + ", ".join(f"{name} {dt * 1e3:.2f} ms" for name, dt in last.items())
             + (" (warm-up)" if s < WARMUP else ""))

    out = {"workload": f"{b} source words against {n} x {d} unit target vectors, CSLS offsets; rank: one gold row per "
                       f"word; offset query at k = {K}; flat index m = {args.quantizers} / k = {args.clusters}; host-pointer "
                       f"calls, per call: median and range of {REPEATS} steps of {CALLS} calls after {WARMUP} warm-up steps",
           "routes": {name: {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}
                      for name, ts in times.items()}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
