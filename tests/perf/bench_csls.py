"""Offset queries and the CSLS pass (csrc/offset.hip, gulon_amd/csls.py): device time of

  exact_offset   gulon_exact_index_query_offset_dev        the offset scan on an ExactIndex over the target vectors
  flat_offset    gulon_index_query_offset_dev              the same on a flat byte-code index of them (m = 16)
  exact_query    gulon_exact_index_batch_query_dev         the handle's ordinary query, the yardstick already in the tree
  flat_query     gulon_index_batch_query_dev
  exact_cosmul   gulon_exact_index_query_cosmul_dev        the E = 1 3CosMul scan: one-term expressions over target rows
  flat_cosmul    gulon_index_query_cosmul_dev
  csls_exact     csls_offsets(exact target, source)        r_S of every target row: compose, the source's neighbours, mean
  csls_flat      csls_offsets(flat target, source)

for `--queries` source words at k = 10.  Every argument lives on the device before the clock starts; a step is the call
and a device synchronisation, timed on the host.  WARMUP steps per route, then REPEATS timed steps, the routes
alternating; median and range.  The two csls passes are long (rows x rows distances) and take fewer steps.

  python tests/perf/bench_csls.py [--rows 200000] [--dim 300] [--queries 1500] [--quantizers 16] [--train-iters 2]

Both sides are standard-normal rows normalised on the host, the source a perturbed copy of the target.  Prints progress
lines and one JSON line.  A measurement needs the GPU: without one the library fails to start."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gulon_amd as g
from gulon_amd import native as N
from gulon_amd.refine import _DeviceArray

WARMUP, REPEATS, PASS_WARMUP, PASS_REPEATS, K = 3, 7, 1, 3, 10


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
    p.add_argument("--quantizers", type=int, default=16)
    p.add_argument("--clusters", type=int, default=256)
    p.add_argument("--train-iters", type=int, default=2)
    p.add_argument("--neighbours", type=int, default=10)
    args = p.parse_args()
    n, d, b = args.rows, args.dim, args.queries
    L = N.lib()

    def note(text):
        print(f"[{time.strftime('%H:%M:%S')}] {text}", flush=True)

    t0 = time.perf_counter()
    T = unit_rows(n, d, 1234)
    S = unit_rows(n, d, 99, base=T, noise=0.03)
    tdm, sdm = g.DeviceMatrix.from_host(T), g.DeviceMatrix.from_host(S)
    pq = g.ProductQuantizer.apply(tdm, g.ProductQuantizerConfig(args.clusters, args.quantizers, args.train_iters))
    flat = g.Index.sorted(tdm, pq, "cosine")
    exact, source = g.ExactIndex(tdm, "cosine"), g.ExactIndex(sdm, "cosine")
    vi = flat.vector_index
    note(f"{n} x {d} unit vectors on both sides, index m = {args.quantizers} / k = {args.clusters} built in "
         f"{time.perf_counter() - t0:.1f} s")

    rows = np.random.default_rng(0).choice(n, b, replace=False).astype(np.int32)
    dev = {name: _DeviceArray() for name in ("q", "oi", "od", "oc", "of", "off", "rows", "w")}
    dev["q"].upload(np.ascontiguousarray(S[rows]))
    dev["off"].upload(np.arange(b + 1, dtype=np.int32)), dev["rows"].upload(rows), dev["w"].upload(np.ones(b, np.float32))
    for name, nbytes in (("oi", 4 * b * K), ("od", 4 * b * K), ("oc", 4 * b), ("of", 4 * b)):
        dev[name].ensure(nbytes)
    q, oi, od, oc, of = (dev[name].ptr for name in ("q", "oi", "od", "oc", "of"))
    offsets = g.csls_offsets(exact, source, args.neighbours)

    def step(call):
        t = time.perf_counter()
        call()
        N.check(L.gulon_device_synchronize())
        return time.perf_counter() - t

    routes = {
        "exact_offset": lambda: N.check(L.gulon_exact_index_query_offset_dev(exact._h, q, b, K, offsets.ptr, None, oi, od,
                                                                             oc, None)),
        "exact_query": lambda: N.check(L.gulon_exact_index_batch_query_dev(exact._h, q, b, K, oi, od, oc, of, None)),
        "exact_cosmul": lambda: N.check(L.gulon_exact_index_query_cosmul_dev(exact._h, dev["off"].ptr, dev["rows"].ptr,
                                                                             dev["w"].ptr, b, K, 1, oi, od, oc, None, None)),
        "flat_offset": lambda: N.check(L.gulon_index_query_offset_dev(vi._h, q, b, K, 0, n, offsets.ptr, None, oi, od, oc,
                                                                      None)),
        "flat_query": lambda: N.check(L.gulon_index_batch_query_dev(vi._h, q, b, K, 0, n, oi, od, oc, of, None)),
        "flat_cosmul": lambda: N.check(L.gulon_index_query_cosmul_dev(vi._h, dev["off"].ptr, dev["rows"].ptr, dev["w"].ptr,
                                                                      b, K, 1, 0, n, oi, od, oc, None)),
    }
    times = {name: [] for name in routes}
    for s in range(WARMUP + REPEATS):
        last = {name: step(call) for name, call in routes.items()}
        if s >= WARMUP:
            for name, dt in last.items():
                times[name].append(dt)
        note(f"step {s}: " + ", ".join(f"{name} {dt * 1e3:.2f} ms" for name, dt in last.items())
             + (" (warm-up)" if s < WARMUP else ""))

    def whole_pass(target):
        g.csls_offsets(target, source, args.neighbours).free()     # (synchronises before it returns)

    passes = {"csls_exact": lambda: whole_pass(exact), "csls_flat": lambda: whole_pass(flat)}
    for name in passes:
        times[name] = []
    for s in range(PASS_WARMUP + PASS_REPEATS):
        for name, call in passes.items():
            dt = step(call)
            if s >= PASS_WARMUP:
                times[name].append(dt)
            note(f"pass {s} {name}: {dt * 1e3:.0f} ms" + (" (warm-up)" if s < PASS_WARMUP else ""))

    out = {"workload": f"{b} source words against {n} x {d} unit target vectors at k = {K}; flat index m = "
                       f"{args.quantizers} / k = {args.clusters}; csls passes: r_S of {n} target rows from their "
                       f"{args.neighbours} nearest of {n} source rows; median and range of {REPEATS} steps after {WARMUP} "
                       f"warm-up steps ({PASS_REPEATS} after {PASS_WARMUP} for the passes)",
           "routes": {name: {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}
                      for name, ts in times.items()}}
    print(json.dumps(out), flush=True)
    offsets.free()
    for a in dev.values():
        a.free()


if __name__ == "__main__":
    main()
