"""The offsets pass of the inverted softmax against the CSLS pass it shares its loop with (gulon_amd/csls.py,
csrc/logsumexp.hip): time of

  isf_offsets    csls.isf_offsets(target, source, beta = 30)     per target row the log of a sum over EVERY source row
  csls_offsets   csls.csls_offsets(target, source, K = 10)       per target row the mean over its 10 nearest source rows

on an ExactIndex over the target and one over the source.  Both cost the same n_t x n_s distance work, in the same
passes of 4096 composed target rows; one ends in a selection, the other in a binary64 exp and sum per pair, and in a
download of the composed rows and an upload of the offsets per pass.  csls_offsets is the yardstick: its device code is
older than this file.  What the exp itself costs shows in two more routes, one pass of 4096 target rows each through
the C entry points: logsumexp_pass beside rank_pass, the rank queries' counting scan, which forms the same distances
in the same geometry and keeps two counters where the other takes an exp.  WARMUP steps per route, then REPEATS timed steps of one call each, the routes alternating; median
and range.

  python tests/perf/bench_isf.py [--rows 200000] [--dim 300] [--beta 30] [--neighbours 10]

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

WARMUP, REPEATS = 3, 7


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
    p.add_argument("--beta", type=float, default=30.0)
    p.add_argument("--neighbours", type=int, default=10)
    args = p.parse_args()
    n, d = args.rows, args.dim

    def note(text):
        print(f"[{time.strftime('%H:%M:%S')}] {text}", flush=True)

    t0 = time.perf_counter()
    T = unit_rows(n, d, 1234)
    S = unit_rows(n, d, 99, base=T, noise=0.03)
    tdm, sdm = g.DeviceMatrix.from_host(T), g.DeviceMatrix.from_host(S)
    target, source = g.ExactIndex(tdm, "cosine"), g.ExactIndex(sdm, "cosine")
    note(f"{n} x {d} unit vectors on both sides in {time.perf_counter() - t0:.1f} s")

    kept = {}

    def run(name, fn):
        t = time.perf_counter()
        dev = fn()
        dt = time.perf_counter() - t
        if name not in kept:
            kept[name] = dev.numpy()
        dev.free()
        return dt

    # one pass of the two scans that differ in the exp alone: the same 4096 target rows against the source through
    # the C entry points, the log-sum-exp scan beside the rank queries' counting scan (one gold row per query, no offsets)
    from gulon_amd import native as N
    from gulon_amd.ranks import gold_lists
    L, pb = N.lib(), min(4096, n)
    pq = N.f32(T[:pb]).reshape(-1)
    goff, grows = gold_lists([[r] for r in range(pb)], pb)
    lse, terms = np.zeros(pb, np.float64), np.zeros(pb, np.int32)
    rank, row, key = np.zeros(pb, np.int32), np.zeros(pb, np.int32), np.zeros(pb, np.float32)

    def timed(call):
        def go():
            t = time.perf_counter()
            N.check(call())
            return time.perf_counter() - t
        return go

    passes = {
        "logsumexp_pass": timed(lambda: L.gulon_exact_index_query_logsumexp(source._h, pq, pb, args.beta, None, lse,
                                                                            terms.ctypes.data)),
        "rank_pass": timed(lambda: L.gulon_exact_index_query_rank(source._h, pq, pb, None, None, goff, grows, rank, row,
                                                                  key, None)),
    }
    routes = {"isf_offsets": lambda: g.isf_offsets(target, source, args.beta),
              "csls_offsets": lambda: g.csls_offsets(target, source, args.neighbours)}
    times = {name: [] for name in list(routes) + list(passes)}
    for s in range(WARMUP + REPEATS):
        last = {name: run(name, fn) for name, fn in routes.items()}
        last.update({name: go() for name, go in passes.items()})
        if s >= WARMUP:
            for name, dt in last.items():
                times[name].append(dt)
        note(f"step {s}: " + ", ".join(f"{name} {dt * 1e3:.1f} ms" for name, dt in last.items())
             + (" (warm-up)" if s < WARMUP else ""))
    for name, off in kept.items():
        assert off.shape == (n,) and np.isfinite(off).all(), name
    out = {"workload": f"offsets for {n} x {d} unit target vectors over {n} source vectors on two exact indexes; "
                       f"isf at beta = {args.beta:g}, csls at K = {args.neighbours}; per call: median and range of {REPEATS} "
                       f"steps of one call after {WARMUP} warm-up steps, routes alternating; logsumexp_pass / rank_pass: "
                       f"one host-pointer call for {pb} target rows, the scan with and without the exp",
           "exp_share_of_the_scan": 1.0 - statistics.median(times["rank_pass"]) / statistics.median(times["logsumexp_pass"]),
           "routes": {name: {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}
                      for name, ts in times.items()},
           "isf_over_csls": statistics.median(times["isf_offsets"]) / statistics.median(times["csls_offsets"])}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
