"""Analogy accuracy (gulon_amd/analogies.py): the time of one whole evaluation of a questions-words.txt sized
set by its three routes --
  index / device    WordIndex: gulon_index_query_terms_dev -> gulon_analogy_counts_dev per batch, one read at the end
  exact / device    ExactWordIndex over the same vectors: gulon_exact_index_query_terms_dev -> the same counts
  index / generic   the same WordIndex through batch_query_expressions and the host form of the counts
A step is one evaluate_analogies over all the questions; it ends in a blocking device-to-host copy of the counters, so
the host clock around it covers the device work.  Three warm-up steps per route, then seven timed steps per route, the
routes alternating; median and range of the seven.  The reports of the two index routes must be equal.

  python tests/perf/bench_analogies.py [--rows 1000000] [--dim 300] [--questions 19544] [--train-iters 2]

prints progress lines and one JSON line.  A measurement needs the GPU: without one the library fails to start."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gulon_amd as g
from gulon_amd.analogies import evaluate_analogies

WARMUP, BLOCKS, SECTIONS, KS = 3, 7, 14, (1, 5, 10)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=300)
    p.add_argument("--questions", type=int, default=19_544)
    p.add_argument("--quantizers", type=int, default=25)
    p.add_argument("--clusters", type=int, default=256)
    p.add_argument("--train-iters", type=int, default=2)
    args = p.parse_args()
    n, d = args.rows, args.dim

    def note(text):
        print(f"[{time.strftime('%H:%M:%S')}] {text}", flush=True)

    t0 = time.perf_counter()
    dm = g.DeviceMatrix.synthetic(n, d, 1, 1234, 1000)
    pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(args.clusters, args.quantizers, args.train_iters))
    words = [f"w{i:07d}" for i in range(n)]                       # String order = row order
    index = g.WordIndex(words, g.Index.sorted(dm, pq, "l2"))
    exact = g.ExactWordIndex(words, g.ExactIndex(dm, "l2"), index.key_index)
    note(f"{n} x {d} synthetic vectors, index m = {args.quantizers} / k = {args.clusters} built in "
         f"{time.perf_counter() - t0:.1f} s")
    rng = np.random.default_rng(0)
    rows = rng.integers(0, n, (args.questions, 4))
    while True:                                                   # four distinct words per question
        again = np.flatnonzero([len(set(q)) < 4 for q in rows.tolist()])
        if not len(again):
            break
        rows[again] = rng.integers(0, n, (len(again), 4))
    per = -(-args.questions // SECTIONS)
    sections = [(f"section {s}", [tuple(words[int(r)] for r in q) for q in rows[s * per:(s + 1) * per]])
                for s in range(SECTIONS)]
    routes = (("index_device", index, None), ("exact_device", exact, None), ("index_generic", index, "generic"))
    reports, times = {}, {name: [] for name, _, _ in routes}
    for step in range(WARMUP + BLOCKS):
        for name, target, route in routes:
            t = time.perf_counter()
            reports[name] = evaluate_analogies(target, sections, KS, route=route)
            dt = time.perf_counter() - t
            if step >= WARMUP:
                times[name].append(dt)
            note(f"step {step} {name}: {dt * 1e3:.1f} ms" + (" (warm-up)" if step < WARMUP else ""))
    assert reports["index_device"].lines() == reports["index_generic"].lines(), "the routes disagree"
    assert all(r.asked == args.questions and r.skipped == 0 for r in reports.values())
    out = {"workload": f"{args.questions} questions in {SECTIONS} sections, ks = {list(KS)}, over {n} x {d} synthetic "
                       f"vectors; index m = {args.quantizers} / k = {args.clusters}; median and range of {BLOCKS} steps "
                       f"after {WARMUP} warm-up steps, one step = one whole evaluation",
           "routes": {name: {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3,
                             "questions_per_s": args.questions / statistics.median(ts)} for name, ts in times.items()},
           "accuracy_at_1": {name: r.hits[1] / max(r.asked, 1) for name, r in reports.items()}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
