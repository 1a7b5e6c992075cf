"""Alignment (csrc/alignment.hip, gulon_amd/alignment.py): wall time, device synchronised, of

  induce          induce_matches                       one dictionary induction with the seed map: X W, two exact indexes,
                                                       the two csls_offsets passes, the two best-match passes, the mutual test
  train           train_alignment                      the seed solve and `--rounds` + 1 inductions with their moments and SVDs
  pair_moment     gulon_dataset_pair_moment_dev        the moment of --pairs row pairs, a tenth of them -1, lists on the device
  gather_moment   gulon_dataset_gather x 2 +           the route without it, from entry points the tree already had: the live
                  gulon_dataset_moment                 pairs compacted on the host, both sides gathered into new datasets,
                                                       the full-matrix moment of the two copies

at `--rows` x `--dim` unit vectors per side with MUSE's defaults (max_rank 15000, 10 neighbours, 5 rounds).  The source is
a rotated, lightly perturbed, permuted copy of the target; the seed dictionary is `--seed-pairs` true pairs.  WARMUP
steps per route, then REPEATS timed ones; median and range.  `train` is long and runs once after one induction has
warmed the kernels up.

  python tests/perf/bench_alignment.py [--rows 200000] [--dim 300] [--pairs 15000] [--rounds 5]

Prints progress lines and one JSON line.  A measurement needs the GPU: without one the library fails to start."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gulon_amd as g
from gulon_amd import alignment, rotation
from gulon_amd import native as N
from gulon_amd.refine import _DeviceArray

WARMUP, REPEATS, PASS_WARMUP, PASS_REPEATS = 3, 7, 1, 3


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
    p.add_argument("--pairs", type=int, default=15_000)
    p.add_argument("--seed-pairs", type=int, default=5000)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--max-rank", type=int, default=15_000)
    p.add_argument("--neighbours", type=int, default=10)
    args = p.parse_args()
    n, d = args.rows, args.dim
    L = N.lib()

    def note(text):
        print(f"[{time.strftime('%H:%M:%S')}] {text}", flush=True)

    t0 = time.perf_counter()
    rng = np.random.default_rng(7)
    Y = unit_rows(n, d, 1234)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    perm = np.concatenate([rng.permutation(min(n, args.max_rank)), np.arange(min(n, args.max_rank), n)])
    X = unit_rows(n, d, 99, base=(Y[perm] @ q.T.astype(np.float32)), noise=0.03)
    source = g.DeviceWordVectors([f"s{i}" for i in range(n)], g.DeviceMatrix.from_host(X))
    target = g.DeviceWordVectors([f"t{i}" for i in range(n)], g.DeviceMatrix.from_host(Y))
    seed_rows = rng.choice(min(n, args.max_rank), min(args.seed_pairs, n, args.max_rank), replace=False)
    pairs = [(f"s{i}", f"t{perm[i]}") for i in seed_rows.tolist()]
    note(f"{n} x {d} unit vectors on both sides, {len(pairs)} seed pairs, ready in {time.perf_counter() - t0:.1f} s")

    def step(call):
        t = time.perf_counter()
        out = call()
        N.check(L.gulon_device_synchronize())
        return time.perf_counter() - t, out

    times = {}
    seed_map, used, _ = alignment.seed_alignment(source, target, pairs)

    def induce():
        fwd, match = alignment.induce_matches(source.matrix, target.matrix, seed_map, args.max_rank, args.neighbours)
        fwd.free(), match.free()
    times["induce"] = []
    for s in range(PASS_WARMUP + PASS_REPEATS):
        dt, _ = step(induce)
        if s >= PASS_WARMUP:
            times["induce"].append(dt)
        note(f"induce {s}: {dt * 1e3:.0f} ms" + (" (warm-up)" if s < PASS_WARMUP else ""))
    dt, (_, history) = step(lambda: alignment.train_alignment(source, target, pairs, args.rounds, args.max_rank,
                                                              args.neighbours))
    times["train"] = [dt]
    note(f"train: {dt * 1e3:.0f} ms, rounds {history['rounds']}, chosen {history['chosen']}")

    # the moment of a round's match list against the route through two gathers
    m = args.pairs
    ra = np.arange(m, dtype=np.int32) % n
    rb = rng.integers(0, n, m).astype(np.int32)
    rb[rng.random(m) < 0.1] = -1
    d_ra, d_rb = _DeviceArray(), _DeviceArray()
    d_ra.upload(ra), d_rb.upload(rb)

    def pair_moment():
        return alignment.pair_moment_dev(source.matrix, target.matrix, d_ra.ptr, d_rb.ptr, m)[0]

    def gather_moment():
        live = rb >= 0                                            # the list comes to the host to be compacted
        ga, gb = np.ascontiguousarray(ra[live]), np.ascontiguousarray(rb[live])
        copies = []
        for matrix, rows in ((source.matrix, ga), (target.matrix, gb)):
            h = C.c_void_p()
            N.check(L.gulon_dataset_gather(matrix._h, rows, len(rows), C.byref(h)))
            copies.append(g.DeviceMatrix(h, len(rows), d))
        try:
            return rotation.moment(copies[0], copies[1])
        finally:
            copies[0].close(), copies[1].close()
    routes = {"pair_moment": pair_moment, "gather_moment": gather_moment}
    for name in routes:
        times[name] = []
    results = {}
    for s in range(WARMUP + REPEATS):
        last = {}
        for name, call in routes.items():
            last[name], results[name] = step(call)
            if s >= WARMUP:
                times[name].append(last[name])
        note(f"step {s}: " + ", ".join(f"{name} {dt * 1e3:.3f} ms" for name, dt in last.items())
             + (" (warm-up)" if s < WARMUP else ""))
    # the two routes add the same products in different chunkings: equal up to the rounding of the additions
    scale = np.abs(results["gather_moment"]).max()
    note(f"largest difference between the routes: {np.abs(results['pair_moment'] - results['gather_moment']).max():.3e} "
         f"(largest entry {scale:.3e})")

    out = {"workload": f"{n} x {d} unit vectors per side, max_rank {args.max_rank}, {args.neighbours} neighbours, "
                       f"{args.rounds} rounds, {len(pairs)} seed pairs; moments of {m} pairs, a tenth of them skipped; "
                       f"induce: median and range of {PASS_REPEATS} after {PASS_WARMUP} warm-up; train: one run; moments: "
                       f"{REPEATS} after {WARMUP}",
           "routes": {name: {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}
                      for name, ts in times.items()},
           "train_rounds": history["rounds"], "chosen": history["chosen"]}
    print(json.dumps(out), flush=True)
    d_ra.free(), d_rb.free()
    source.matrix.close(), target.matrix.close()


if __name__ == "__main__":
    main()
