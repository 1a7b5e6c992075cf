"""word2vec text ingest: the host reader against the device reader, and build-index on the same file.

    python tests/perf/bench_ingest.py [--rows 100000] [--dim 300] [--modes host,device,build] [--file PATH]

Generates (or reuses) a ROWS x DIM file of %.6f tokens and prints one JSON line:
  host_s      word_vectors.read_word2vec (the per-token Python reader), wall time
  device_s    word_vectors.read_word2vec_device end to end: file read, copies, kernels, fix-ups, word decoding
              (best of --repeat runs after one warm-up), plus its stats
  build       the RUNNING/SUCCESS lines of `build-index -d l2` with the CLI's defaults, stage by stage
For the kernels alone run `--modes device` under `rocprofv3 --kernel-trace --stats` in a run of its own: the ingest_*
and normalize_rows kernels' total time over `text_bytes` is the parse rate."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def generate(path, rows, dim, seed=7):
    rng = np.random.default_rng(seed)
    with open(path, "w", encoding="utf-8", newline="\n") as fh:
        fh.write(f"{rows} {dim}\n")
        for s in range(0, rows, 2000):
            x = rng.uniform(-10, 10, (min(2000, rows - s), dim))
            toks = np.char.mod("%.6f", x)
            fh.write("".join(f"w{s + i} " + " ".join(r) + "\n" for i, r in enumerate(toks)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=300)
    ap.add_argument("--modes", default="host,device,build")
    ap.add_argument("--file", default=None)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    modes = args.modes.split(",")
    from gulon_amd import cli, word_vectors as W

    tmp = None
    path = args.file
    if path is None:
        tmp = tempfile.TemporaryDirectory()
        path = os.path.join(tmp.name, "vectors.txt")
    if not os.path.exists(path):
        generate(path, args.rows, args.dim)
    out = {"rows": args.rows, "dim": args.dim, "text_bytes": os.path.getsize(path)}
    if "device" in modes:
        times = []
        for _ in range(args.repeat + 1):
            t = time.perf_counter()
            dev = W.read_word2vec_device(path)
            times.append(time.perf_counter() - t)
            stats = dev.stats
            dev.matrix.close()
        out.update(device_first_s=round(times[0], 4), device_s=round(min(times[1:]), 4),
                   device_all_s=[round(t, 4) for t in times[1:]], flagged=stats.flagged, tokens=stats.tokens)
    if "host" in modes:
        t = time.perf_counter()
        host = W.read_word2vec(path)
        out["host_s"] = round(time.perf_counter() - t, 3)
        out["host_us_per_token"] = round(out["host_s"] / (host.size * host.dimension) * 1e6, 3)
        if "device" in modes:
            out["host_over_device"] = round(out["host_s"] / out["device_s"], 1)
    if "build" in modes:
        lines = []
        with tempfile.TemporaryDirectory() as d:
            t = time.perf_counter()
            cli.run_build_index(cli.BuildConfig("l2", 256, 25, 100, None, os.path.join(d, "index.bin"), path),
                                lines.append)
            out["build_s"] = round(time.perf_counter() - t, 3)
            out["index_bytes"] = os.path.getsize(os.path.join(d, "index.bin"))
        out["build"] = [ln.split("\u001b[0m ", 1)[1].strip() for ln in lines if "SUCCESS" in ln]
    print(json.dumps(out))
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
