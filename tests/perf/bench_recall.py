"""Stage times of `python -m gulon_amd test` (tests_recall.Tests, csrc/recall.hip); prints one JSON line.

N x D synthetic rows (clustered, DeviceMatrix.synthetic), a sorted and a grouped index over them, --sample queries,
k up to 1000.  Per index: the index query at maxK and the evaluation; once: sample + exact kNN.  The evaluation is timed
two ways on the same inputs, alternating, --reps times each: gulon_recall_counts (distances and counts on the device),
and the way it had to be done before it -- gulon_distance_sq_rows, the B x maxK distances copied back, counted in numpy.
Both must give the same counts.  --ingest-rows R > 0 also writes R x D rows as word2vec text and times
read_word2vec_device on it (the text of the full 1 M x 300 is 2.9 GB: the ingest is measured on a part).
Every time is a host clock around a call that ends in a device synchronisation."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=300)
    ap.add_argument("--m", type=int, default=25)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--sample", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--limit", type=int, default=50)
    ap.add_argument("--ingest-rows", type=int, default=0)
    ap.add_argument("--no-grouped", action="store_true")
    a = ap.parse_args()

    import gulon_amd as g
    from gulon_amd import native as N
    from gulon_amd import tests_recall as tr
    n, d = a.n, a.d
    out = {"shape": {"n": n, "d": d, "m": a.m, "sample": a.sample, "ks": list(tr.DEFAULT_KS)}}

    if a.ingest_rows:
        part = g.DeviceMatrix.synthetic(a.ingest_rows, d, 1, 7, 1000).to_host()
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "vectors.txt")
            with open(path, "w") as fh:
                fh.write(f"{a.ingest_rows} {d}\n")
                for s in range(0, a.ingest_rows, 10000):
                    fh.write("".join(f"w{s + i:07d} " + " ".join(map("{:.6f}".format, row)) + "\n"
                                     for i, row in enumerate(part[s:s + 10000].tolist())))
            g.read_word2vec_device(path)
            _, ms = timed(lambda: g.read_word2vec_device(path))
        out["ingest"] = {"rows": a.ingest_rows, "ms": ms}

    dm = g.DeviceMatrix.synthetic(n, d, 1, 7, 1000)
    words = [f"w{i:07d}" for i in range(n)]
    vectors = g.DeviceWordVectors(words, dm, g.KeyIndexSorted(words))
    tr.Tests.sample(vectors, 16)                                        # warm-up of the peeled exact kNN
    tests, ms = timed(lambda: tr.Tests.sample(vectors, a.sample))
    out["sample_exact_knn_ms"] = ms
    ks = np.asarray(tests.ks, np.int32)
    max_k = int(ks[-1])
    cut = tr.cutoff(tests.kth, 0.0)
    cfg = g.ProductQuantizerConfig(256, a.m, a.iters)

    def old_way(rows):
        dist = np.zeros(rows.shape, np.float32)
        N.check(N.lib().gulon_distance_sq_rows(dm._h, tests.queries.reshape(-1), len(rows), rows.reshape(-1), max_k,
                                               dist.reshape(-1)))
        pos = np.arange(max_k)
        return np.stack([((rows >= 0) & (pos[None, :] < k) & (dist <= cut[:, j][:, None])).sum(axis=1)
                         for j, k in enumerate(ks)], axis=1).astype(np.int32)

    def measure(name, index):
        index.batch_query_raw(max_k, tests.queries[:16])
        (rows, _, counts, flags), q_ms = timed(lambda: index.batch_query_raw(max_k, tests.queries))
        row_map = np.full(index.size, -2, np.int64)
        vrows, map_ms = timed(lambda: tests._vector_rows(index, rows, row_map))
        new_way = lambda: tr.recall_counts(dm, tests.queries, vrows, ks, cut)
        assert np.array_equal(new_way(), old_way(vrows)), "the two evaluations disagree"
        new_ms, old_ms = [], []
        for _ in range(a.reps):                                          # alternating, same process, same inputs
            new_ms.append(timed(new_way)[1])
            old_ms.append(timed(lambda: old_way(vrows))[1])
        _, total_ms = timed(lambda: tests.recall_of(index))
        out[name] = {"index_query_ms": q_ms, "word_to_row_ms": map_ms, "evaluate_new_ms": new_ms,
                     "evaluate_old_ms": old_ms, "old_over_new": float(np.median(old_ms) / np.median(new_ms)),
                     "recall_of_ms": total_ms, "flagged": int(np.count_nonzero(flags & 3)),
                     "mean_count": float(counts.mean())}

    pq = g.ProductQuantizer.apply(dm, cfg)
    srt = g.WordIndex(words, g.Index.sorted(dm, pq))
    measure("sorted", srt)
    srt.close()
    if not a.no_grouped:
        clustering = g.KMeans.compute_clusters(g.Vectors(dm), g.KMeansConfig(a.groups, a.iters))
        gw, gv = vectors.grouped(clustering, gather=False)
        gpq = g.ProductQuantizer.apply(gv.residuals, cfg)
        grp = g.WordIndex(gw.words, g.Index.grouped(gv, gpq, g.LimitGroups(a.limit)))
        measure("grouped", grp)
        grp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
