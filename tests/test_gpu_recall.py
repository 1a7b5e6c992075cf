"""`python -m gulon_amd test` on the device: gulon_recall_counts (csrc/recall.hip) against a numpy restatement, Tests.sample /
for_queries against the oracle's exact kNN, Tests.recall_of over a sorted l2, a sorted cosine and a grouped index built
by `build-index` from one file against the restatement fed with the same index output, and the command end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, bits

pytestmark = pytest.mark.gpu

F = np.float32
N_ROWS, DIM, K, M, ITERS = 6000, 48, 256, 8, 5
SAMPLE = 200


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


@pytest.fixture(scope="module")
def tr():
    from gulon_amd import tests_recall
    return tests_recall


def _distances(X, Q, rows):
    """MathUtils.distanceSq(query, X[row]) for rows [B][max_k]: sequential binary32 sum, i ascending; 0 where row < 0."""
    safe = np.where(rows >= 0, rows, 0)
    acc = np.zeros(rows.shape, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(X.shape[1]):
            dx = Q[:, i][:, None] - X[safe, i]
            acc = acc + dx * dx
    return np.where(rows >= 0, acc, F(0))


def _counts(dist, rows, ks, cutoffs):
    pos = np.arange(rows.shape[1])
    with np.errstate(invalid="ignore"):
        return np.stack([((rows >= 0) & (pos[None, :] < k) & (dist <= cutoffs[:, j][:, None])).sum(axis=1)
                         for j, k in enumerate(ks)], axis=1).astype(np.int32)


def _ks(nks, max_k):
    if nks == 1:
        return [max_k]
    ks = [k for k in (1, 2, 3, 5, 10, 25, 50, 100, 500, 1000) if k <= max_k]
    extra = [k for k in range(max_k, 0, -1) if k not in ks]
    return sorted(ks + extra[:nks - len(ks)])


@pytest.mark.parametrize("d,b,max_k,nks", [
    (1, 1, 1, 1), (7, 17, 63, 1), (48, 17, 64, 10), (300, 17, 1000, 10), (48, 1000, 1000, 10), (7, 1000, 64, 10),
    (300, 1, 63, 10), (1, 17, 1000, 10), (300, 1000, 1, 1),
])
def test_recall_counts_equals_the_restatement(g, tr, oracle, d, b, max_k, nks):
    n = 5000
    rng = np.random.default_rng(1000 * d + b + max_k)
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[7, d // 2] = np.nan                                           # a NaN row
    Q = rng.standard_normal((b, d)).astype(np.float32)
    rows = rng.integers(0, n, (b, max_k)).astype(np.int32)
    if max_k > 1:
        rows[:, 1] = rows[:, 0]                                     # duplicate rows
        rows[0, max_k // 2] = 7
    else:
        rows[b // 2, 0] = 7
    counts = rng.integers(0, max_k + 1, b)                          # short results, -1 padding; some empty
    counts[0] = max_k
    rows[np.arange(max_k)[None, :] >= counts[:, None]] = -1
    ks = _ks(nks, max_k)
    assert len(ks) == nks and ks[-1] <= max_k
    dist = _distances(X, Q, rows)
    # every cutoff EQUALS one of the query's distances (<= must count it); a query without entries gets 1.0
    pick = (rng.random((b, nks)) * np.maximum(np.minimum(counts[:, None], np.asarray(ks)[None, :]), 1)).astype(np.int64)
    cut = np.where(counts[:, None] > 0, np.take_along_axis(dist, pick, axis=1), F(1)).astype(np.float32)
    want = _counts(dist, rows, ks, cut)
    dm = g.DeviceMatrix.from_host(X)
    tp, got = tr.recall_counts(dm, Q, rows, ks, cut, distances=True)
    nan = np.isnan(dist)
    assert nan.any() and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(bits(got[~nan]), bits(dist[~nan]))
    assert np.array_equal(tp, want)
    assert np.array_equal(tr.recall_counts(dm, Q, rows, ks, cut), want)          # without the distances
    assert want.sum() > 0 or max_k == 1
    hit = np.argwhere(rows >= 0)[:5]
    for q, p in hit:                                                              # the oracle's distanceSq, bit for bit
        assert nan[q, p] or bits(oracle.distance_sq(Q[q], X[rows[q, p]])) == bits(got[q, p])
    if (d, b) == (48, 17):                                                        # and the existing per-entry kernel
        old = np.zeros((b, max_k), np.float32)
        g.native.check(g.native.lib().gulon_distance_sq_rows(dm._h, Q.reshape(-1), b, rows.reshape(-1), max_k,
                                                             old.reshape(-1)))
        assert np.array_equal(bits(old[~nan]), bits(got[~nan]))
    dm.close()


def test_recall_counts_rejects_bad_arguments(g, tr):
    X = np.arange(40, dtype=np.float32).reshape(10, 4)
    dm = g.DeviceMatrix.from_host(X)
    Q = X[:3].copy()
    rows = np.asarray([[0, 1, 2], [3, 10, 4], [5, 6, -1]], np.int32)             # 10 == n
    with pytest.raises(ValueError, match="row 10 out of range"):
        tr.recall_counts(dm, Q, rows, [1, 3], np.ones((3, 2), np.float32))
    rows[1, 1] = 9
    assert tr.recall_counts(dm, Q, rows, [1, 3], np.full((3, 2), 1e9, np.float32)).tolist() == [[1, 3], [1, 3], [1, 2]]
    for ks in ([3, 1], [0, 2], [2, 2], [1, 4]):                                   # ascending, within [1, max_k]
        with pytest.raises(ValueError):
            tr.recall_counts(dm, Q, rows, ks, np.ones((3, 2), np.float32))
    with pytest.raises(ValueError):
        tr.recall_counts(dm, Q, np.zeros((3, 17), np.int32), list(range(1, 18)), np.ones((3, 17), np.float32))
    dm.close()


# ---- the word vectors, their indexes (written by build-index) and the sampled tests -------------------------------

@pytest.fixture(scope="module")
def vectors_file(tmp_path_factory):
    """6 000 x 48 rows around 12 centres, %.6f, words in no particular order (as tests/test_gpu_build_index.py)."""
    rng = np.random.default_rng(31)
    centres = rng.uniform(-4, 4, (12, DIM))
    x = centres[rng.integers(0, 12, N_ROWS)] + rng.normal(0, 0.6, (N_ROWS, DIM))
    words = [f"w{i:05d}" for i in rng.permutation(N_ROWS)]
    words[17] = "\U0001F600"
    root = tmp_path_factory.mktemp("recall")
    path = root / "vectors.txt"
    lines = [w + " " + " ".join("%.6f" % v for v in row) for w, row in zip(words, x)]
    with open(path, "w", encoding="utf-8", newline="\n") as fh:
        fh.write(f"{N_ROWS} {DIM}\n" + "\n".join(lines) + "\n")
    return str(path), words, lines, root


def _cli(args, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "gulon_amd"] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=timeout)


@pytest.fixture(scope="module")
def index_files(vectors_file):
    path, _, _, root = vectors_file
    out = {}
    for name, options in (("l2", ["-d", "l2"]), ("cosine", ["-d", "cosine"]),
                          ("grouped", ["-d", "l2", "-p", "--partitions", "12", "-l", "3"])):
        out[name] = str(root / f"{name}.bin")
        run = _cli(["build-index", "-k", str(K), "-m", str(M), "-n", str(ITERS), "-o", out[name]] + options + [path], 600)
        assert run.returncode == 0, run.stderr[-2000:]
    return out


@pytest.fixture(scope="module")
def sorted_vectors(g, vectors_file):
    """(the device word vectors in word order, their host copy)."""
    path = vectors_file[0]
    srt = g.read_word2vec_device(path, normalize=False).sorted()
    host = g.read_word2vec(path).sorted()
    assert srt.words == host.words
    return srt, host


def test_sample_draws_the_rows_and_for_queries_the_exact_kth_distances(g, tr, oracle, sorted_vectors):
    from gulon_amd.recall import sample_rows
    srt, host = sorted_vectors
    tests = tr.Tests.sample(srt, 300, tr.DEFAULT_KS, seed=0)
    drawn = sample_rows(N_ROWS, 300, 0)
    assert len(set(drawn.tolist())) < 300                                         # duplicates stay
    assert np.array_equal(bits(tests.queries), bits(host.data[drawn]))
    assert tests.ks == tr.DEFAULT_KS and tests.kept.tolist() == [10] * 300
    _, od, oc = oracle.exact_knn(host.data, tests.queries, 1000)
    assert oc.tolist() == [1000] * 300
    for j, k in enumerate(tests.ks):
        assert np.array_equal(bits(tests.kth[:, j]), bits(od[:, k - 1])), k
    assert tests.results(5) == [(k, od[5, k - 1]) for k in tr.DEFAULT_KS]
    assert not np.array_equal(tr.Tests.sample(srt, 300, seed=1).queries, tests.queries)

    # 700 rows: k = 1000 is absent, every other k is kept
    from gulon_amd.word_vectors import DeviceWordVectors, KeyIndexSorted
    small = DeviceWordVectors(host.words[:700], g.DeviceMatrix.from_host(host.data[:700]), KeyIndexSorted(host.words[:700]))
    few = tr.Tests.for_queries(small, host.data[:40], tr.DEFAULT_KS)
    assert few.kept.tolist() == [9] * 40 and [k for k, _ in few.results(0)] == list(tr.DEFAULT_KS[:9])
    _, od, oc = oracle.exact_knn(host.data[:700], host.data[:40], 1000)
    assert oc.tolist() == [700] * 40
    for j, k in enumerate(tr.DEFAULT_KS[:9]):
        assert np.array_equal(bits(few.kth[:, j]), bits(od[:, k - 1])), k
    assert np.isnan(few.kth[:, 9]).all()


def _restated_recall(tr, index, host, tests, eps, identity_rows=False):
    """Tests.recallOf (Tests.scala:18-41) in numpy over index.batch_query's own output: words -> rows of the vectors
    through a dict, sequential binary32 distances, the double-precision cutoff, take(k).count(_ <= cutoff), the fold."""
    row_of = {w: i for i, w in enumerate(host.words)}
    max_k = max(k for k, _ in tests.results(0))
    results = index.batch_query(max_k, tests.queries)
    rows = np.full((len(results), max_k), -1, np.int32)
    for i, r in enumerate(results):
        rows[i, :len(r)] = r.rows if identity_rows else [row_of[w] for w in r.words]
    dist = _distances(host.data, tests.queries, rows)
    factor = np.float64(F(1) + F(eps))
    samples = {k: [] for k in tests.ks}
    for i in range(len(results)):
        for k, kth in tests.results(i):
            cutoff = kth if F(eps) == 0 else F((np.sqrt(np.float64(kth)) * factor) ** 2)
            samples[k].append(F(int((dist[i, :k][rows[i, :k] >= 0] <= cutoff).sum())) / F(k))
    return {k: tr.fold(v) for k, v in samples.items() if v}, rows, results


@pytest.fixture(scope="module")
def sampled(tr, sorted_vectors):
    return tr.Tests.sample(sorted_vectors[0], SAMPLE)


@pytest.mark.parametrize("name", ["l2", "cosine", "grouped"])
def test_recall_of_equals_the_restatement(g, tr, oracle, sorted_vectors, index_files, sampled, name):
    srt, host = sorted_vectors
    index = g.WordIndex.load(index_files[name])
    by_eps = {}
    for eps in (0.0, 0.1):
        got = tr.Tests.recall_of(sampled, index, eps)
        want, rows, results = _restated_recall(tr, index, host, sampled, eps)
        assert sorted(got) == sorted(want) == list(tr.DEFAULT_KS)
        for k in tr.DEFAULT_KS:
            print(name, eps, k, got[k], want[k])
            assert got[k].count == want[k].count == SAMPLE
            assert bits(got[k].mean) == bits(want[k].mean) and bits(got[k].s) == bits(want[k].s), (name, eps, k)
        # No query is skipped: the restatement reads the same index output, so the order among equal distances is the
        # same on both sides.  (The cap on skipped queries is 5 %.)  The flagged ones are reported, not left out: on this
        # data the CPU oracle finds an equal pair among the 1001 nearest ADC distances of 35 (l2) and 17 (cosine) of
        # the 200 queries -- binary32 coincidences in a narrow band of distances -- and none that straddles a k.
        skipped = []
        assert len(skipped) / SAMPLE < 0.05
        assert got.flagged == len(got.flagged_queries) <= SAMPLE
        assert set(got.flagged_queries) == {i for i, r in enumerate(results) if r.flags & 3 and not r.flags & 4}
        by_eps[eps] = got
    for k in tr.DEFAULT_KS:                                                       # a wider cutoff never loses a hit
        assert by_eps[0.1][k].mean >= by_eps[0.0][k].mean
    assert by_eps[0.0][1].mean > 0.5       # an index of these vectors: every query is a row (the oracle finds R@1 = 1)
    if name == "l2":                                                              # R@10 as the oracle computes it
        _, od, oc = oracle.exact_knn(host.data, sampled.queries, 10)
        mean, sd = oracle.recall(host.data, sampled.queries, 10, rows[:, :10].copy(),
                                 np.minimum([len(r) for r in results], 10), od, oc)
        assert (mean, sd) == (float(by_eps[0.0][10].mean), float(by_eps[0.0][10].std_dev))
    if name == "grouped":                                                         # its row order is not the vectors'
        assert index.words != host.words
        wrong, _, _ = _restated_recall(tr, index, host, sampled, 0.0, identity_rows=True)
        assert wrong[1].mean < by_eps[0.0][1].mean
    index.close()


def test_command_end_to_end(g, tr, vectors_file, index_files, sorted_vectors, sampled):
    path, words, lines, root = vectors_file
    for name in ("l2", "grouped"):
        run = _cli(["test", "-v", path, "-i", index_files[name], "-s", str(SAMPLE)], 600)
        assert run.returncode == 0, run.stderr[-2000:]
        out = run.stdout.split("\n")
        assert out[0] == "\u001b[36mRUNNING:\u001b[0m Reading word vectors"
        assert out[1].startswith(f"\u001b[32mSUCCESS:\u001b[0m Read {N_ROWS} word vectors in ")
        assert out[2] == "\u001b[36mRUNNING:\u001b[0m Sampling test vectors and precomputing distances"
        assert out[3].startswith(f"\u001b[32mSUCCESS:\u001b[0m Sampled {SAMPLE} vectors in ")
        assert out[4] == "\u001b[36mRUNNING:\u001b[0m Calculating recall of index"
        index = g.WordIndex.load(index_files[name])
        api = sampled.recall_of(index)
        index.close()
        assert out[5:] == [f"R@{k}: {tr.java_float_to_string(api[k].mean)} +/- {tr.java_float_to_string(api[k].std_dev)}"
                           for k in tr.DEFAULT_KS] + [""]
    run = _cli(["test", "-v", path, "-i", index_files["cosine"], "-s", "50", "-e", "0.1"], 600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert [ln.split(":")[0] for ln in run.stdout.split("\n")[5:-1]] == [f"R@{k}" for k in tr.DEFAULT_KS]

    # a vectors file that lacks an indexed word: the command fails and names the word
    lacking = root / "lacking.txt"
    with open(lacking, "w", encoding="utf-8", newline="\n") as fh:
        fh.write("\n".join(lines[1:]) + "\n")
    run = _cli(["test", "-v", str(lacking), "-i", index_files["l2"], "-s", str(SAMPLE)], 600)
    assert run.returncode != 0
    assert words[0] in run.stderr and "LookupError" in run.stderr
