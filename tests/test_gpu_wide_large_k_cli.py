"""The commands over an index built with `build-index -k 1024` (10-bit codes): `test` asks for 1000 neighbours,
`query-words -v` for 10 * k candidates -- both beyond the 63 of a wavefront list.  Tests.recall_of against a numpy
restatement fed with the index's own output, the `test` command end to end, and the refined query-words against
refine_topk over the index's own candidates."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, bits

pytestmark = pytest.mark.gpu

F = np.float32
N_ROWS, DIM, K, M, ITERS = 6000, 48, 1024, 8, 3
SAMPLE = 100


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


@pytest.fixture(scope="module")
def tr():
    from gulon_amd import tests_recall
    return tests_recall


def _cli(args, timeout, stdin=None):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "gulon_amd"] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=timeout, input=stdin)


@pytest.fixture(scope="module")
def vectors_file(tmp_path_factory):
    """6 000 x 48 rows around 12 centres, %.6f, words in no particular order."""
    rng = np.random.default_rng(31)
    centres = rng.uniform(-4, 4, (12, DIM))
    x = centres[rng.integers(0, 12, N_ROWS)] + rng.normal(0, 0.6, (N_ROWS, DIM))
    words = [f"w{i:05d}" for i in rng.permutation(N_ROWS)]
    root = tmp_path_factory.mktemp("wide_recall")
    path = root / "vectors.txt"
    lines = [w + " " + " ".join("%.6f" % v for v in row) for w, row in zip(words, x)]
    with open(path, "w", encoding="utf-8", newline="\n") as fh:
        fh.write(f"{N_ROWS} {DIM}\n" + "\n".join(lines) + "\n")
    return str(path), words, root


@pytest.fixture(scope="module")
def index_files(vectors_file):
    path, _, root = vectors_file
    out = {}
    for name, options in (("sorted", ["-d", "l2"]), ("grouped", ["-d", "l2", "-p", "--partitions", "12", "-l", "3"])):
        out[name] = str(root / f"{name}.bin")
        run = _cli(["build-index", "-k", str(K), "-m", str(M), "-n", str(ITERS), "-o", out[name]] + options + [path], 600)
        assert run.returncode == 0, run.stderr[-2000:]
    return out


@pytest.fixture(scope="module")
def sorted_vectors(g, vectors_file):
    path = vectors_file[0]
    srt = g.read_word2vec_device(path, normalize=False).sorted()
    host = g.read_word2vec(path).sorted()
    assert srt.words == host.words
    return srt, host


@pytest.fixture(scope="module")
def sampled(tr, sorted_vectors):
    return tr.Tests.sample(sorted_vectors[0], SAMPLE)


def _distances(X, Q, rows):
    """MathUtils.distanceSq(query, X[row]) for rows [B][max_k]: sequential binary32 sum, i ascending; 0 where row < 0."""
    safe = np.where(rows >= 0, rows, 0)
    acc = np.zeros(rows.shape, np.float32)
    for i in range(X.shape[1]):
        dx = Q[:, i][:, None] - X[safe, i]
        acc = acc + dx * dx
    return np.where(rows >= 0, acc, F(0))


def _restated_recall(tr, index, host, tests, eps):
    """Tests.recallOf (Tests.scala:18-41) in numpy over index.batch_query's own output."""
    row_of = {w: i for i, w in enumerate(host.words)}
    max_k = max(k for k, _ in tests.results(0))
    results = index.batch_query(max_k, tests.queries)
    rows = np.full((len(results), max_k), -1, np.int32)
    for i, r in enumerate(results):
        rows[i, :len(r)] = [row_of[w] for w in r.words]
    dist = _distances(host.data, tests.queries, rows)
    factor = np.float64(F(1) + F(eps))
    samples = {k: [] for k in tests.ks}
    for i in range(len(results)):
        for k, kth in tests.results(i):
            cutoff = kth if F(eps) == 0 else F((np.sqrt(np.float64(kth)) * factor) ** 2)
            samples[k].append(F(int((dist[i, :k][rows[i, :k] >= 0] <= cutoff).sum())) / F(k))
    return {k: tr.fold(v) for k, v in samples.items() if v}, results


@pytest.mark.parametrize("name", ["sorted", "grouped"])
def test_recall_of_a_wide_index_equals_the_restatement(g, tr, sorted_vectors, index_files, sampled, name):
    srt, host = sorted_vectors
    index = g.WordIndex.load(index_files[name])
    pq = index.index.quantizer if name == "grouped" else index.index.vector_index.product_quantizer
    assert pq.num_clusters == K                                               # 10-bit codes: the wide path
    by_eps = {}
    for eps in (0.0, 0.1):
        got = tr.Tests.recall_of(sampled, index, eps)
        want, results = _restated_recall(tr, index, host, sampled, eps)
        assert sorted(got) == sorted(want) == list(tr.DEFAULT_KS)
        assert all(len(r) == 1000 for r in results) or name == "grouped"
        for k in tr.DEFAULT_KS:
            print(name, eps, k, got[k], want[k])
            assert got[k].count == want[k].count == SAMPLE
            assert bits(got[k].mean) == bits(want[k].mean) and bits(got[k].s) == bits(want[k].s), (name, eps, k)
        by_eps[eps] = got
    for k in tr.DEFAULT_KS:                                                       # a wider cutoff never loses a hit
        assert by_eps[0.1][k].mean >= by_eps[0.0][k].mean
    assert by_eps[0.0][1].mean > 0.5
    index.close()


def test_the_test_command_on_wide_indexes(g, tr, vectors_file, index_files, sampled):
    path = vectors_file[0]
    for name in ("sorted", "grouped"):
        run = _cli(["test", "-v", path, "-i", index_files[name], "-s", str(SAMPLE)], 600)
        assert run.returncode == 0, run.stderr[-2000:]
        out = run.stdout.split("\n")
        assert out[4] == "\u001b[36mRUNNING:\u001b[0m Calculating recall of index"
        index = g.WordIndex.load(index_files[name])
        api = sampled.recall_of(index)
        index.close()
        assert out[5:] == [f"R@{k}: {tr.java_float_to_string(api[k].mean)} +/- {tr.java_float_to_string(api[k].std_dev)}"
                           for k in tr.DEFAULT_KS] + [""]
        assert len(tr.DEFAULT_KS) == 10 and max(tr.DEFAULT_KS) == 1000


@pytest.mark.parametrize("name", ["sorted", "grouped"])
def test_query_words_refined_over_a_wide_index(g, vectors_file, index_files, sorted_vectors, name):
    """`query-words -k 10 -v VECTORS` takes c = 100 candidates per word from the index (more than a wavefront list) and
    re-ranks them: the same words as refine_topk over the index's own 100 candidates."""
    path, words, _ = vectors_file
    srt, _ = sorted_vectors
    index = g.WordIndex.load(index_files[name])
    ask = [words[0], words[17], "absent", words[4000], words[-1]]
    row_map = np.asarray([srt.key_index.lookup(w) for w in index.words], np.int32)
    lines = []
    for w in ask:
        plain = index.query_by_word(100, w)
        if plain is None:
            lines.append(f"{w}: not found")
            continue
        assert len(plain.rows) == 100
        decoded = np.asarray(index.lookup(w), np.float32).reshape(1, -1)
        rows, dist, counts = g.refine_topk(srt.matrix, decoded, np.asarray(plain.rows, np.int32).reshape(1, -1), 10,
                                           row_map=row_map)
        assert counts[0] == 10
        lines.append(f"{w}: {','.join(index.words[i] for i in rows[0, :10].tolist())}")
    index.close()
    run = _cli(["query-words", "-i", index_files[name], "-k", "10", "-v", path], 600, stdin="\n".join(ask) + "\n")
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.split("\n") == lines + [""]
