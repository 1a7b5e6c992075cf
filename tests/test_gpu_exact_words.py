"""WordIndex.exact and `query-words --exact` over a sorted and a grouped index, l2 and cosine, built from one small
word2vec text: the exact index's row ids are the index's, its neighbours those of exact_nearest_neighbours over the
matched vectors, and a refined index fed every row as a candidate agrees with it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, bits

pytestmark = pytest.mark.gpu

N_WORDS, DIM, K = 1500, 16, 20
CONFIGS = [("sorted", "l2"), ("sorted", "cosine"), ("grouped", "l2"), ("grouped", "cosine")]


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    """the word2vec text: words in no particular order, clustered vectors of six decimals"""
    rng = np.random.default_rng(77)
    centres = rng.uniform(-3, 3, (5, DIM))
    x = centres[rng.integers(0, 5, N_WORDS)] + rng.normal(0, 1, (N_WORDS, DIM))
    names = [f"w{i:04d}" for i in rng.permutation(N_WORDS)]
    path = tmp_path_factory.mktemp("exact_words") / "vectors.txt"
    path.write_text(f"{N_WORDS} {DIM}\n" + "".join(w + " " + " ".join("%.6f" % v for v in row) + "\n"
                                                    for w, row in zip(names, x)))
    return str(path)


@pytest.fixture(scope="module")
def world(g, text):
    """(kind, metric) -> (WordIndex, the vectors sorted by word, their host copy)"""
    from gulon_amd.build import Partitioned, build_index
    from gulon_amd.product_quantizer import Config
    out = {}
    for kind, metric in CONFIGS:
        read = g.read_word2vec_device(text, normalize=metric == "cosine")
        part = Partitioned(6, 6) if kind == "grouped" else None      # every group searched: all rows are candidates
        words, index = build_index(read, metric, part, Config(32, 4, 3))
        vectors = read.sorted()
        out[kind, metric] = (g.WordIndex(words, index), vectors, vectors.matrix.to_host())
    return out


@pytest.mark.parametrize("kind,metric", CONFIGS)
def test_exact_word_index(g, world, kind, metric):
    index, vectors, V = world[kind, metric]
    exact = index.exact(vectors)
    assert (exact.size, exact.dimension, exact.metric, exact.words) == (N_WORDS, DIM, metric, index.words)
    row_of = {w: i for i, w in enumerate(vectors.words)}
    M = V[[row_of[w] for w in index.words]]                          # the vectors in the index's row order
    assert (kind == "grouped") == (index.words != vectors.words)
    asked = [index.words[7], "no such word", index.words[N_WORDS - 1], index.words[700]]
    got = exact.batch_query_by_words(K, asked)
    assert got[1] is None and exact.row_of("no such word") is None and exact.lookup("no such word") is None
    present = [(w, r) for w, r in zip(asked, got) if r is not None]
    rows = [index.row_of(w) for w, _ in present]
    assert rows == [exact.row_of(w) for w, _ in present]             # its row ids are the index's
    truth = g.exact_nearest_neighbours(M, M[rows], K)
    for (w, r), t, row in zip(present, truth, rows):
        assert r.words == [index.words[i] for i in t.rows.tolist()] and r.rows.tolist() == t.rows.tolist()
        assert np.array_equal(bits(r.distances), bits(t.distances)) and r.flags == t.flags
        assert r.words[0] == w and r.distances[0] == 0               # the word itself, as queryByWord gives it
        assert np.array_equal(bits(exact.lookup(w)), bits(M[row]))
        one = exact.query_by_word(K, w)
        assert one.words == r.words and np.array_equal(bits(one.distances), bits(r.distances))
    # by vector: the refined index with every row as a candidate sees the same distances
    Q = (M[[3, 500, 1499]] + np.float32(0.25)).astype(np.float32)
    by_vector = exact.batch_query(K, Q)
    assert exact.query(K, Q[1]).words == by_vector[1].words
    refined = index.refined(vectors, candidates=N_WORDS)
    for e, r in zip(by_vector, refined.batch_query(K, Q)):
        assert len(e) == K
        if e.flags == 0:
            assert set(e.words) == set(r.words) and np.array_equal(bits(e.distances), bits(r.distances))
    refined.close()
    exact.close()


def test_a_missing_word_is_a_lookup_error(g, world):
    from gulon_amd.word_vectors import DeviceWordVectors, KeyIndexSorted
    index, vectors, V = world["sorted", "l2"]
    fewer = DeviceWordVectors(vectors.words[1:], g.DeviceMatrix.from_host(V[1:]), KeyIndexSorted(vectors.words[1:]))
    with pytest.raises(LookupError, match="the index holds the word 'w0000', the word vectors do not"):
        index.exact(fewer)


@pytest.mark.parametrize("kind,metric", [("sorted", "l2"), ("grouped", "cosine")])
def test_cli_query_words_exact(g, world, text, tmp_path, kind, metric):
    from gulon_amd.index_file import dump_index
    index, vectors, _ = world[kind, metric]
    path = tmp_path / "words.index"
    path.write_bytes(dump_index(index.index, index.words))
    asked = [index.words[11], "not-a-word", index.words[900]]
    exact = index.exact(vectors)
    want = "".join(f"{w}: not found\n" if r is None else f"{w}: {','.join(r.words)}\n"
                   for w, r in zip(asked, exact.batch_query_by_words(5, asked))).encode()
    exact.close()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "gulon_amd", "query-words", "--exact", "-i", str(path), "-v", text, "-k", "5"],
                       input="\n".join(asked).encode(), capture_output=True, cwd=ROOT, env=env, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")
    assert p.stdout == want
