"""`python -m gulon_amd build-index` end to end (cli.run_build_index, build.build_index, the device ingest under them)
against the index assembled from the pieces that were there before it and are oracle-checked on their own:
read_word2vec -> .sorted() / .grouped() -> ProductQuantizer.apply -> Index.sorted / Index.grouped -> dump_index.
The written file must hold the same bytes; query-words over it must answer as WordIndex over the expected bytes."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

N_ROWS, DIM, K, M, ITERS = 6000, 48, 16, 8, 5


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


@pytest.fixture(scope="module")
def vectors_file(tmp_path_factory):
    """6 000 x 48 rows around 12 centres, %.6f, words in no particular order (some beyond the BMP)."""
    rng = np.random.default_rng(31)
    centres = rng.uniform(-4, 4, (12, DIM))
    x = centres[rng.integers(0, 12, N_ROWS)] + rng.normal(0, 0.6, (N_ROWS, DIM))
    words = [f"w{i:05d}" for i in rng.permutation(N_ROWS)]
    words[17], words[4000] = "\U0001F600", "￿"
    path = tmp_path_factory.mktemp("build_index") / "vectors.txt"
    with open(path, "w", encoding="utf-8", newline="\n") as fh:
        fh.write(f"{N_ROWS} {DIM}\n")
        for w, row in zip(words, x):
            fh.write(w + " " + " ".join("%.6f" % v for v in row) + "\n")
    return str(path), words


def _expected(g, path, metric, partitioned):
    from gulon_amd.index_file import dump_index
    cfg = g.ProductQuantizerConfig(K, M, ITERS)
    wv = g.read_word2vec(path, normalize=metric == "cosine")
    if partitioned is None:
        srt = wv.sorted()
        pq = g.ProductQuantizer.apply(srt.data, cfg)
        return dump_index(g.Index.sorted(srt.data, pq, metric), srt.words)
    partitions, limit = partitioned
    clustering = g.KMeans.compute_clusters(g.Vectors(g.Matrix(wv.data)), g.KMeansConfig(partitions, ITERS))
    gw, gv = wv.grouped(clustering)
    pq = g.ProductQuantizer.apply(gv.residuals, cfg)
    return dump_index(g.Index.grouped(gv, pq, g.LimitGroups(limit), metric), gw.words)


@pytest.mark.parametrize("name,metric,options,partitioned", [
    ("l2 linear", "l2", [], None),
    ("cosine linear", "cosine", [], None),
    ("l2 partitioned 12 / 3", "l2", ["-p", "--partitions", "12", "-l", "3"], (12, 3)),
    ("l2 partitioned, defaults", "l2", ["-p"], (N_ROWS // 1000, max(int(N_ROWS // 1000 * 0.05), 5))),
])
def test_build_index_writes_the_bytes_of_the_existing_pieces(g, vectors_file, tmp_path, name, metric, options,
                                                             partitioned):
    from gulon_amd import cli
    path, words = vectors_file
    out = str(tmp_path / "index.bin")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "gulon_amd", "build-index", "-d", metric, "-k", str(K), "-m", str(M),
                          "-n", str(ITERS), "-o", out] + options + [path],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-2000:]
    log = run.stdout
    assert f"Read {N_ROWS} word vectors in " in log and f"Built index for {N_ROWS} word vectors in " in log
    assert f"Wrote index to {out} in " in log and log.count("RUNNING:") == log.count("SUCCESS:")
    assert ("Computed" in log) == (partitioned is not None)
    if partitioned is not None:
        assert f"Computed {partitioned[0]} partitions in " in log
    want = _expected(g, path, metric, partitioned)
    with open(out, "rb") as fh:
        got = fh.read()
    assert len(got) == len(want)
    assert got == want
    # query-words over the written file = WordIndex over the expected bytes
    ask = [words[0], words[17], words[4000], "w00042", "absent", words[-1]]
    stdout = io.BytesIO()
    assert cli.main(["query-words", "-i", out, "-k", "5"], stdin=io.BytesIO("\n".join(ask).encode("utf-8")),
                    stdout=stdout) == 0
    ref = g.WordIndex.load(want)
    lines = [f"{w}: not found" if r is None else f"{w}: {','.join(r.words)}"
             for w, r in zip(ask, ref.batch_query_by_words(5, ask))]
    ref.close()
    assert stdout.getvalue().decode("utf-8").split("\n")[:-1] == lines
    assert lines[4] == "absent: not found" and lines[0].startswith(words[0] + ": ")
