"""Dictionary evaluation by ranks (gulon_amd/ranks.py, csrc/rank.hip) and `translate -e --ranks`.

The pair of spaces is test_gpu_csls.py's: 600 unit target vectors in 32 dimensions around a common component, ten of
them hubs, and a source that is a permuted, lightly perturbed copy -- source word i translates to target word PERM[i]."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, K_CSLS = 600, 32, 10
HUBS = range(40, 50)
T_WORDS = [f"t{i:03d}" for i in range(N)]
S_WORDS = [f"s{i:03d}" for i in range(N)]
KS = (1, 5, 10)


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def dictionary(perm):
    """Every third source word, some with a second gold translation, and four pairs with an absent word."""
    pairs = []
    for i in range(0, N, 3):
        pairs.append((S_WORDS[i], T_WORDS[perm[i]]))
        if i % 9 == 0:
            pairs.append((S_WORDS[i], T_WORDS[perm[(i + 1) % N]]))
    pairs += [("absent", "t001"), ("s001", "absent"), ("s002", "nowhere"), ("ghost", "t002")]
    return pairs


@pytest.fixture(scope="module")
def spaces(g, tmp_path_factory):
    from gulon_amd.index_file import dump_index
    root = tmp_path_factory.mktemp("rank_translate")
    rng = np.random.default_rng(2018)
    centre = rng.standard_normal(D)
    centre /= np.linalg.norm(centre)
    T = unit(rng.standard_normal((N, D)) / np.sqrt(D) + 0.7 * centre)
    for h in HUBS:
        T[h] = 0.3 * T[h] + centre
    T = unit(T)
    perm = rng.permutation(N)
    S = unit(T[perm] + 0.1 * rng.standard_normal((N, D)))
    tdm, sdm = g.DeviceMatrix.from_host(T), g.DeviceMatrix.from_host(S)
    exact = g.ExactWordIndex(T_WORDS, g.ExactIndex(tdm, "cosine"))
    pq = g.ProductQuantizer.apply(tdm, g.ProductQuantizerConfig(256, 8, 2))
    flat = g.WordIndex(T_WORDS, g.Index.sorted(tdm, pq, "cosine"))
    source = g.ExactWordIndex(S_WORDS, g.ExactIndex(sdm, "cosine"))
    paths = {n: str(root / n) for n in ("target.idx", "grouped.idx", "target.txt", "source.txt", "dict.txt")}
    with open(paths["target.idx"], "wb") as fh:
        fh.write(dump_index(flat.index, T_WORDS))
    for name, words, X in (("target.txt", T_WORDS, T), ("source.txt", S_WORDS, S)):
        with open(paths[name], "w") as fh:
            fh.write(f"{N} {D}\n")
            for w, row in zip(words, X):
                fh.write(w + " " + " ".join(repr(float(x)) for x in row) + "\n")
    pairs = dictionary(perm)
    with open(paths["dict.txt"], "w") as fh:
        fh.write("".join(f"{s}\t{t}\n" for s, t in pairs))
    yield {"exact": exact, "flat": flat, "source": source, "paths": paths, "pairs": pairs}
    for ix in (exact, flat, source):
        ix.close()
    tdm.close()
    sdm.close()


@pytest.mark.parametrize("kind", ("exact", "flat"))
def test_csls_hits_equal_those_of_the_lists_and_deeper_depths_are_answered(g, spaces, kind):
    target, source, pairs = spaces[kind], spaces["source"], spaces["pairs"]
    lists = g.evaluate_dictionary(target, source, pairs, KS, "csls", K_CSLS)
    report = g.evaluate_dictionary_ranks(target, source, pairs, KS + (64, 100, N), "csls", K_CSLS)
    assert (report.asked, report.skipped) == (lists.asked, lists.skipped) == (200, 4)
    assert {k: report.hits(k) for k in KS} == lists.hits
    assert report.unranked == 0 and report.hits(N) == 200        # every row is a candidate: the last depth holds all
    assert lists.hits[10] <= report.hits(64) <= report.hits(100) <= 200
    ranked = report.ranked
    assert report.mrr == pytest.approx(float(np.mean(1.0 / (ranked + 1.0))), rel=1e-12)
    assert report.median_rank == float(np.median(ranked + 1)) and 1.0 <= report.mean_rank <= N
    assert report.line().startswith("csls ranks: mrr ") and report.line().endswith("(n = 200, unranked 0, skipped 4)")
    for depth in (64, 100):                                      # past an offset query's list
        with pytest.raises(NotImplementedError, match="k_nn"):
            g.evaluate_dictionary(target, source, pairs, (1, depth), "csls", K_CSLS)


def test_nn_ranks_on_the_exact_target_are_positions_in_its_ordinary_answer(g, spaces):
    """(distance, row) with no offsets: where no two rows are equally far from a query, the position in batch_query."""
    target, source, pairs = spaces["exact"], spaces["source"], spaces["pairs"]
    lists = g.evaluate_dictionary(target, source, pairs, KS, "nn")
    report = g.evaluate_dictionary_ranks(target, source, pairs, KS, "nn")
    assert {k: report.hits(k) for k in KS} == lists.hits and report.unranked == 0


def test_the_command_prints_the_line_after_the_precision_line(g, spaces):
    from gulon_amd import cli
    paths, pairs = spaces["paths"], spaces["pairs"]

    def run(extra, status=0):
        out = io.BytesIO()
        assert cli.main(["translate", "-i", paths["target.idx"], "-s", paths["source.txt"], "-e", paths["dict.txt"]]
                        + extra, stdout=out) == status
        return out.getvalue().decode("utf-8").splitlines()

    loaded = g.WordIndex.load(paths["target.idx"])
    vectors = cli.read_originals(paths["source.txt"], True)
    source = g.ExactWordIndex(vectors.words, g.ExactIndex(vectors.matrix, "cosine"), vectors.key_index)
    try:
        for method in ("nn", "csls"):
            plain = run(["--method", method])
            ranked = run(["--method", method, "--ranks"])
            report = g.evaluate_dictionary_ranks(loaded, source, pairs, KS, method, K_CSLS)
            assert len(plain) == 1 and ranked == plain + [report.line()]         # the first line is today's, byte for byte
            assert ranked[1].startswith(f"{method} ranks: mrr ") and ranked[1].endswith("(n = 200, unranked 0, skipped 4)")
        deep = run(["--method", "csls", "--ranks", "-k", "1,64,100", "-n", "3"])
        report = g.evaluate_dictionary_ranks(loaded, source, pairs, (1, 64, 100), "csls", 3)
        assert deep[1] == report.line() and " @64 " in deep[0] and " @100 " in deep[1]
        assert deep[0] == ("csls: " + " ".join(f"@{k} {report.precision(k):.4f}" for k in (1, 64, 100))
                           + " (n = 200, skipped 4)")
        exact = run(["--method", "csls", "--ranks", "-v", paths["target.txt"], "--exact"])
        assert len(exact) == 2 and exact[1].startswith("csls ranks: mrr ")
    finally:
        source.close()
        loaded.close()


def test_a_grouped_target_is_refused_with_status_one(g, spaces, capsys):
    from gulon_amd import cli
    paths = spaces["paths"]
    assert cli.main(["build-index", "-d", "cosine", "-k", "256", "-m", "8", "-n", "2", "-p", "--partitions", "6", "-l", "3",
                     "-o", paths["grouped.idx"], paths["target.txt"]], stdout=io.BytesIO()) == 0
    capsys.readouterr()
    out = io.BytesIO()
    argv = ["translate", "-i", paths["grouped.idx"], "-s", paths["source.txt"], "-e", paths["dict.txt"], "--method", "csls"]
    assert cli.main(argv + ["--ranks"], stdout=out) == 1
    assert out.getvalue() == b"" and "error: rank queries are not supported by a grouped index" in capsys.readouterr().err
    assert cli.main(argv, stdout=out) == 0                       # without --ranks it answers as before
    assert out.getvalue().startswith(b"csls: @1 ")
    target = g.WordIndex.load(paths["grouped.idx"])
    try:
        with pytest.raises(NotImplementedError, match="grouped"):
            g.evaluate_dictionary_ranks(target, spaces["source"], spaces["pairs"], KS, "csls", K_CSLS)
        with pytest.raises(NotImplementedError, match="grouped"):
            target.index.batch_query_rank_raw(np.zeros((1, D), np.float32), [[0]])
    finally:
        target.close()
