"""CSLS translation on a partitioned index (gulon_amd/csls.py, csrc/grouped_offset.hip): the r_S pass, the
dictionary evaluation, translate_words and the `translate` command against an index file built by `build-index -d cosine
-p`, bit for bit against a numpy pipeline over the handle's own distances.  The pair of spaces is test_gpu_csls.py's: 600
unit target vectors in 32 dimensions with ten hubs, and a permuted, lightly perturbed source."""
import io

import numpy as np
import pytest

from conftest import bits
from grouped_offset_ref import reference, scattered_distances

pytestmark = pytest.mark.gpu

N, D, K_CSLS = 600, 32, 10
HUBS = range(40, 50)
T_WORDS = [f"t{i:03d}" for i in range(N)]
S_WORDS = [f"s{i:03d}" for i in range(N)]
KS = (1, 5, 10)
BUILD = ["-d", "cosine", "-k", "256", "-m", "8", "-n", "2", "-p", "--partitions", "6"]


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
    from gulon_amd import cli
    root = tmp_path_factory.mktemp("grouped_csls")
    rng = np.random.default_rng(2018)
    centre = rng.standard_normal(D)
    centre /= np.linalg.norm(centre)
    T = unit(rng.standard_normal((N, D)) / np.sqrt(D) + 0.7 * centre)
    for h in HUBS:
        T[h] = 0.3 * T[h] + centre
    T = unit(T)
    perm = rng.permutation(N)
    S = unit(T[perm] + 0.1 * rng.standard_normal((N, D)))
    paths = {n: str(root / n) for n in ("target.idx", "rotated.idx", "target.rot", "target.txt", "source.txt", "words.txt",
                                        "dict.txt")}
    for name, words, X in (("target.txt", T_WORDS, T), ("source.txt", S_WORDS, S)):
        with open(paths[name], "w") as fh:
            fh.write(f"{N} {D}\n")
            for w, row in zip(words, X):
                fh.write(w + " " + " ".join(repr(float(x)) for x in row) + "\n")
    with open(paths["dict.txt"], "w") as fh:
        fh.write("".join(f"{s}\t{t}\n" for s, t in dictionary(perm)))
    assert cli.main(["build-index"] + BUILD + ["-l", "3", "-o", paths["target.idx"], paths["target.txt"]],
                    stdout=io.BytesIO()) == 0
    target = g.WordIndex.load(paths["target.idx"])
    assert isinstance(target.index, g.GroupedIndex) and target.metric == "cosine" and sorted(target.words) == T_WORDS
    vectors = cli.read_originals(paths["source.txt"], True)        # the source as the command reads it
    source = g.ExactWordIndex(vectors.words, g.ExactIndex(vectors.matrix, "cosine"), vectors.key_index)
    yield {"perm": perm, "target": target, "source": source, "paths": paths}
    target.close()
    source.close()


def reference_offsets(g, sp):
    """r_S by the host calls: GroupedIndex.lookup of every grouped row position, normalised; the source's ordinary query
    of those vectors (a cosine index: it normalises what it is given once more, as composing a one-term expression for a
    cosine index normalises the term and then the sum); mean_similarity_reference."""
    from gulon_amd.index import normalize
    rows = np.stack([normalize(r) for r in sp["target"].index.lookup_rows(np.arange(N))])
    _, od, oc, _ = sp["source"].index.batch_query_raw(K_CSLS, rows)
    return g.mean_similarity_reference(od, oc, K_CSLS)


def test_csls_offsets_match_the_reference(g, spaces):
    target = spaces["target"]
    dev = g.csls_offsets(target, spaces["source"], K_CSLS)
    try:
        got = dev.numpy()
    finally:
        dev.free()
    want = reference_offsets(g, spaces)
    assert got.shape == (N,) and np.array_equal(bits(got), bits(want))
    hubs = np.isin(np.asarray(target.words), [T_WORDS[h] for h in HUBS])
    assert got[hubs].min() > np.percentile(got[~hubs], 90)       # the hubs are what the offsets single out
    with pytest.raises(ValueError, match="exact index"):
        g.csls_offsets(target, target)                           # the source still must be exact


def numpy_pipeline(g, sp, method):
    """-> (source rows asked, their lists [b][10], the report's numbers) without csls.py's evaluation: the handle's own
    distances of every asked source vector (+inf outside its searched groups), the reference offsets, the reference
    order, and a count of the lists."""
    target, source = sp["target"], sp["source"]
    gold, skipped = {}, 0
    for s, t in dictionary(sp["perm"]):
        rs, rt = source.row_of(s), target.row_of(t)
        if rs is None or rt is None:
            skipped += 1
        else:
            gold.setdefault(int(rs), set()).add(int(rt))
    rows = list(gold)
    vectors = source.index.lookup_rows(np.asarray(rows, np.int32))
    if method == "nn":                                           # the index's own order is the definition, ties and all
        lists, _, counts, _ = target.batch_query_raw(KS[-1], vectors)
    else:
        dist = scattered_distances(target.index, vectors)
        assert np.isposinf(dist).any()                           # LimitGroups(3) of 6: some groups are not searched
        lists, _, counts = reference(g, dist, reference_offsets(g, sp), KS[-1])
    hits = {k: sum(bool(gold[r] & set(lists[i, :min(k, counts[i])].tolist())) for i, r in enumerate(rows)) for k in KS}
    return rows, lists, counts, (len(rows), skipped, hits)


@pytest.mark.parametrize("method", ("nn", "csls"))
def test_evaluate_dictionary_and_translate_words_match_the_numpy_pipeline(g, spaces, method):
    from gulon_amd.csls import translation_lists
    target, source = spaces["target"], spaces["source"]
    rows, lists, counts, (asked, skipped, hits) = numpy_pipeline(g, spaces, method)
    report = g.evaluate_dictionary(target, source, dictionary(spaces["perm"]), KS, method, K_CSLS)
    print(f"grouped {method}: {report.line()}")
    assert (report.asked, report.skipped, report.hits) == (asked, skipped, hits)
    assert asked == 200 and skipped == 4 and report.method == method and hits[10] > 100
    offsets = g.csls_offsets(target, source, K_CSLS) if method == "csls" else None
    try:
        got = translation_lists(target, source, rows, KS[-1], method, offsets)
        words = [source.words[r] for r in rows[:7]] + ["nobody"]
        translated = g.translate_words(target, source, words, KS[-1], method, K_CSLS, offsets)
    finally:
        if offsets is not None:
            offsets.free()
    assert np.array_equal(got[0], lists) and np.array_equal(got[2], counts)
    assert translated[-1] is None
    for i, r in enumerate(translated[:-1]):
        assert r.rows.tolist() == lists[i, :counts[i]].tolist() and r.words == [target.words[j] for j in r.rows.tolist()]
        assert (np.diff(r.distances) >= 0).all()


def test_the_command_on_a_partitioned_index(g, spaces):
    from gulon_amd import cli
    paths, target, source = spaces["paths"], spaces["target"], spaces["source"]
    asked = ["s003", "S010", "missing", "s599"]
    with open(paths["words.txt"], "w") as fh:
        fh.write("\n".join(asked) + "\n")
    pairs = dictionary(spaces["perm"])

    def run(index, extra):
        out = io.BytesIO()
        assert cli.main(["translate", "-i", index, "-s", paths["source.txt"]] + extra, stdout=out) == 0
        return out.getvalue().decode("utf-8").splitlines()

    for method in ("nn", "csls"):
        lines = run(paths["target.idx"], ["--method", method, "-k", "4", "--lowercase", paths["words.txt"]])
        want = g.translate_words(target, source, [w.lower() for w in asked], 4, method, K_CSLS)
        assert lines == [f"{w}: not found" if r is None else f"{w}: {','.join(r.words)}" for w, r in zip(asked, want)]
        assert lines[2] == "missing: not found" and all(len(l.split(": ")[1].split(",")) == 4 for l in lines[:2])
        report = run(paths["target.idx"], ["--method", method, "-e", paths["dict.txt"]])
        assert report == g.evaluate_dictionary(target, source, pairs, KS, method, K_CSLS).lines()
        assert len(report) == 1 and report[0].startswith(f"{method}: @1 ") and report[0].endswith("(n = 200, skipped 4)")


def test_a_partitioned_index_behind_a_rotation(g, spaces):
    """build-index -p -R learns a rotation and builds over the rotated vectors; translate -R rotates the source after it
    is read.  A rotation keeps every distance, so with -R the pair translates as the unrotated pair does; without it the
    source points somewhere else."""
    from gulon_amd import cli
    paths = spaces["paths"]
    assert cli.main(["build-index"] + BUILD + ["-l", "6", "-R", paths["target.rot"], "-o", paths["rotated.idx"],
                                               paths["target.txt"]], stdout=io.BytesIO()) == 0

    def at_ten(extra):
        out = io.BytesIO()
        assert cli.main(["translate", "-i", paths["rotated.idx"], "-s", paths["source.txt"], "-e", paths["dict.txt"]]
                        + extra, stdout=out) == 0
        line = out.getvalue().decode("utf-8").splitlines()[0]
        print(extra, line)
        return float(line.split("@10 ")[1].split()[0])

    for method in ("nn", "csls"):
        with_r, without = at_ten(["--method", method, "-R", paths["target.rot"]]), at_ten(["--method", method])
        assert with_r > 0.9 > 0.5 > without, (method, with_r, without)
