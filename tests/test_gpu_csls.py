"""CSLS translation (gulon_amd/csls.py, csrc/offset.hip): the mean-similarity reduction, the r_S pass, the
dictionary evaluation and the `translate` command, all bit for bit against the numpy restatement.

The pair of spaces: 600 unit target vectors in 32 dimensions around a common component, ten of them pulled towards it so
that they are near everything (hubs), and a source that is a permuted, lightly perturbed copy -- source word i translates to target word
PERM[i]."""
import io

import numpy as np
import pytest

from conftest import bits
from offset_ref import distances_by_row

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


@pytest.fixture(scope="module")
def spaces(g):
    rng = np.random.default_rng(2018)
    centre = rng.standard_normal(D)
    centre /= np.linalg.norm(centre)
    T = unit(rng.standard_normal((N, D)) / np.sqrt(D) + 0.7 * centre)    # a cloud with a common component
    for h in HUBS:                                               # towards the middle of the cloud: near every row
        T[h] = 0.3 * T[h] + centre
    T = unit(T)
    perm = rng.permutation(N)                                    # source word i <-> target word perm[i]
    S = unit(T[perm] + 0.1 * rng.standard_normal((N, D)))
    tdm, sdm = g.DeviceMatrix.from_host(T), g.DeviceMatrix.from_host(S)
    exact = g.ExactWordIndex(T_WORDS, g.ExactIndex(tdm, "cosine"))
    pq = g.ProductQuantizer.apply(tdm, g.ProductQuantizerConfig(256, 8, 2))
    flat = g.WordIndex(T_WORDS, g.Index.sorted(tdm, pq, "cosine"))
    source = g.ExactWordIndex(S_WORDS, g.ExactIndex(sdm, "cosine"))
    as_given = g.ExactIndex(sdm, "l2")                           # the same rows, queries taken as they are
    yield {"T": T, "S": S, "perm": perm, "exact": exact, "flat": flat, "source": source, "as_given": as_given,
           "tdm": tdm, "sdm": sdm}
    for ix in (exact, flat, source):
        ix.close()
    as_given.close()
    tdm.close()
    sdm.close()


def dictionary(perm):
    """Every third source word, some with a second gold translation, and four pairs with an absent word."""
    pairs = []
    for i in range(0, N, 3):
        pairs.append((S_WORDS[i], T_WORDS[perm[i]]))
        if i % 9 == 0:
            pairs.append((S_WORDS[i], T_WORDS[perm[(i + 1) % N]]))
    pairs += [("absent", "t001"), ("s001", "absent"), ("s002", "nowhere"), ("ghost", "t002")]
    return pairs


# ---- the reduction --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", (1, 10, 12, 20))
def test_mean_similarity_matches_the_reference(g, K):
    rng = np.random.default_rng(K)
    b, kin = 1000, 12
    dist = np.sort(rng.random((b, kin)).astype(np.float32) * np.float32(2.5), axis=1)
    counts = (np.arange(b) % (kin + 1)).astype(np.int32)         # 0 .. 12
    for c in (counts, None):
        got = g.mean_similarity(dist, c, K)
        want = g.mean_similarity_reference(dist, c, K)
        assert np.array_equal(bits(got), bits(want))
    assert (g.mean_similarity(dist, counts, K)[counts == 0] == 0).all()
    with pytest.raises(ValueError):
        g.mean_similarity(dist, counts, 0)


# ---- the r_S pass ------------------------------------------------------------------------------------------------------------

def reference_offsets(g, sp, target):
    """r_S by the host calls: the target's own compose of every row, the source's ordinary query of those vectors as
    they are, mean_similarity_reference."""
    rows = target.index.compose_rows([[(r, 1.0)] for r in range(N)])
    _, od, oc, _ = sp["as_given"].batch_query_raw(K_CSLS, rows)
    return g.mean_similarity_reference(od, oc, K_CSLS)


@pytest.mark.parametrize("kind", ("exact", "flat"))
def test_csls_offsets_match_the_reference(g, spaces, kind):
    target = spaces[kind]
    dev = g.csls_offsets(target, spaces["source"], K_CSLS)
    try:
        got = dev.numpy()
    finally:
        dev.free()
    want = reference_offsets(g, spaces, target)
    assert got.shape == (N,) and np.array_equal(bits(got), bits(want))
    hubs = np.zeros(N, bool)
    hubs[list(HUBS)] = True
    assert got[hubs].min() > np.percentile(got[~hubs], 90)       # the hubs are what the offsets single out


def test_csls_offsets_of_a_range_handle_and_bad_pairs(g, spaces):
    ranged = g.ExactIndex(spaces["tdm"], "cosine", 100, 333)
    try:
        dev = g.csls_offsets(ranged, spaces["source"], K_CSLS)
        got = dev.numpy()
        dev.free()
        want = reference_offsets(g, spaces, spaces["exact"])
        assert np.array_equal(bits(got[100:333]), bits(want[100:333]))
        assert np.isposinf(got[:100]).all() and np.isposinf(got[333:]).all()
    finally:
        ranged.close()
    l2 = g.ExactIndex(spaces["tdm"], "l2")
    other = g.DeviceMatrix.from_host(np.ones((4, D + 1), np.float32))
    narrow = g.ExactIndex(other, "cosine")
    try:
        with pytest.raises(ValueError, match="cosine"):
            g.csls_offsets(l2, spaces["source"])
        with pytest.raises(ValueError, match="dimensions"):
            g.csls_offsets(spaces["exact"], narrow)
        with pytest.raises(ValueError, match="dimensions"):
            g.evaluate_dictionary(spaces["exact"], g.ExactWordIndex(list("abcd"), narrow), [])
        with pytest.raises(ValueError, match="cosine"):
            g.evaluate_dictionary(g.ExactWordIndex(T_WORDS, l2), spaces["source"], [], method="csls")
        with pytest.raises(ValueError, match="method"):
            g.evaluate_dictionary(spaces["exact"], spaces["source"], [], method="mnn")
    finally:
        l2.close()
        narrow.close()
        other.close()


# ---- the evaluation ----------------------------------------------------------------------------------------------------------

def numpy_pipeline(g, sp, kind, method):
    """-> (source rows asked, their lists [b][10], the report's numbers) without csls.py's evaluation: the distances of
    every asked source vector to every target row by the target's ordinary query at k = n, the reference offsets, the
    reference order, and a count of the lists."""
    target, source, perm = sp[kind], sp["source"], sp["perm"]
    gold, skipped = {}, 0
    for s, t in dictionary(perm):
        if s in S_WORDS and t in T_WORDS:
            gold.setdefault(S_WORDS.index(s), set()).add(T_WORDS.index(t))
        else:
            skipped += 1
    rows = list(gold)
    vectors = sp["S"][rows]
    if method == "nn" and kind == "flat":                        # the index's own order is the definition, ties and all
        lists = target.batch_query_raw(KS[-1], vectors)[0]
    else:
        if kind == "exact":                                      # (the exact index prepares its queries itself)
            raw = target.index.batch_query_raw(N, vectors)
        else:
            raw = target.index.vector_index.batch_query_raw(N, target.index._prepare(vectors))
        dist = distances_by_row(raw, np.arange(N))
        offsets = reference_offsets(g, sp, target) if method == "csls" else np.zeros(N, np.float32)
        lists = g.offset_query_reference(dist, offsets, KS[-1])[0]
    hits = {k: sum(bool(gold[r] & set(lists[i, :k].tolist())) for i, r in enumerate(rows)) for k in KS}
    return rows, lists, (len(rows), skipped, hits)


@pytest.mark.parametrize("method", ("nn", "csls"))
@pytest.mark.parametrize("kind", ("exact", "flat"))
def test_evaluate_dictionary_matches_the_numpy_pipeline(g, spaces, kind, method):
    from gulon_amd.csls import translation_lists
    target, source = spaces[kind], spaces["source"]
    rows, lists, (asked, skipped, hits) = numpy_pipeline(g, spaces, kind, method)
    report = g.evaluate_dictionary(target, source, dictionary(spaces["perm"]), KS, method, K_CSLS)
    print(f"{kind} {method}: {report.line()}")
    assert (report.asked, report.skipped, report.hits) == (asked, skipped, hits)
    assert asked == 200 and skipped == 4 and report.ks == KS and report.method == method
    offsets = g.csls_offsets(target, source, K_CSLS) if method == "csls" else None
    try:
        got = translation_lists(target, source, rows, KS[-1], method, offsets)
    finally:
        if offsets is not None:
            offsets.free()
    assert np.array_equal(got[0], lists) and (got[2] == KS[-1]).all()


def test_translate_words_and_scores(g, spaces):
    target, source = spaces["exact"], spaces["source"]
    words = ["s000", "nobody", "s007"]
    nn = g.translate_words(target, source, words, 5)
    csls = g.translate_words(target, source, words, 5, "csls", K_CSLS)
    assert nn[1] is None and csls[1] is None
    for got, method in ((nn, "nn"), (csls, "csls")):
        for r in (got[0], got[2]):
            assert len(r.words) == 5 and r.words == [T_WORDS[i] for i in r.rows.tolist()]
            assert (np.diff(r.distances) >= 0).all()
    # the keys of a CSLS answer are distance + r_S of the row
    offsets = reference_offsets(g, spaces, target)
    dist = distances_by_row(target.index.batch_query_raw(N, spaces["S"][[0]]), np.arange(N))[0]
    r = csls[0]
    assert np.array_equal(bits(r.distances), bits((dist[r.rows] + offsets[r.rows]).astype(np.float32)))
    scores = g.translation_scores(r.distances, np.float32(0.25))
    assert scores.dtype == np.float32 and (np.diff(scores) <= 0).all()
    assert bits(scores[0]) == bits(np.float32(np.float32(2) - r.distances[0]) - np.float32(0.25))


# ---- the command -------------------------------------------------------------------------------------------------------------

def test_the_command_end_to_end(g, spaces, tmp_path):
    from gulon_amd import cli
    from gulon_amd.index_file import dump_index
    paths = {n: str(tmp_path / n) for n in ("target.idx", "target.txt", "source.txt", "words.txt", "dict.txt")}
    with open(paths["target.idx"], "wb") as fh:
        fh.write(dump_index(spaces["flat"].index, T_WORDS))
    for name, words, X in (("target.txt", T_WORDS, spaces["T"]), ("source.txt", S_WORDS, spaces["S"])):
        with open(paths[name], "w") as fh:
            fh.write(f"{N} {D}\n")
            for w, row in zip(words, X):
                fh.write(w + " " + " ".join(repr(float(x)) for x in row) + "\n")
    asked = ["s003", "S010", "missing", "s599"]
    with open(paths["words.txt"], "w") as fh:
        fh.write("\n".join(asked) + "\n")
    pairs = dictionary(spaces["perm"])
    with open(paths["dict.txt"], "w") as fh:
        fh.write("".join(f"{s}\t{t}\n" for s, t in pairs))

    def run(extra):
        out = io.BytesIO()
        assert cli.main(["translate", "-i", paths["target.idx"], "-s", paths["source.txt"]] + extra, stdout=out) == 0
        return out.getvalue().decode("utf-8").splitlines()

    # the objects the command builds: the loaded index, the source as read (normalised on the device)
    loaded = g.WordIndex.load(paths["target.idx"])
    vectors = cli.read_originals(paths["source.txt"], True)
    source = g.ExactWordIndex(vectors.words, g.ExactIndex(vectors.matrix, "cosine"), vectors.key_index)
    try:
        for method in ("nn", "csls"):
            lines = run(["--method", method, "-k", "4", "--lowercase", paths["words.txt"]])
            want = g.translate_words(loaded, source, [w.lower() for w in asked], 4, method, K_CSLS)
            assert lines == [f"{w}: not found" if r is None else f"{w}: {','.join(r.words)}" for w, r in zip(asked, want)]
            assert lines[2] == "missing: not found" and all(len(l.split(": ")[1].split(",")) == 4 for l in lines[:2])
            report = run(["--method", method, "-e", paths["dict.txt"]])
            assert report == g.evaluate_dictionary(loaded, source, pairs, KS, method, K_CSLS).lines()
            assert len(report) == 1 and report[0].startswith(f"{method}: @1 ") and report[0].endswith("(n = 200, skipped 4)")
        assert run(["--method", "csls", "-n", "3", "-k", "1,2", "-e", paths["dict.txt"]]) \
            == g.evaluate_dictionary(loaded, source, pairs, (1, 2), "csls", 3).lines()
        assert run([paths["words.txt"]])[1] == "S010: not found"                 # without --lowercase
        exact = run(["--method", "csls", "-v", paths["target.txt"], "--exact", "-e", paths["dict.txt"]])
        assert exact[0].startswith("csls: @1 ") and exact[0].endswith("(n = 200, skipped 4)")
    finally:
        source.close()
        loaded.close()
    # -R: an index built over rotated target vectors meets source vectors rotated after they are read
    from gulon_amd.rotation import Rotation
    rotation = Rotation(np.linalg.qr(np.random.default_rng(5).standard_normal((D, D)))[0])
    rotation.save(str(tmp_path / "target.rot"))
    rotated = rotation.apply_device(spaces["tdm"])
    pq = g.ProductQuantizer.apply(rotated, g.ProductQuantizerConfig(256, 8, 2))
    index = g.Index.sorted(rotated, pq, "cosine")
    try:
        with open(paths["target.idx"], "wb") as fh:
            fh.write(dump_index(index, T_WORDS))
    finally:
        index.vector_index.close()
        rotated.close()

    def at_ten(line):
        return float(line.split("@10 ")[1].split()[0])
    # a rotation keeps every distance, so with -R the precision is that of the unrotated pair (about 1 here); without it
    # the source points somewhere else and 10 answers out of 600 rows hit by chance
    for method in ("nn", "csls"):
        with_r = run(["--method", method, "-R", str(tmp_path / "target.rot"), "-e", paths["dict.txt"]])
        without = run(["--method", method, "-e", paths["dict.txt"]])
        assert at_ten(with_r[0]) > 0.9 > 0.5 > at_ten(without[0]), (with_r, without)

    out = io.BytesIO()                                           # a source of another dimension: reported, exit code 1
    with open(paths["source.txt"], "w") as fh:
        fh.write("2 3\na 1 0 0\nb 0 1 0\n")
    assert cli.main(["translate", "-i", paths["target.idx"], "-s", paths["source.txt"], paths["words.txt"]],
                    stdout=out) == 1
