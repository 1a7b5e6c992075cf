"""Inverted-softmax translation (gulon_amd/softmax.py, csls.py, ranks.py, csrc/logsumexp.hip): the offsets
pass against the handle's own log-sum-exp query and against the float64 reference, the lists, words, precision and ranks
against the numpy restatement over the handle's own distances and the device's offsets, the probabilities, a planted hub,
and the `translate` command.

The pair of spaces is test_gpu_csls.py's: 600 unit target vectors in 32 dimensions with ten hubs, and a permuted, lightly
perturbed source.  The targets: the exact index over the vectors, a flat byte-code index, and the partitioned index
`build-index -d cosine -p` writes (test_gpu_grouped_csls.py's build)."""
import io

import numpy as np
import pytest

from conftest import bits
from cosmul_ref import exact_distances
from grouped_offset_ref import scattered_distances
from offset_ref import distances_by_row

pytestmark = pytest.mark.gpu

N, D, K_CSLS, BETA = 600, 32, 10, 30.0
HUBS = range(40, 50)
T_WORDS = [f"t{i:03d}" for i in range(N)]
S_WORDS = [f"s{i:03d}" for i in range(N)]
KS = (1, 5, 10)
KINDS = ("exact", "flat", "grouped")
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
    from gulon_amd.index_file import dump_index
    root = tmp_path_factory.mktemp("isf")
    rng = np.random.default_rng(2018)
    centre = rng.standard_normal(D)
    centre /= np.linalg.norm(centre)
    T = unit(rng.standard_normal((N, D)) / np.sqrt(D) + 0.7 * centre)
    for h in HUBS:
        T[h] = 0.3 * T[h] + centre
    T = unit(T)
    perm = rng.permutation(N)
    S = unit(T[perm] + 0.1 * rng.standard_normal((N, D)))
    paths = {n: str(root / n) for n in ("flat.idx", "grouped.idx", "target.txt", "source.txt", "words.txt", "dict.txt")}
    for name, words, X in (("target.txt", T_WORDS, T), ("source.txt", S_WORDS, S)):
        with open(paths[name], "w") as fh:
            fh.write(f"{N} {D}\n")
            for w, row in zip(words, X):
                fh.write(w + " " + " ".join(repr(float(x)) for x in row) + "\n")
    with open(paths["dict.txt"], "w") as fh:
        fh.write("".join(f"{s}\t{t}\n" for s, t in dictionary(perm)))
    with open(paths["words.txt"], "w") as fh:
        fh.write("s003\nmissing\ns599\n")
    tdm = g.DeviceMatrix.from_host(T)
    exact = g.ExactWordIndex(T_WORDS, g.ExactIndex(tdm, "cosine"))
    pq = g.ProductQuantizer.apply(tdm, g.ProductQuantizerConfig(256, 8, 2))
    flat = g.WordIndex(T_WORDS, g.Index.sorted(tdm, pq, "cosine"))
    with open(paths["flat.idx"], "wb") as fh:
        fh.write(dump_index(flat.index, T_WORDS))
    assert cli.main(["build-index"] + BUILD + ["-l", "3", "-o", paths["grouped.idx"], paths["target.txt"]],
                    stdout=io.BytesIO()) == 0
    grouped = g.WordIndex.load(paths["grouped.idx"])
    assert isinstance(grouped.index, g.GroupedIndex) and grouped.metric == "cosine"
    vectors = cli.read_originals(paths["source.txt"], True)        # the source as the command reads it
    source = g.ExactWordIndex(vectors.words, g.ExactIndex(vectors.matrix, "cosine"), vectors.key_index)
    as_given = g.ExactIndex(vectors.matrix, "l2")                  # the same rows, queries taken as they are
    yield {"perm": perm, "exact": exact, "flat": flat, "grouped": grouped, "source": source, "as_given": as_given,
           "paths": paths, "tdm": tdm}
    for ix in (exact, flat, grouped, source):
        ix.close()
    as_given.close()
    tdm.close()


def composed_rows(target):
    """What the offsets pass composes: every target row as a one-term expression, by the target's own compose."""
    return target.index.compose_rows([[(r, 1.0)] for r in range(N)])


def device_offsets(g, sp, kind, beta=BETA, sources=None):
    dev = g.isf_offsets(sp[kind], sp["source"], beta, sources)
    try:
        return dev.numpy()
    finally:
        dev.free()


# ---- the offsets pass --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sources", (None, 200))
@pytest.mark.parametrize("kind", KINDS)
def test_isf_offsets_match_the_handle_and_the_reference(g, spaces, kind, sources):
    from gulon_amd.exact import normalize_rows
    target, source = spaces[kind], spaces["source"].index
    got = device_offsets(g, spaces, kind, BETA, sources)
    assert got.shape == (N,) and got.dtype == np.float32 and np.isfinite(got).all()
    rows = composed_rows(target)
    scan = source if sources is None else g.ExactIndex(source.matrix, "cosine", 0, sources)
    try:
        L, terms = scan.batch_query_logsumexp(rows, BETA)          # one batch of N, as the pass asks it
    finally:
        if scan is not source:
            scan.close()
    n_s = N if sources is None else sources
    assert (terms == n_s).all()
    assert np.array_equal(bits(got), bits(g.isf_offsets_from(L, terms, BETA)))
    # the float64 reference over distances restated in numpy: the source's rows as the device holds them
    dist = exact_distances(source.lookup_rows(np.arange(n_s)), normalize_rows(rows))
    want = (2.0 / BETA) * g.logsumexp_reference(dist, BETA)[0]
    err = np.abs(got.astype(np.float64) - want)
    bound = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + (2.0 / BETA) * 2.0 ** -40
    print(f"{kind} sources={sources}: largest error {err.max():.3g}, smallest bound {bound.min():.3g}")
    assert (err <= bound).all()
    if sources is None and kind == "exact":                      # the hubs are what the offsets single out
        hubs = np.isin(np.asarray(target.words), [T_WORDS[h] for h in HUBS])
        assert got[hubs].min() > np.percentile(got[~hubs], 90)


def test_isf_offsets_of_a_range_handle_and_bad_pairs(g, spaces):
    ranged = g.ExactIndex(spaces["tdm"], "cosine", 100, 333)
    l2 = g.ExactIndex(spaces["tdm"], "l2")
    try:
        dev = g.isf_offsets(ranged, spaces["source"], BETA)
        got = dev.numpy()
        dev.free()
        assert np.isposinf(got[:100]).all() and np.isposinf(got[333:]).all() and np.isfinite(got[100:333]).all()
        with pytest.raises(ValueError, match="cosine"):
            g.isf_offsets(l2, spaces["source"])
        with pytest.raises(ValueError, match="exact index"):
            g.isf_offsets(spaces["exact"], spaces["flat"])
        with pytest.raises(ValueError, match="beta"):
            g.isf_offsets(spaces["exact"], spaces["source"], 0.0)
        with pytest.raises(ValueError, match="sources"):
            g.isf_offsets(spaces["exact"], spaces["source"], BETA, N + 1)
        with pytest.raises(ValueError, match="beta too large for these distances"):
            g.isf_offsets(spaces["exact"], spaces["source"], 3e38)           # every term but a row's own twin underflows
    finally:
        ranged.close()
        l2.close()


def test_sources_as_rows(g, spaces):
    """An array of source rows sums over a gather of those rows in the order given: the first 200 in order are
    sources=200 bit for bit; another choice of 200 rows matches the float64 reference over those rows and differs."""
    from gulon_amd.exact import normalize_rows
    source = spaces["source"].index
    first = device_offsets(g, spaces, "exact", BETA, 200)
    assert np.array_equal(bits(device_offsets(g, spaces, "exact", BETA, np.arange(200))), bits(first))
    chosen = np.random.default_rng(5).permutation(N)[:200]
    got = device_offsets(g, spaces, "exact", BETA, chosen)
    assert not np.array_equal(bits(got), bits(first))
    dist = exact_distances(source.lookup_rows(chosen), normalize_rows(composed_rows(spaces["exact"])))
    want = (2.0 / BETA) * g.logsumexp_reference(dist, BETA)[0]
    bound = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + (2.0 / BETA) * 2.0 ** -40
    assert (np.abs(got.astype(np.float64) - want) <= bound).all()
    for bad in ([], [0, 0], [-1, 3], [N]):
        with pytest.raises(ValueError, match="sources"):
            g.isf_offsets(spaces["exact"], spaces["source"], BETA, np.asarray(bad, np.int64))


def csls_reference_offsets(g, sp, kind):
    """r_S as test_gpu_csls.py and test_gpu_grouped_csls.py restate it: the composed rows, the source's ordinary query of
    them as they are, mean_similarity_reference."""
    _, od, oc, _ = sp["as_given"].batch_query_raw(K_CSLS, composed_rows(sp[kind]))
    return g.mean_similarity_reference(od, oc, K_CSLS)


@pytest.mark.parametrize("kind", KINDS)
def test_csls_offsets_did_not_move(g, spaces, kind):
    dev = g.csls_offsets(spaces[kind], spaces["source"], K_CSLS)
    try:
        got = dev.numpy()
    finally:
        dev.free()
    assert got.shape == (N,) and np.array_equal(bits(got), bits(csls_reference_offsets(g, spaces, kind)))


# ---- lists, words, precision, ranks ----------------------------------------------------------------------------------------

def own_distances(sp, kind, vectors):
    """[b][N]: the handle's own distance of every vector to every target row, +inf where a grouped index does not look."""
    target = sp[kind]
    if kind == "exact":                                          # (the exact index prepares its queries itself)
        return distances_by_row(target.index.batch_query_raw(N, vectors), np.arange(N))
    if kind == "flat":
        return distances_by_row(target.index.vector_index.batch_query_raw(N, target.index._prepare(vectors)), np.arange(N))
    return scattered_distances(target.index, vectors)


def asked_rows(sp, kind):
    target, source = sp[kind], sp["source"]
    gold, skipped = {}, 0
    for s, t in dictionary(sp["perm"]):
        rs, rt = source.row_of(s), target.row_of(t)
        if rs is None or rt is None:
            skipped += 1
        else:
            gold.setdefault(int(rs), set()).add(int(rt))
    return list(gold), gold, skipped


@pytest.mark.parametrize("kind", KINDS)
def test_lists_words_and_precision_match_the_numpy_pipeline(g, spaces, kind):
    from gulon_amd.csls import translation_lists
    target, source = spaces[kind], spaces["source"]
    rows, gold, skipped = asked_rows(spaces, kind)
    vectors = source.index.lookup_rows(np.asarray(rows, np.int32))
    offsets = device_offsets(g, spaces, kind)
    want = g.offset_query_reference(own_distances(spaces, kind, vectors), offsets, KS[-1], rows=np.arange(N))
    dev = g.isf_offsets(target, source, BETA)
    try:
        got = translation_lists(target, source, rows, KS[-1], "isf", dev)
        words = [source.words[r] for r in rows[:7]] + ["nobody"]
        translated = g.translate_words(target, source, words, KS[-1], "isf", offsets=dev)
    finally:
        dev.free()
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    own = g.translate_words(target, source, words, KS[-1], "isf", beta=BETA)         # computes the offsets itself
    assert translated[-1] is None and own[-1] is None
    for i, (r, o) in enumerate(zip(translated[:-1], own[:-1])):
        c = want[2][i]
        assert r.rows.tolist() == want[0][i, :c].tolist() == o.rows.tolist()
        assert np.array_equal(bits(r.distances), bits(want[1][i, :c])) and np.array_equal(bits(o.distances), bits(r.distances))
        assert r.words == [target.words[j] for j in r.rows.tolist()]
    hits = {k: sum(bool(gold[r] & set(want[0][i, :min(k, want[2][i])].tolist())) for i, r in enumerate(rows)) for k in KS}
    report = g.evaluate_dictionary(target, source, dictionary(spaces["perm"]), KS, "isf", beta=BETA)
    print(f"{kind} isf: {report.line()}")
    assert (report.method, report.asked, report.skipped, report.hits) == ("isf", 200, 4, hits) and skipped == 4
    assert hits[10] > 100
    other = g.evaluate_dictionary(target, source, dictionary(spaces["perm"]), KS, "isf", beta=10.0, sources=200)
    assert other.asked == 200 and other.hits[10] > 100


@pytest.mark.parametrize("kind", ("exact", "flat"))
def test_ranks_agree_with_the_lists(g, spaces, kind):
    target, source, pairs = spaces[kind], spaces["source"], dictionary(spaces["perm"])
    by_ranks = g.evaluate_dictionary_ranks(target, source, pairs, (1, 100), "isf", beta=BETA, sources=300)
    assert by_ranks.method == "isf" and by_ranks.asked == 200 and by_ranks.skipped == 4 and by_ranks.unranked == 0
    for first in range(1, 64, 16):                               # every depth a list reaches, 16 depths to a report
        depths = tuple(range(first, min(first + 16, 64)))
        by_lists = g.evaluate_dictionary(target, source, pairs, depths, "isf", beta=BETA, sources=300)
        assert {k: by_ranks.hits(k) for k in depths} == by_lists.hits
    assert by_ranks.line().startswith("isf ranks: mrr ")


def test_ranks_on_a_grouped_target_stay_refused(g, spaces):
    with pytest.raises(NotImplementedError, match="grouped"):
        g.evaluate_dictionary_ranks(spaces["grouped"], spaces["source"], dictionary(spaces["perm"]), KS, "isf")


def test_probabilities_sum_to_one_over_the_sources(g, spaces):
    target, source = spaces["exact"], spaces["source"]
    offsets = device_offsets(g, spaces, "exact")
    dist = own_distances(spaces, "exact", source.index.lookup_rows(np.arange(N)))    # [sources][targets]
    keys = (dist + offsets[None, :]).astype(np.float32)          # the keys an offset query forms
    got = target.batch_query_offset_raw(5, source.index.lookup_rows(np.arange(8)), offsets)
    for q in range(8):
        assert np.array_equal(bits(got[1][q]), bits(keys[q, got[0][q]]))
    total = g.isf_probabilities(keys, BETA).sum(axis=0)
    print(f"largest |sum - 1| = {np.abs(total - 1).max():.3g}")
    assert (np.abs(total - 1) <= N * 2.0 ** -20).all()


# ---- a planted hub -----------------------------------------------------------------------------------------------------------

def test_a_planted_hub_beats_nn_and_not_isf(g):
    """300 random unit target rows in 32 dimensions; source word i is target row i but for a little noise, and source
    words 1 .. 60 are tilted towards target row 0, the hub, so far that the hub is nearer to them than their own row.
    The hub's normaliser then carries 60 large terms, a gold row's one: log 60 * 2 / beta = 0.27 in distance, against a
    lead of the hub of about 0.07.  The margins were chosen in float64 first and are asserted before the outcome."""
    n, d, tilted, beta = 300, 32, np.arange(1, 61), 30.0
    rng = np.random.default_rng(7)
    T = rng.standard_normal((n, d))
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    S = T.copy()
    S[tilted] = 0.7 * T[tilted] + 0.8 * T[0]
    S += 0.02 * rng.standard_normal((n, d))
    T, S = unit(T), unit(S)
    T64, S64 = T.astype(np.float64), S.astype(np.float64)
    dist = ((S64[:, None, :] - T64[None, :, :]) ** 2).sum(axis=2)                    # [sources][targets]
    keys = dist + (2 / beta) * np.log(np.exp(-(beta / 2) * dist).sum(axis=0))[None, :]
    gold = np.arange(n)
    assert (dist[tilted, tilted] - dist[tilted, 0]).min() > 0.05                     # nn: the hub leads every tilted word
    rest = dist.copy()
    rest[gold, gold] = np.inf
    assert np.delete(rest.min(axis=1) - dist[gold, gold], tilted).min() > 0.5       # ... and no other word loses its row
    rest = keys.copy()
    rest[gold, gold] = np.inf
    assert (rest.min(axis=1) - keys[gold, gold]).min() > 0.05                        # isf: every gold row leads

    words_t, words_s = [f"t{i}" for i in range(n)], [f"s{i}" for i in range(n)]
    tdm, sdm = g.DeviceMatrix.from_host(T), g.DeviceMatrix.from_host(S)
    target = g.ExactWordIndex(words_t, g.ExactIndex(tdm, "cosine"))
    source = g.ExactWordIndex(words_s, g.ExactIndex(sdm, "cosine"))
    try:
        pairs = list(zip(words_s, words_t))
        nn = g.evaluate_dictionary(target, source, pairs, (1,), "nn")
        isf = g.evaluate_dictionary(target, source, pairs, (1,), "isf", beta=beta)
        assert nn.asked == isf.asked == n
        assert nn.hits[1] == n - len(tilted) and isf.hits[1] == n
        first = g.translate_words(target, source, ["s1", "s60", "s61"], 1, "nn")
        assert [r.words for r in first] == [["t0"], ["t0"], ["t61"]]
    finally:
        target.close()
        source.close()
        tdm.close()
        sdm.close()


# ---- the command -------------------------------------------------------------------------------------------------------------

def test_the_command(g, spaces):
    from gulon_amd import cli
    paths, source, pairs = spaces["paths"], spaces["source"], dictionary(spaces["perm"])
    asked = ["s003", "missing", "s599"]

    def run(index, extra, status=0):
        out = io.BytesIO()
        assert cli.main(["translate", "-i", paths[index], "-s", paths["source.txt"], "--method", "isf"] + extra,
                        stdout=out) == status
        return out.getvalue().decode("utf-8").splitlines()

    for index, kind in (("flat.idx", "flat"), ("grouped.idx", "grouped")):
        target = spaces[kind]
        lines = run(index, ["-k", "4", paths["words.txt"]])
        want = g.translate_words(target, source, asked, 4, "isf")
        assert lines == [f"{w}: not found" if r is None else f"{w}: {','.join(r.words)}" for w, r in zip(asked, want)]
        assert lines[1] == "missing: not found" and len(lines[0].split(": ")[1].split(",")) == 4
        report = run(index, ["-e", paths["dict.txt"]])
        assert report == g.evaluate_dictionary(target, source, pairs, KS, "isf").lines()
        assert len(report) == 1 and report[0].startswith("isf: @1 ") and report[0].endswith("(n = 200, skipped 4)")
        assert run(index, ["--beta", "10", "-e", paths["dict.txt"]]) \
            == g.evaluate_dictionary(target, source, pairs, KS, "isf", beta=10.0).lines()
        assert run(index, ["--isf-sources", "150", "-k", "1,2", "-e", paths["dict.txt"]]) \
            == g.evaluate_dictionary(target, source, pairs, (1, 2), "isf", sources=150).lines()      # a file in word order
    ranked = run("flat.idx", ["--beta", "10", "--isf-sources", "400", "-e", paths["dict.txt"], "--ranks", "-k", "1,100"])
    by_ranks = g.evaluate_dictionary_ranks(spaces["flat"], source, pairs, (1, 100), "isf", beta=10.0, sources=400)
    assert len(ranked) == 2 and ranked[1] == by_ranks.line() and ranked[1].startswith("isf ranks: mrr ")
    assert ranked[0] == f"isf: @1 {by_ranks.precision(1):.4f} @100 {by_ranks.precision(100):.4f} (n = 200, skipped 4)"
    assert run("grouped.idx", ["-e", paths["dict.txt"], "--ranks"], status=1) == []  # refused, as for csls
    assert run("flat.idx", ["--isf-sources", "601", "-e", paths["dict.txt"]], status=1) == []
    exact = run("flat.idx", ["-v", paths["target.txt"], "--exact", "-e", paths["dict.txt"]])
    assert exact[0].startswith("isf: @1 ") and exact[0].endswith("(n = 200, skipped 4)")


def test_isf_sources_counts_lines_of_the_source_file(g, spaces, tmp_path):
    """A word2vec file lists its words by frequency and the command holds the source in word order: --isf-sources N
    must sum over the words of the file's first N lines, wherever they sort.  The source file here is the fixture's
    with its lines shuffled; the expected offsets are isf_offsets over the rows those words have in word order."""
    from gulon_amd import cli
    paths, pairs = spaces["paths"], dictionary(spaces["perm"])
    lines = open(paths["source.txt"]).read().splitlines()[1:]
    order = np.random.default_rng(11).permutation(N)
    shuffled = str(tmp_path / "shuffled.txt")
    with open(shuffled, "w") as fh:
        fh.write(f"{N} {D}\n" + "".join(lines[i] + "\n" for i in order))
    top = 120
    frequent = sorted(int(i) for i in order[:top])               # S_WORDS sort as their numbers: row = word number
    assert frequent != list(range(top))
    vectors = cli.read_originals(shuffled, True)
    assert vectors.words == S_WORDS and vectors.file_rows[order].tolist() == list(range(N))
    assert cli._frequent_rows(top, vectors).tolist() == frequent
    source = g.ExactWordIndex(vectors.words, g.ExactIndex(vectors.matrix, "cosine"), vectors.key_index)

    def run(extra):
        out = io.BytesIO()
        assert cli.main(["translate", "-i", paths["flat.idx"], "-s", shuffled, "--method", "isf", "--isf-sources", str(top)]
                        + extra, stdout=out) == 0
        return out.getvalue().decode("utf-8").splitlines()
    try:
        target = spaces["flat"]
        by_rows = g.evaluate_dictionary(target, source, pairs, tuple(range(1, 11)), "isf", sources=np.asarray(frequent))
        by_prefix = g.evaluate_dictionary(target, source, pairs, tuple(range(1, 11)), "isf", sources=top)
        assert run(["-k", "1,2,3,4,5,6,7,8,9,10", "-e", paths["dict.txt"]]) == by_rows.lines()
        ranked = run(["-e", paths["dict.txt"], "--ranks", "-k", "1,100"])
        want = g.evaluate_dictionary_ranks(target, source, pairs, (1, 100), "isf", sources=np.asarray(frequent))
        assert ranked[1] == want.line()
        words = run(["-k", "3", paths["words.txt"]])
        mine = g.translate_words(target, source, ["s003", "missing", "s599"], 3, "isf", sources=np.asarray(frequent))
        assert words == [f"{w}: not found" if r is None else f"{w}: {','.join(r.words)}"
                         for w, r in zip(["s003", "missing", "s599"], mine)]
        a = g.isf_offsets(target, source, BETA, np.asarray(frequent))
        b = g.isf_offsets(target, source, BETA, top)
        try:
            assert not np.array_equal(bits(a.numpy()), bits(b.numpy()))      # the first 120 in word order are other words
        finally:
            a.free()
            b.free()
        print(by_rows.line(), "|", by_prefix.line())
    finally:
        source.close()
