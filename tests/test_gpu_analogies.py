"""Analogy accuracy on the device (csrc/analogy.hip, gulon_amd/analogies.py): the counts kernel against numpy, a planted
question set the true vectors must answer 200/200, the device route against the generic route and against the lists of
batch_query_expressions read in Python, skipped and never-hit questions, and the command end to end."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_WORDS, N_BASE, N_QUESTIONS, D = 2000, 1800, 200, 32
WORDS = [f"w{i:04d}" for i in range(N_WORDS)]            # String order = row order


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


# ---- the counts kernel -----------------------------------------------------------------------------------------------

KS_OF = {1: (1,), 64: (1, 5, 64), 65: (1, 64, 65), 300: (1, 5, 10, 65, 300)}


def _lists(kin, nsections, seed):
    """Lists of distinct rows with counts in [0, kin]; the expected row absent, at position 0, at ks[j] - 1 and ks[j] for
    each j, past the live entries, and at random positions."""
    rng = np.random.default_rng(seed)
    ks = KS_OF[kin]
    places = [None, 0] + [k - 1 for k in ks] + [k for k in ks if k < kin] + [int(p) for p in rng.integers(0, kin, 12)]
    b = 2 * len(places) + 1
    lists = np.stack([rng.permutation(5000)[:kin] for _ in range(b)]).astype(np.int32)
    counts = rng.integers(0, kin + 1, b).astype(np.int32)
    expected = np.zeros(b, np.int32)
    for q in range(b):
        place = places[q % len(places)]
        if q < len(places):
            counts[q] = kin                                # the first round: every place is live
        expected[q] = 6000 + q if place is None else lists[q, place]
    counts[-1], expected[-1] = 0, 3                        # an answer of nothing but padding
    lists = np.where(np.arange(kin)[None, :] < counts[:, None], lists, -1).astype(np.int32)   # padded as the queries pad
    if kin > 1:                                            # the expected row only past the live entries: not found
        q = len(places) + 1
        counts[q] = kin // 2
        lists[q, :kin // 2] = np.arange(7000, 7000 + kin // 2)
        lists[q, kin // 2:] = expected[q]
    section = rng.integers(0, nsections, b).astype(np.int32)
    return lists, counts, expected, section, np.asarray(ks, np.int32)


def _numpy_counts(lists, counts, expected, section, ks, nsections):
    rank = np.full(len(lists), -1, np.int32)
    for q in range(len(lists)):
        at = np.flatnonzero(lists[q, :counts[q]] == expected[q])
        if len(at):
            rank[q] = at[0]
    hits, asked = np.zeros((nsections, len(ks)), np.int32), np.zeros(nsections, np.int32)
    for q in range(len(lists)):
        asked[section[q]] += 1
        for j, k in enumerate(ks):
            hits[section[q], j] += 0 <= rank[q] < k
    return hits, asked, rank


@pytest.mark.parametrize("nsections", [1, 20])
@pytest.mark.parametrize("kin", [1, 64, 65, 300])
def test_counts_kernel_against_numpy(g, kin, nsections):
    import torch
    from gulon_amd.analogies import count_lists
    N = g.native
    first = _lists(kin, nsections, 10 * kin + nsections)
    second = _lists(kin, nsections, 10 * kin + nsections + 5)
    ks = first[4]
    want1, want2 = _numpy_counts(*first, nsections), _numpy_counts(*second, nsections)
    assert (want1[2] == -1).any() and (want1[2] == 0).any() and (want1[2] == ks[-1] - 1).any()
    # the host form: ranks given, then two calls into the same counters with the ranks null
    hits, asked, rank = count_lists(*first[:4], ks, nsections, ranks=True)
    assert np.array_equal(hits, want1[0]) and np.array_equal(asked, want1[1]) and np.array_equal(rank, want1[2])
    hits, asked = count_lists(*second[:4], ks, nsections, hits, asked)
    assert np.array_equal(hits, want1[0] + want2[0]) and np.array_equal(asked, want1[1] + want2[1])
    assert asked.sum() == len(first[0]) + len(second[0])
    # the device form, on torch's buffers
    d_hits = torch.zeros((nsections, len(ks)), dtype=torch.int32, device="cuda")
    d_asked = torch.zeros(nsections, dtype=torch.int32, device="cuda")
    d_ks = torch.from_numpy(ks).cuda()
    for (lists, counts, expected, section, _), want, with_rank in ((first, want1, True), (second, want2, False)):
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (lists, counts, expected, section)]
        d_rank = torch.full((len(lists),), 7, dtype=torch.int32, device="cuda")
        N.check(N.lib().gulon_analogy_counts_dev(t[0].data_ptr(), t[1].data_ptr(), len(lists), kin, t[2].data_ptr(),
                                                 t[3].data_ptr(), d_ks.data_ptr(), len(ks), nsections, d_hits.data_ptr(),
                                                 d_asked.data_ptr(), d_rank.data_ptr() if with_rank else None, None))
        torch.cuda.synchronize()
        if with_rank:
            assert np.array_equal(d_rank.cpu().numpy(), want[2])
    assert np.array_equal(d_hits.cpu().numpy(), want1[0] + want2[0])
    assert np.array_equal(d_asked.cpu().numpy(), want1[1] + want2[1])


def test_counts_host_form_checks_its_arguments(g):
    from gulon_amd.analogies import count_lists
    lists, counts = np.arange(8, dtype=np.int32).reshape(2, 4), np.array([4, 4], np.int32)
    for kw, message in ((dict(section=[0, 3]), r"section\[1\] = 3 outside \[0, 3\)"),
                        (dict(ks=[1, 5]), r"ks\[1\] = 5"), (dict(ks=[2, 2]), r"ks\[1\] = 2"), (dict(ks=[0]), r"ks\[0\] = 0"),
                        (dict(expected=[1, -1]), r"expected\[1\] = -1"), (dict(ks=list(range(1, 18))), "nks=17")):
        args = dict(expected=[1, 6], section=[0, 2], ks=[1, 4])
        args.update(kw)
        with pytest.raises(ValueError, match=message):
            count_lists(lists, counts, args["expected"], args["section"], args["ks"], 3)
    hits, asked = count_lists(np.zeros((0, 4), np.int32), [], [], [], [1, 4], 3)              # b = 0
    assert not hits.any() and not asked.any()


# ---- the planted set -------------------------------------------------------------------------------------------------

def _normalize64(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def planted(metric):
    """2 000 standard-normal vectors; question i is rows (3i, 3i + 1, 3i + 2) -> row 1 800 + i, which is set to
    b - a + c + 0.01 noise (cosine: all rows normalised, the planted row normalize(b^ - a^ + c^ + 0.01 noise))."""
    rng = np.random.default_rng(7)
    X = rng.standard_normal((N_WORDS, D))
    noise = rng.standard_normal((N_QUESTIONS, D))
    if metric == "cosine":
        X = _normalize64(X)
    a, b, c = (X[np.arange(N_QUESTIONS) * 3 + j] for j in range(3))
    X[N_BASE:] = b - a + c + 0.01 * noise
    if metric == "cosine":
        X[N_BASE:] = _normalize64(X[N_BASE:])
    X = X.astype(np.float32)
    questions = [(WORDS[3 * i], WORDS[3 * i + 1], WORDS[3 * i + 2], WORDS[N_BASE + i]) for i in range(N_QUESTIONS)]
    return X, questions


def margin(X, metric):
    """float64: the smallest ratio, over the questions, of the squared distance of the nearest other non-operand word
    to that of the planted word."""
    X = X.astype(np.float64)
    worst = np.inf
    for i in range(N_QUESTIONS):
        a, b, c = X[3 * i], X[3 * i + 1], X[3 * i + 2]
        q = b - a + c
        if metric == "cosine":
            q = _normalize64(_normalize64(b) - _normalize64(a) + _normalize64(c))
        dist = ((X - q) ** 2).sum(axis=1)
        others = np.delete(dist, [3 * i, 3 * i + 1, 3 * i + 2, N_BASE + i])
        worst = min(worst, others.min() / dist[N_BASE + i])
    return worst


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_the_true_vectors_answer_every_planted_question(g, metric):
    """The margin is checked in float64 before the GPU is touched: the nearest other non-operand word is at least 100
    times farther in squared distance than the planted one (with this generator: 8 029 times for l2, 347 for cosine),
    so binary32 rounding -- a relative error below 1e-5 in a sum of 32 squares, and as little in the composed query --
    cannot reorder them."""
    from gulon_amd.analogies import evaluate_analogies
    X, questions = planted(metric)
    assert margin(X, metric) >= 100
    dm = g.DeviceMatrix.from_host(X)
    target = g.ExactWordIndex(WORDS, g.ExactIndex(dm, metric))
    report = evaluate_analogies(target, [("planted", questions)], ks=(1,))
    assert (report.sections[0].asked, report.sections[0].skipped, report.sections[0].hits) == (200, 0, {1: 200})
    assert report.lines() == ["planted: @1 1.0000 (n = 200, skipped 0)", "total: @1 1.0000 (n = 200, skipped 0)"]
    assert evaluate_analogies(target, [("planted", questions)], ks=(1,), route="generic").lines() == report.lines()
    r = target.query_expression(3, f"{questions[5][1]} - {questions[5][0]} + {questions[5][2]}")
    assert r.words[0] == questions[5][3] and not set(r.words) & set(questions[5][:3])
    assert target.batch_query_expressions(3, ["w0001 - nowhere", [("w0001", 1.0)]])[0] is None
    target.close()
    dm.close()


# ---- routes ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def indexes(g):
    """A sorted and a grouped WordIndex over the same words (the planted l2 vectors), and the true vectors."""
    from gulon_amd.grouped import GroupedIndex, group
    from gulon_amd.kmeans import Config as KMeansConfig
    X, questions = planted("l2")
    dm = g.DeviceMatrix.from_host(X)
    pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(64, 8, 4))
    sorted_index = g.WordIndex(WORDS, g.Index.sorted(dm, pq, "l2"))
    clustering = g.KMeans.compute_clusters(g.Vectors(dm), KMeansConfig(12, 4))
    gv = group(dm, clustering)
    rpq = g.ProductQuantizer.apply(gv.residuals, g.ProductQuantizerConfig(64, 8, 4))
    gx = GroupedIndex(rpq, rpq.encode(gv.residuals), gv.centroids, gv.offsets, g.LimitGroups(3), "l2")
    grouped_index = g.WordIndex([WORDS[i] for i in gv.perm], gx)
    exact = g.ExactWordIndex(WORDS, g.ExactIndex(dm, "l2"))
    return {"sorted": sorted_index, "grouped": grouped_index, "exact": exact, "X": X, "questions": questions}


def _sections(target, questions):
    """Sections that exercise the report: planted questions; questions whose d is what the target itself answers at a
    chosen rank (so every k gets hits and misses); repeated operands (one and two distinct); absent words; a d that
    is an operand."""
    rng = np.random.default_rng(3)
    ranked = []
    for i in range(60):
        a, b, c = (WORDS[int(r)] for r in rng.choice(N_BASE, 3, replace=False))
        ranked.append((a, b, c, i % 12))
    answers = target.batch_query_expressions(12, [[(b, 1.0), (a, -1.0), (c, 1.0)] for a, b, c, _ in ranked])
    at_rank = [(a, b, c, r.words[rank]) for (a, b, c, rank), r in zip(ranked, answers)]
    repeats = [("w0007", "w0007", "w0009", "w0009"), ("w0010", "w0011", "w0010", "w0011"), ("w0012", "w0012", "w0012", "w0013"),
               ("w0020", "w0021", "w0021", "w0500")]
    odd = [("w0001", "w0002", "w0003", "w0002"), ("w0001", "absent", "w0003", "w0004"), ("w0001", "w0002", "w0003", "absent"),
           ("W0001", "w0002", "w0003", "w0004"), ("w0030", "w0031", "w0032", "w0030")]
    return [("planted", questions[:40]), ("at rank", at_rank), ("", repeats), ("odd", odd), ("empty", [])]


def _python_report(target, sections, ks):
    """The report read off batch_query_expressions in Python."""
    out = []
    for name, questions in sections:
        asked, skipped, hits = 0, 0, {k: 0 for k in ks}
        for a, b, c, d in questions:
            if any(target.row_of(w) is None for w in (a, b, c, d)):
                skipped += 1
                continue
            asked += 1
            words = target.batch_query_expressions(ks[-1], [[(b, 1.0), (a, -1.0), (c, 1.0)]])[0].words
            for k in ks:
                hits[k] += d in words[:k]
        out.append((name, asked, skipped, hits))
    return out


@pytest.mark.parametrize("kind", ["sorted", "grouped", "exact"])
def test_the_routes_give_one_report(g, indexes, kind):
    from gulon_amd.analogies import evaluate_analogies
    target, ks = indexes[kind], (1, 5, 10)
    sections = _sections(target, indexes["questions"])
    device = evaluate_analogies(target, sections, ks)
    generic = evaluate_analogies(target, sections, ks, route="generic")
    want = _python_report(target, sections, ks)
    for report in (device, generic):
        assert [(s.name, s.asked, s.skipped, s.hits) for s in report.sections] == want
    by_name = {s.name: s for s in device.sections}
    assert by_name["at rank"].hits == {1: 5, 5: 25, 10: 50} and by_name["at rank"].asked == 60
    assert (by_name["odd"].asked, by_name["odd"].skipped) == (2, 3) and by_name["odd"].hits == {1: 0, 5: 0, 10: 0}
    assert (by_name["empty"].asked, by_name["empty"].skipped) == (0, 0)
    assert device.asked == 40 + 60 + 4 + 2 and device.skipped == 3 and device.lines() == generic.lines()
    if kind == "exact":
        assert by_name["planted"].hits == {1: 40, 5: 40, 10: 40}


def test_skipped_and_never_hit_questions(g, indexes):
    """A question with an absent word is skipped; a d that is an operand is asked and never hit, at any depth: the
    operands are dropped from every answer."""
    from gulon_amd.analogies import evaluate_analogies
    exact, X = indexes["exact"], indexes["X"]
    i = 9
    a, b, c, d = indexes["questions"][i]
    raw = exact.index.batch_query_raw(3, (X[3 * i + 1] - X[3 * i] + X[3 * i + 2])[None, :])
    assert raw[0][0, 0] == N_BASE + i                                  # the planted row first, operands among the rest
    for target in (exact, indexes["sorted"]):
        sections = [("s", [(a, b, c, d), (a, b, c, b), (a, b, c, a), (a, "nowhere", c, d), (a, b, c, "nowhere")])]
        for route in (None, "generic"):
            s = evaluate_analogies(target, sections, (1, 2000), route=route).sections[0]
            assert (s.asked, s.skipped) == (3, 2)
            assert s.hits[2000] == 1                                 # d = b and d = a: asked, never among the answers
            assert s.hits[1] == 1 or target is not exact


# ---- the command -----------------------------------------------------------------------------------------------------

def test_the_command_end_to_end(g, indexes, tmp_path, capsys):
    from gulon_amd import cli
    from gulon_amd.analogies import evaluate_analogies, read_questions
    from gulon_amd.index_file import dump_index
    X, questions = indexes["X"], indexes["questions"]
    index_path, vectors_path, questions_path = (str(tmp_path / n) for n in ("planted.idx", "vectors.txt", "questions.txt"))
    with open(index_path, "wb") as fh:
        fh.write(dump_index(indexes["sorted"].index, WORDS))
    with open(vectors_path, "w") as fh:
        fh.write(f"{N_WORDS} {D}\n")
        for w, row in zip(WORDS, X):
            fh.write(w + " " + " ".join(repr(float(x)) for x in row) + "\n")
    text = ": First Half\n" + "".join(" ".join(q).upper() + "\n" for q in questions[:100]) + \
           ": second half\n" + "".join(" ".join(q) + "\n" for q in questions[100:]) + "w0001 w0002 nowhere w0003\n"
    with open(questions_path, "w") as fh:
        fh.write(text)
    sections = read_questions(text.splitlines(), lowercase=True)

    def run(argv):
        out = io.BytesIO()
        assert cli.main(["analogies", "-i", index_path] + argv + [questions_path], stdout=out) == 0
        return out.getvalue().decode("utf-8").splitlines()
    alone = run(["--lowercase", "-k", "1,5"])
    want = evaluate_analogies(indexes["sorted"], sections, (1, 5))
    assert alone == want.lines() and len(alone) == 3
    assert alone[0].startswith("First Half: @1 ") and alone[0].endswith("(n = 100, skipped 0)")
    assert alone[1].startswith("second half: @1 ") and alone[1].endswith("(n = 100, skipped 1)")
    assert alone[2] == f"total: @1 {want.hits[1] / 200:.4f} @5 {want.hits[5] / 200:.4f} (n = 200, skipped 1)"
    exact = run(["--lowercase", "-v", vectors_path, "--exact"])
    assert exact == ["First Half: @1 1.0000 @5 1.0000 @10 1.0000 (n = 100, skipped 0)",
                     "second half: @1 1.0000 @5 1.0000 @10 1.0000 (n = 100, skipped 1)",
                     "total: @1 1.0000 @5 1.0000 @10 1.0000 (n = 200, skipped 1)"]
    assert exact == evaluate_analogies(indexes["exact"], sections).lines()
    # without --lowercase the upper-case half names no word of the index
    assert run([])[0] == "First Half: @1 0.0000 @5 0.0000 @10 0.0000 (n = 0, skipped 100)"
    bad = tmp_path / "bad.txt"
    bad.write_text("a b c d\na b c\n")
    assert cli.main(["analogies", "-i", index_path, str(bad)], stdout=io.BytesIO()) == 1
    assert "bad.txt: line 2" in capsys.readouterr().err
