"""Analogy accuracy by 3CosMul (analogies.evaluate_analogies(method="mul"), csrc/cosmul.hip): the device
route against the generic route and against the counts of the numpy reference lists through count_lists, for a flat
WordIndex and an ExactWordIndex; the two commands end to end on files; a grouped index reported as an error."""
import io

import numpy as np
import pytest

from cosmul_ref import adc_distances, exact_distances, per_expression, reference_lists

pytestmark = pytest.mark.gpu

N_WORDS, N_BASE, N_QUESTIONS, D = 400, 340, 60, 24
WORDS = [f"w{i:04d}" for i in range(N_WORDS)]            # String order = row order
KS = (1, 5, 10)


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def planted():
    """Unit vectors; question i is rows (3i, 3i + 1, 3i + 2) -> row N_BASE + i = normalize(b - a + c + 0.01 noise)."""
    rng = np.random.default_rng(7)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    X = unit(rng.standard_normal((N_WORDS, D)))
    a, b, c = (X[np.arange(N_QUESTIONS) * 3 + j] for j in range(3))
    X[N_BASE:] = unit(b - a + c + 0.01 * rng.standard_normal((N_QUESTIONS, D)))
    questions = [(WORDS[3 * i], WORDS[3 * i + 1], WORDS[3 * i + 2], WORDS[N_BASE + i]) for i in range(N_QUESTIONS)]
    return X.astype(np.float32), questions


def sections_of(questions):
    """Planted questions; random ones with a repeated operand among them; skipped questions (an absent word) and questions
    that can never hit (d is an operand)."""
    rng = np.random.default_rng(3)
    random = [tuple(WORDS[int(r)] for r in rng.choice(N_BASE, 4, replace=False)) for _ in range(30)]
    random += [("w0007", "w0007", "w0009", "w0010"), ("w0010", "w0011", "w0010", "w0011")]
    odd = [("w0001", "w0002", "w0003", "w0002"), ("w0001", "absent", "w0003", "w0004"), ("w0001", "w0002", "w0003", "absent"),
           ("W0001", "w0002", "w0003", "w0004"), ("w0030", "w0031", "w0032", "w0030")]
    return [("planted", questions), ("random", random), ("odd", odd)]


@pytest.fixture(scope="module")
def world(g):
    from gulon_amd.grouped import GroupedIndex, group
    from gulon_amd.kmeans import Config as KMeansConfig
    X, questions = planted()
    dm = g.DeviceMatrix.from_host(X)
    pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(64, 8, 4))
    flat = g.WordIndex(WORDS, g.Index.sorted(dm, pq, "cosine"))
    exact = g.ExactWordIndex(WORDS, g.ExactIndex(dm, "cosine"))
    gv = group(dm, g.KMeans.compute_clusters(g.Vectors(dm), KMeansConfig(6, 4)))
    rpq = g.ProductQuantizer.apply(gv.residuals, g.ProductQuantizerConfig(64, 8, 4))
    gx = GroupedIndex(rpq, rpq.encode(gv.residuals), gv.centroids, gv.offsets, g.LimitGroups(3), "cosine")
    grouped = g.WordIndex([WORDS[i] for i in gv.perm], gx)
    return {"X": X, "questions": questions, "pq": pq, "flat": flat, "exact": exact, "grouped": grouped}


def reference_report(world, oracle, kind, sections):
    """(asked, skipped, hits) per section from the numpy reference lists, scored by count_lists."""
    from gulon_amd.analogies import count_lists
    target, X = world[kind], world["X"]
    items, skipped = [], [0] * len(sections)
    for s, (_, questions) in enumerate(sections):
        for q in questions:
            rows = [target.row_of(w) for w in q]
            if any(r is None for r in rows):
                skipped[s] += 1
            else:
                items.append((s, rows))
    exprs = [[(b, 1.0), (a, -1.0), (c, 1.0)] for _, (a, b, c, _) in items]
    units = [[(r, 1.0)] for e in exprs for r, _ in e]
    if kind == "exact":
        D = exact_distances(X, target.index.compose_rows(units))
    else:
        pq, vi = world["pq"], target.index.vector_index
        Q = target.index.compose_rows(units)
        codes = np.ascontiguousarray(vi.data.indices().T)
        D = adc_distances(oracle.prepare_query(pq.flat_centroids(), X.shape[1], codes.shape[1], 64, Q), codes)
    lists, _, counts = reference_lists(per_expression(D, exprs), exprs, np.arange(N_WORDS), KS[-1])
    hits, asked = count_lists(lists, counts, [rows[3] for _, rows in items], [s for s, _ in items], KS, len(sections))
    return [(int(asked[s]), skipped[s], {k: int(hits[s, j]) for j, k in enumerate(KS)}) for s in range(len(sections))]


@pytest.mark.parametrize("kind", ["flat", "exact"])
def test_the_routes_give_the_reference_report(g, oracle, world, kind):
    from gulon_amd.analogies import evaluate_analogies
    target, sections = world[kind], sections_of(world["questions"])
    device = evaluate_analogies(target, sections, KS, method="mul")
    generic = evaluate_analogies(target, sections, KS, route="generic", method="mul")
    want = reference_report(world, oracle, kind, sections)
    for report in (device, generic):
        assert [(s.asked, s.skipped, s.hits) for s in report.sections] == want
    assert device.lines() == generic.lines()
    by_name = {s.name: s for s in device.sections}
    assert (by_name["odd"].asked, by_name["odd"].skipped, by_name["odd"].hits) == (2, 3, {1: 0, 5: 0, 10: 0})
    assert by_name["random"].asked == 32 and device.asked == N_QUESTIONS + 32 + 2
    if kind == "exact":
        assert by_name["planted"].hits[10] == N_QUESTIONS       # the true vectors find every planted word


def test_method_is_checked(g, world):
    from gulon_amd.analogies import evaluate_analogies
    sections = sections_of(world["questions"])
    with pytest.raises(ValueError):
        evaluate_analogies(world["exact"], sections, KS, method="max")
    with pytest.raises(NotImplementedError):
        evaluate_analogies(world["grouped"], sections, KS, method="mul")
    with pytest.raises(NotImplementedError):
        evaluate_analogies(world["flat"].restrict(WORDS[:50]), sections, KS, method="mul")


def test_the_commands_end_to_end(g, world, tmp_path, capsys):
    from gulon_amd import cli
    from gulon_amd.analogies import evaluate_analogies, read_questions
    from gulon_amd.index_file import dump_index
    X, questions = world["X"], world["questions"]
    paths = {n: str(tmp_path / n) for n in ("flat.idx", "grouped.idx", "vectors.txt", "questions.txt", "lines.txt")}
    with open(paths["flat.idx"], "wb") as fh:
        fh.write(dump_index(world["flat"].index, WORDS))
    with open(paths["grouped.idx"], "wb") as fh:
        fh.write(dump_index(world["grouped"].index, world["grouped"].words))
    with open(paths["vectors.txt"], "w") as fh:
        fh.write(f"{N_WORDS} {D}\n")
        for w, row in zip(WORDS, X):
            fh.write(w + " " + " ".join(repr(float(x)) for x in row) + "\n")
    text = ": planted\n" + "".join(" ".join(q) + "\n" for q in questions) + ": odd\nw0001 w0002 nowhere w0003\n" \
           "w0001 w0002 w0003 w0002\n"
    with open(paths["questions.txt"], "w") as fh:
        fh.write(text)
    sections = read_questions(text.splitlines())

    def run(argv, code=0):
        out = io.BytesIO()
        assert cli.main(argv, stdout=out) == code
        return out.getvalue().decode("utf-8").splitlines()
    alone = run(["analogies", "-i", paths["flat.idx"], "--method", "mul", paths["questions.txt"]])
    assert alone == evaluate_analogies(world["flat"], sections, method="mul").lines() and len(alone) == 3
    assert alone[1].startswith("odd: @1 0.0000") and alone[1].endswith("(n = 1, skipped 1)")
    exact = run(["analogies", "-i", paths["flat.idx"], "--method", "mul", "-v", paths["vectors.txt"], "--exact",
                 paths["questions.txt"]])
    assert exact == evaluate_analogies(world["exact"], sections, method="mul").lines()
    assert exact[0].startswith("planted: ") and "@10 1.0000" in exact[0]
    # the additive method is what it was
    add = run(["analogies", "-i", paths["flat.idx"], paths["questions.txt"]])
    assert add == evaluate_analogies(world["flat"], sections).lines()
    # query-words -x --method mul
    lines = ["w0001 - w0000 + w0002", "w0005", "w0001 - nowhere", "w0001 +"]
    with open(paths["lines.txt"], "w") as fh:
        fh.write("\n".join(lines) + "\n")
    got = run(["query-words", "-i", paths["flat.idx"], "-k", "3", "-x", "--method", "mul", paths["lines.txt"]])
    want = world["flat"].batch_query_cosmul(3, lines[:2])
    assert got == [f"{lines[0]}: {','.join(want[0].words)}", f"{lines[1]}: {','.join(want[1].words)}",
                   f"{lines[2]}: not found", f"{lines[3]}: invalid expression"]
    assert not set(want[0].words) & {"w0000", "w0001", "w0002"}
    # a grouped index has no cosmul queries: reported, exit code 1
    capsys.readouterr()
    assert run(["analogies", "-i", paths["grouped.idx"], "--method", "mul", paths["questions.txt"]], code=1) == []
    assert capsys.readouterr().err.startswith("error: ")
    assert run(["query-words", "-i", paths["grouped.idx"], "-x", "--method", "mul", paths["lines.txt"]], code=1) == []
    assert capsys.readouterr().err.startswith("error: ")
