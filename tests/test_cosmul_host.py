"""The host side of the 3CosMul work (expressions.cosmul_reference, analogies.evaluate_analogies(method=...), the
--method option of the analogies and query-words commands), against stubs.  No GPU."""
import io

import numpy as np
import pytest

from gulon_amd import cli
from gulon_amd.analogies import AnalogyReport, SectionScore
from gulon_amd.expressions import COSMUL_EPS, cosmul_reference

f32 = np.float32


# ---- cosmul_reference ------------------------------------------------------------------------------------------------

def test_one_positive_term_ranks_as_distance_ascending():
    d = np.random.default_rng(0).uniform(0, 4, 200).astype(f32)
    score = cosmul_reference(d[None, :], [1.0])
    assert score.dtype == f32 and (score >= 0).all()
    order = np.lexsort((np.arange(200), -score))
    assert (np.diff(d[order]) >= 0).all()
    assert np.array_equal(score, ((f32(1) - f32(0.25) * d) / (f32(1) + COSMUL_EPS)).astype(f32))   # P / (1 + eps)


def test_clamp_and_nan():
    d = np.array([[0.0, 4.0, 4.000001, 7.5, np.nan, np.inf, 2.0]], f32)
    score = cosmul_reference(d, [1.0])
    assert score[0] == f32(1) / (f32(1) + COSMUL_EPS)
    assert (score[1:6] == 0).all() and not np.signbit(score[1:6]).any() and np.isfinite(score).all()
    assert score[6] == f32(0.5) / (f32(1) + COSMUL_EPS)
    # a NaN or a distance above 4 in a negative term: the denominator is eps alone
    both = cosmul_reference(np.array([[2.0, 2.0], [np.nan, 9.0]], f32), [1.0, -1.0])
    assert (both == f32(0.5) / (f32(0) + COSMUL_EPS)).all()


def test_products_in_list_order_with_float32_at_every_step():
    rng = np.random.default_rng(1)
    d = rng.uniform(0, 4, (5, 300)).astype(f32)
    w = [-1.0, 1.0, 1.0, 1.0, -1.0]
    s = [np.maximum(f32(1) - (f32(0.25) * d[t]).astype(f32), f32(0)).astype(f32) for t in range(5)]
    P = ((s[1] * s[2]).astype(f32) * s[3]).astype(f32)
    N = (s[0] * s[4]).astype(f32)
    want = (P / (N + f32(0.001)).astype(f32)).astype(f32)
    got = cosmul_reference(d, w)
    assert got.dtype == f32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # float64 arithmetic rounded once differs somewhere: every step is its own rounding
    s64 = [np.maximum(1 - 0.25 * d[t].astype(np.float64), 0) for t in range(5)]
    once = (s64[1] * s64[2] * s64[3] / (s64[0] * s64[4] + 0.001)).astype(f32)
    assert (once != got).any() and np.allclose(once, got, rtol=1e-5)
    assert COSMUL_EPS.dtype == f32 and COSMUL_EPS == f32(0.001)
    assert cosmul_reference(d.astype(np.float64), w).dtype == f32


def test_reference_checks_its_arguments():
    d = np.zeros((2, 3), f32)
    for bad in ([1.0], [-1.0, -1.0], [0.0, -2.0], []):
        with pytest.raises(ValueError):
            cosmul_reference(d, bad)
    with pytest.raises(ValueError):
        cosmul_reference(np.zeros(3, f32), [1.0])
    assert np.array_equal(cosmul_reference(d, [1.0, 0.0]), cosmul_reference(d, [1.0, -1.0]))   # not > 0: negative


# ---- the commands' parsers -------------------------------------------------------------------------------------------

def _report():
    return AnalogyReport((1, 5, 10), [SectionScore("s", 4, 1, {1: 1, 5: 2, 10: 3})])


class StubIndex:
    metric = "cosine"

    def __init__(self, tag="plain"):
        self.tag = tag

    def exact(self, vectors):
        return StubIndex("exact")

    def refined(self, vectors, candidates):
        return StubIndex("refined")


def _analogies(argv, analogies=None, stub=None):
    out, seen = io.BytesIO(), []

    def default(config, load, vectors):
        seen.append(config)
        return _report()
    rc = cli.main(["analogies"] + argv, stdout=out, load=lambda path: stub if stub is not None else StubIndex(),
                  vectors=lambda path, normalize: ("vectors of " + path, normalize),
                  analogies=analogies if analogies is not None else default)
    return rc, out.getvalue().decode("utf-8"), seen


def test_analogies_method_option():
    assert cli.AnalogiesConfig("i", "q").method == "add"
    assert cli.AnalogiesConfig("i", "q", (1,), False, None, False, None) == cli.AnalogiesConfig("i", "q", (1,), method="add")
    _, _, seen = _analogies(["-i", "idx", "q.txt"])
    assert seen[0].method == "add" and seen == [cli.AnalogiesConfig("idx", "q.txt", (1, 5, 10), False, None, False, None)]
    _, _, seen = _analogies(["-i", "idx", "--method", "mul", "q.txt"])
    assert seen == [cli.AnalogiesConfig("idx", "q.txt", (1, 5, 10), False, None, False, None, "mul")]
    _, _, seen = _analogies(["-i", "idx", "--method", "mul", "-v", "vec.txt", "--exact", "q.txt"])
    assert seen[0].method == "mul" and seen[0].exact and seen[0].vectors == "vec.txt"
    _, _, seen = _analogies(["-i", "idx", "--method", "add", "-v", "vec.txt", "-c", "9", "q.txt"])
    assert seen[0].method == "add" and seen[0].candidates == 9


@pytest.mark.parametrize("command,argv,message", [
    ("analogies", ["-i", "idx", "--method", "mul", "-v", "vec.txt", "q.txt"], "--method mul is only applicable with --vectors"),
    ("analogies", ["-i", "idx", "--method", "mul", "-v", "vec.txt", "-c", "5", "q.txt"], "--method mul is only"),
    ("analogies", ["-i", "idx", "--method", "max", "q.txt"], "invalid choice"),
    ("query-words", ["-i", "idx", "--method", "mul"], "--method mul needs -x/--expressions"),
    ("query-words", ["-i", "idx", "-x", "--method", "mul", "-f", "fine.idx"], "--method mul is not applicable with -f/--fine"),
    ("query-words", ["-i", "idx", "-x", "--method", "mul", "-R", "rot.bin"], "not applicable with -R/--rotation"),
    ("query-words", ["-i", "idx", "-x", "--method", "mul", "-r", "words.txt"], "not applicable with -r/--restrict"),
    ("query-words", ["-i", "idx", "-x", "--method", "mul", "-v", "vec.txt"], "not applicable with -v/--vectors"),
    ("query", ["-i", "idx", "--method", "mul", "q.txt"], "unrecognized arguments")])
def test_parser_rules(command, argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main([command] + argv, stdout=io.BytesIO(), stdin=io.BytesIO(b""), load=lambda path: StubIndex())
    assert e.value.code == 2
    assert message in capsys.readouterr().err


# ---- the method is passed through ------------------------------------------------------------------------------------

def test_run_analogies_passes_the_method(tmp_path, monkeypatch):
    from gulon_amd import analogies
    path = tmp_path / "q.txt"
    path.write_text(": s\na b c d\n")
    calls = []

    def evaluate(target, sections, ks, **kw):
        calls.append((target.tag, ks, kw))
        return _report()
    monkeypatch.setattr(analogies, "evaluate_analogies", evaluate)
    rc, out, _ = _analogies(["-i", "idx", str(path)], analogies=cli.run_analogies)
    assert rc == 0 and calls.pop() == ("plain", (1, 5, 10), {})                    # add: the three arguments alone
    rc, out, _ = _analogies(["-i", "idx", "--method", "mul", str(path)], analogies=cli.run_analogies)
    assert rc == 0 and calls.pop() == ("plain", (1, 5, 10), {"method": "mul"})
    rc, out, _ = _analogies(["-i", "idx", "--method", "mul", "-v", "v.txt", "--exact", str(path)], analogies=cli.run_analogies)
    assert rc == 0 and calls.pop() == ("exact", (1, 5, 10), {"method": "mul"})
    assert out.splitlines()[-1].startswith("total: ")


class WordsStub:
    """query-words' index: records which query answered."""

    def __init__(self):
        self.calls = []

    def _answer(self, name, k, exprs):
        self.calls.append((name, k, [[(t.key, t.weight) for t in e] for e in exprs]))
        from gulon_amd.word_index import WordResult
        return [WordResult([name], np.zeros(1, f32), np.zeros(1, np.int32), 0) if e.terms[0].key != "absent" else None
                for e in exprs]

    def batch_query_expressions(self, k, exprs):
        return self._answer("add", k, exprs)

    def batch_query_cosmul(self, k, exprs):
        return self._answer("mul", k, exprs)


def test_query_expressions_passes_the_method():
    lines = ["king - man + woman", "absent", "bad -"]
    for kw, name in (({}, "add"), ({"method": "add"}, "add"), ({"method": "mul"}, "mul")):
        stub, out = WordsStub(), []
        cli.query_expressions(stub, 3, lines, out.append, **kw)               # four positional parameters, as before
        assert stub.calls == [(name, 3, [[("king", 1.0), ("man", -1.0), ("woman", 1.0)], [("absent", 1.0)]])]
        assert out == [f"king - man + woman: {name}\n", "absent: not found\n", "bad -: invalid expression\n"]
    stub, out = WordsStub(), io.BytesIO()
    rc = cli.main(["query-words", "-i", "idx", "-k", "2", "-x", "--method", "mul"], stdin=io.BytesIO(b"a + b\n"), stdout=out,
                  load=lambda path: stub)
    assert rc == 0 and out.getvalue() == b"a + b: mul\n" and stub.calls[0][:2] == ("mul", 2)
    stub, out = WordsStub(), io.BytesIO()
    cli.main(["query-words", "-i", "idx", "-x"], stdin=io.BytesIO(b"a + b\n"), stdout=out, load=lambda path: stub)
    assert out.getvalue() == b"a + b: add\n"


# ---- evaluate_analogies, the generic route ---------------------------------------------------------------------------

class Target:
    """Rows by word; answers d's row first for the multiplicative query and last for the additive one."""
    metric = "cosine"
    words = ["a", "b", "c", "d", "e", "f"]

    def __init__(self):
        self.asked = []

    def row_of(self, word):
        return self.words.index(word) if word in self.words else None

    def _answers(self, name, k, exprs, first):
        from gulon_amd.index import Result
        self.asked.append((name, k, len(exprs)))
        rows = np.asarray([3, 4, 5] if first else [5, 4, 3], np.int32)
        return [Result(rows, np.zeros(3, f32), 0) for _ in exprs]

    def batch_query_expressions(self, k, exprs):
        return self._answers("add", k, exprs, False)

    def batch_query_cosmul(self, k, exprs):
        assert [[(t.key, t.weight) for t in e] for e in exprs][0] == [("b", 1.0), ("a", -1.0), ("c", 1.0)]
        return self._answers("mul", k, exprs, True)


def _numpy_count_lists(lists, counts, expected, section, ks, nsections, hits=None, asked=None, ranks=False):
    hits = np.zeros((nsections, len(ks)), np.int32) if hits is None else hits
    asked = np.zeros(nsections, np.int32) if asked is None else asked
    for q in range(len(lists)):
        asked[section[q]] += 1
        at = np.flatnonzero(np.asarray(lists[q][:counts[q]]) == expected[q])
        for j, k in enumerate(ks):
            hits[section[q], j] += bool(len(at)) and at[0] < k
    return hits, asked


def test_generic_route_asks_the_multiplicative_query(monkeypatch):
    from gulon_amd import analogies
    monkeypatch.setattr(analogies, "count_lists", _numpy_count_lists)
    sections = [("s", [("a", "b", "c", "d"), ("a", "b", "c", "nowhere")]), ("t", [("a", "b", "c", "e")])]
    target = Target()
    mul = analogies.evaluate_analogies(target, sections, (1, 3), method="mul")      # a stub has no device route
    assert target.asked == [("mul", 3, 2)]
    assert [(s.asked, s.skipped, s.hits) for s in mul.sections] == [(1, 1, {1: 1, 3: 1}), (1, 0, {1: 0, 3: 1})]
    add = analogies.evaluate_analogies(target, sections, (1, 3), route="generic")
    assert target.asked[-1] == ("add", 3, 2) and add.sections[0].hits == {1: 0, 3: 1}
    with pytest.raises(ValueError, match="unknown method"):
        analogies.evaluate_analogies(target, sections, (1,), method="cosmul")


def test_targets_that_cannot_answer():
    from gulon_amd import analogies

    class NoCosmul(Target):
        batch_query_cosmul = property()                      # hasattr: False

    class L2(Target):
        metric = "l2"
    sections = [("s", [("a", "b", "c", "d")])]
    with pytest.raises(NotImplementedError, match="cosmul"):
        analogies.evaluate_analogies(NoCosmul(), sections, (1,), method="mul")
    with pytest.raises(ValueError, match="cosine"):
        analogies.evaluate_analogies(L2(), sections, (1,), method="mul")


def test_a_target_without_cosmul_ends_as_an_error(tmp_path, capsys):
    path = tmp_path / "q.txt"
    path.write_text(": s\na b c d\n")
    rc, out, _ = _analogies(["-i", "idx", "--method", "mul", str(path)], analogies=cli.run_analogies)   # StubIndex: no cosmul
    err = capsys.readouterr().err
    assert rc == 1 and out == "" and err.startswith("error: ") and "cosmul" in err


def test_forms_without_cosmul_say_so():
    from gulon_amd.rotation import RotatedWordIndex
    from gulon_amd.word_index import RestrictedWordIndex, WordIndex
    assert callable(WordIndex.batch_query_cosmul) and callable(WordIndex.query_cosmul)
    with pytest.raises(NotImplementedError):
        RestrictedWordIndex.batch_query_cosmul(None, 1, [])
    with pytest.raises(NotImplementedError):
        RotatedWordIndex.batch_query_cosmul(None, 1, [])
