"""`query-words -x/--expressions` (gulon_amd/cli.py) against a stub index: no GPU."""
import io

from gulon_amd import cli
from gulon_amd.expressions import Expression, Term


class _Result:
    def __init__(self, words):
        self.words = words


class StubIndex:
    """Knows the words a, b, c and `a - b`.  An expression is answered with its own terms spelled out, k times; a word
    with "word:" + the word."""
    WORDS = {"a", "b", "c", "a - b", "e-mail"}

    def __init__(self, metric="l2", tag="", log=None):
        self.metric, self.tag, self.log = metric, tag, [] if log is None else log

    def refined(self, vectors, candidates):
        self.log.append(("refined", vectors, candidates))
        return StubIndex(self.metric, "refined:", self.log)

    def batch_query_by_words(self, k, words):
        self.log.append(("words", list(words)))
        return [_Result([self.tag + "word:" + w] * k) if w in self.WORDS else None for w in words]

    def batch_query_expressions(self, k, expressions):
        expressions = list(expressions)
        self.log.append(("expressions", expressions))
        out = []
        for e in expressions:
            assert isinstance(e, Expression)
            spelled = "".join(("+" if t.weight > 0 else "-") + t.key for t in e)
            out.append(_Result([self.tag + spelled] * k) if all(t.key in self.WORDS for t in e) else None)
        return out


def _run(argv, stdin):
    out, stub = io.BytesIO(), StubIndex()
    rc = cli.main(argv, stdin=io.BytesIO(stdin), stdout=out, load=lambda path: stub,
                  vectors=lambda path, normalize: "vectors of " + path)
    return rc, out.getvalue().decode("utf-8"), stub.log


def test_expression_lines_in_input_order():
    rc, out, log = _run(["query-words", "-i", "idx", "-k", "2", "-x"], b"a - b + c\nb\na + zebra\nc - c\n")
    assert rc == 0
    assert out == ("a - b + c: +a-b+c,+a-b+c\n"
                   "b: +b,+b\n"
                   "a + zebra: not found\n"
                   "c - c: +c-c,+c-c\n")
    assert [kind for kind, _ in log] == ["expressions"]
    assert log[0][1][0] == Expression((Term("a", 1.0), Term("b", -1.0), Term("c", 1.0)))


def test_invalid_lines_are_answered_in_place():
    lines = ["a + b", "", "+ a", "a -", "a + - b", "a b", "zebra", "e-mail - a", "   "]
    rc, out, log = _run(["query-words", "--index", "idx", "--expressions"], "\n".join(lines).encode() + b"\n")
    assert rc == 0
    assert out.splitlines() == ["a + b: +a+b", ": invalid expression", "+ a: invalid expression",
                                "a -: invalid expression", "a + - b: invalid expression", "a b: invalid expression",
                                "zebra: not found", "e-mail - a: +e-mail-a", "   : invalid expression"]
    # only the valid ones reach the index, in order
    assert [[t.key for t in e] for e in log[0][1]] == [["a", "b"], ["zebra"], ["e-mail", "a"]]


def test_only_invalid_lines():
    rc, out, log = _run(["query-words", "-i", "idx", "-x"], b"+\n")
    assert rc == 0 and out == "+: invalid expression\n"


def test_without_the_flag_a_line_is_one_word():
    rc, out, log = _run(["query-words", "-i", "idx", "-k", "1"], b"a - b\na + b\n")
    assert rc == 0 and out == "a - b: word:a - b\na + b: not found\n"
    assert log == [("words", ["a - b", "a + b"])]


def test_together_with_refinement():
    rc, out, log = _run(["query-words", "-i", "idx", "-k", "1", "-x", "-v", "vec.txt", "-c", "40"], b"a - b\n")
    assert rc == 0 and out == "a - b: refined:+a-b\n"
    assert log[0] == ("refined", "vectors of vec.txt", 40) and log[1][0] == "expressions"


def test_the_query_command_has_no_such_flag(tmp_path, capsys):
    import pytest
    path = tmp_path / "q.txt"
    path.write_text("1 2\nx 0 1\n")
    with pytest.raises(SystemExit) as e:
        _run(["query", "-i", "idx", "-x", str(path)], b"")
    assert e.value.code == 2


def test_chunks_keep_the_order(monkeypatch):
    monkeypatch.setattr(cli, "CHUNK", 2)
    rc, out, log = _run(["query-words", "-i", "idx", "-x"], b"a\n+\nb\nzebra\nc\n")
    assert out.splitlines() == ["a: +a", "+: invalid expression", "b: +b", "zebra: not found", "c: +c"]
    assert len([1 for kind, _ in log if kind == "expressions"]) == 3
