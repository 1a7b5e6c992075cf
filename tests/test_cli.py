"""The query commands' argument handling and line reading (gulon_amd/cli.py, command/QueryWords.scala and
command/Query.scala) against a stub index: no GPU."""
import io

import numpy as np
import pytest

from gulon_amd import cli


class _Result:
    def __init__(self, words):
        self.words = words


class StubIndex:
    """Knows the words "a".."e"; the neighbours of a word are the word itself, then the next ones."""
    known = ["a", "b", "c", "d", "e"]

    def __init__(self):
        self.batches = []

    def batch_query_by_words(self, k, words):
        self.batches.append(list(words))
        out = []
        for w in words:
            i = self.known.index(w) if w in self.known else None
            out.append(None if i is None else _Result([self.known[(i + j) % 5] for j in range(k)]))
        return out

    def batch_query(self, k, vectors):
        return [_Result([self.known[int(v[0]) % 5]] * k) for v in vectors]


def _run(argv, stdin=b""):
    out = io.BytesIO()
    stub = StubIndex()
    rc = cli.main(argv, stdin=io.BytesIO(stdin), stdout=out, load=lambda path: stub)
    return rc, out.getvalue().decode("utf-8"), stub


def test_k_must_be_at_least_one(capsys):
    for k in ("0", "-3", "x"):
        with pytest.raises(SystemExit) as e:
            _run(["query-words", "-i", "idx", "-k", k])
        assert e.value.code == 2
    assert "must be at least 1" in capsys.readouterr().err


def test_index_is_required():
    with pytest.raises(SystemExit):
        _run(["query-words"])
    with pytest.raises(SystemExit):
        _run(["query", "-i", "idx"])       # query needs its file


@pytest.mark.parametrize("data,lines", [
    (b"", []), (b"a", ["a"]), (b"a\n", ["a"]), (b"a\r\nb\r\n", ["a", "b"]), (b"a\rb", ["a", "b"]),
    (b"a\n\nb\n", ["a", "", "b"]), (b"\n", [""]), (b"a\r", ["a"]), (b"a\r\n\r\n", ["a", ""]), (b"x\r\r\ny", ["x", "", "y"]),
    ("été\n\U0001F600\n".encode(), ["été", "\U0001F600"]),
])
def test_lines_end_as_readline_ends_them(data, lines):
    assert cli.read_lines(data) == lines


def test_query_words_output_and_order():
    rc, out, stub = _run(["query-words", "-i", "idx", "-k", "2"], b"c\r\nzz\r\n\r\na\nc\n")
    assert rc == 0
    assert out == "c: c,d\nzz: not found\n: not found\na: a,b\nc: c,d\n"
    assert stub.batches == [["c", "zz", "", "a", "c"]]


def test_query_words_default_k_and_file_argument(tmp_path):
    f = tmp_path / "words.txt"
    f.write_bytes(b"e\nb")
    rc, out, _ = _run(["query-words", "-i", "idx", str(f)], b"ignored\n")
    assert out == "e: e\nb: b\n"


def test_query_words_batches_give_the_same_text(monkeypatch):
    words = [("abcdeX"[i % 6]) for i in range(25)]
    data = "\n".join(words).encode()
    _, one, _ = _run(["query-words", "-i", "idx", "-k", "3"], data)
    monkeypatch.setattr(cli, "CHUNK", 4)
    _, chunked, stub = _run(["query-words", "-i", "idx", "-k", "3"], data)
    assert chunked == one and len(stub.batches) == 7
    assert one.splitlines()[5] == "X: not found"


def test_query_reads_word2vec(tmp_path):
    f = tmp_path / "q.vec"
    f.write_text("2 3\nfoo 1 0 0\nbar 3.5 1 1\n")
    rc, out, _ = _run(["query", "-i", "idx", "-k", "2", str(f)])
    assert rc == 0 and out == "foo: b,b\nbar: d,d\n"
