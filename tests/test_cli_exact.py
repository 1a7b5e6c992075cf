"""--exact of the query commands (gulon_amd/cli.py) against stubs: no GPU."""
import io

import pytest

from gulon_amd import cli


class _Result:
    def __init__(self, words):
        self.words = words


class StubIndex:
    """Answers every word and vector with "plain"; its exact form answers with "exact"."""

    def __init__(self, metric, tag="plain", log=None):
        self.metric, self.tag, self.log = metric, tag, [] if log is None else log

    def exact(self, vectors):
        self.log.append(("exact", vectors))
        return StubIndex(self.metric, "exact", self.log)

    def refined(self, vectors, candidates):
        self.log.append(("refined", vectors, candidates))
        return StubIndex(self.metric, "refined", self.log)

    def batch_query_by_words(self, k, words):
        return [None if w == "missing" else _Result([self.tag] * k) for w in words]

    def batch_query(self, k, vectors):
        return [_Result([self.tag] * k) for _ in vectors]


def _run(argv, metric="l2", stdin=b"a\nb\n"):
    out, stub, reads = io.BytesIO(), StubIndex(metric), []

    def vectors(path, normalize):
        reads.append((path, normalize))
        return "vectors of " + path
    rc = cli.main(argv, stdin=io.BytesIO(stdin), stdout=out, load=lambda path: stub, vectors=vectors)
    return rc, out.getvalue().decode("utf-8"), stub.log, reads


@pytest.fixture()
def query_file(tmp_path):
    path = tmp_path / "q.txt"
    path.write_text("2 2\nx 0 1\ny 1 0\n")
    return str(path)


def test_the_parser_accepts_exact_with_vectors(query_file):
    for command, tail in (("query-words", []), ("query", [query_file])):
        args = cli._parser().parse_args([command, "-i", "idx", "--exact", "-v", "vec.txt"] + tail)
        assert args.exact and args.vectors == "vec.txt"
        assert not cli._parser().parse_args([command, "-i", "idx"] + tail).exact


@pytest.mark.parametrize("command", ["query-words", "query"])
def test_exact_needs_vectors(command, query_file, capsys):
    with pytest.raises(SystemExit) as e:
        _run([command, "-i", "idx", "--exact", query_file])
    assert e.value.code == 2
    assert "--exact needs -v/--vectors" in capsys.readouterr().err


@pytest.mark.parametrize("extra,named", [(["-c", "50"], "-c/--candidates"), (["-f", "fine.idx"], "-f/--fine"),
                                         (["-r", "words.txt"], "-r/--restrict"), (["-x"], "-x/--expressions"),
                                         (["-R", "rot.bin"], "-R/--rotation")])
def test_exact_refuses_the_other_refinements(extra, named, query_file, capsys):
    commands = ["query-words"] if extra == ["-x"] else ["query-words", "query"]      # -x is query-words' alone
    for command in commands:
        with pytest.raises(SystemExit) as e:
            _run([command, "-i", "idx", "--exact", "-v", "vec.txt"] + extra + [query_file])
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert f"--exact is not applicable with {named}" in err
        assert err.count("error:") == 1                                               # one line saying which


def test_output_lines_are_the_plain_commands(query_file):
    rc, out, log, reads = _run(["query-words", "-i", "idx", "-k", "3", "--exact", "-v", "vec.txt"], stdin=b"a\nmissing\nb\n")
    assert rc == 0 and out == "a: exact,exact,exact\nmissing: not found\nb: exact,exact,exact\n"
    assert log == [("exact", "vectors of vec.txt")] and reads == [("vec.txt", False)]
    plain = _run(["query-words", "-i", "idx", "-k", "3"], stdin=b"a\nmissing\nb\n")[1]
    assert plain == out.replace("exact", "plain")
    rc, out, log, reads = _run(["query", "-i", "idx", "-k", "2", "-v", "vec.txt", "--exact", query_file], metric="cosine")
    assert rc == 0 and out == "x: exact,exact\ny: exact,exact\n"
    assert log == [("exact", "vectors of vec.txt")] and reads == [("vec.txt", True)]   # cosine: the normalised reading
    assert _run(["query", "-i", "idx", "-k", "2", query_file])[1] == out.replace("exact", "plain")


def test_without_exact_the_vectors_refine_as_before():
    rc, out, log, _ = _run(["query-words", "-i", "idx", "-v", "vec.txt"])
    assert rc == 0 and log == [("refined", "vectors of vec.txt", 10)] and out == "a: refined\nb: refined\n"
