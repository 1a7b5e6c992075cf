"""-v/--vectors and -c/--candidates of the query commands and -c of `test` (gulon_amd/cli.py) against stubs: no GPU."""
import io

import pytest

from gulon_amd import cli


class _Result:
    def __init__(self, words):
        self.words = words


class StubIndex:
    """Answers every word and vector with "plain"; its refined form answers with "refined"."""

    def __init__(self, metric, tag="plain", log=None):
        self.metric, self.tag, self.log = metric, tag, [] if log is None else log

    def refined(self, vectors, candidates):
        self.log.append(("refined", vectors, candidates))
        return StubIndex(self.metric, "refined", self.log)

    def batch_query_by_words(self, k, words):
        return [_Result([self.tag] * k) for _ in words]

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


@pytest.mark.parametrize("command", ["query-words", "query"])
def test_candidates_without_vectors_is_a_parser_error(command, query_file, capsys):
    with pytest.raises(SystemExit) as e:
        _run([command, "-i", "idx", "-c", "50", query_file])
    assert e.value.code == 2
    assert "--candidates is only applicable with --vectors" in capsys.readouterr().err
    for bad in ("0", "-4", "x"):
        with pytest.raises(SystemExit) as e:
            _run([command, "-i", "idx", "-v", "vec.txt", "-c", bad, query_file])
        assert e.value.code == 2


def test_options_reach_the_refined_index():
    rc, out, log, reads = _run(["query-words", "-i", "idx", "-k", "3", "-v", "vec.txt", "-c", "77"])
    assert rc == 0 and out == "a: refined,refined,refined\nb: refined,refined,refined\n"
    assert log == [("refined", "vectors of vec.txt", 77)] and reads == [("vec.txt", False)]
    rc, out, log, reads = _run(["query-words", "--index", "idx", "--neighbours", "2", "--vectors", "v", "--candidates", "1"],
                               metric="cosine")
    assert out == "a: refined,refined\nb: refined,refined\n"
    assert log == [("refined", "vectors of v", 1)] and reads == [("v", True)]        # cosine: the normalised reading


def test_query_command_takes_the_same_options(query_file):
    rc, out, log, reads = _run(["query", "-i", "idx", "-k", "2", "-v", "vec.txt", "-c", "9", query_file], metric="cosine")
    assert rc == 0 and out == "x: refined,refined\ny: refined,refined\n"
    assert log == [("refined", "vectors of vec.txt", 9)] and reads == [("vec.txt", True)]


def test_default_is_ten_candidates_per_neighbour(query_file):
    assert _run(["query-words", "-i", "idx", "-k", "7", "-v", "vec.txt"])[2] == [("refined", "vectors of vec.txt", 70)]
    assert _run(["query-words", "-i", "idx", "-v", "vec.txt"])[2] == [("refined", "vectors of vec.txt", 10)]    # k = 1
    assert _run(["query", "-i", "idx", "-k", "25", "-v", "vec.txt", query_file])[2] == [("refined", "vectors of vec.txt", 250)]


def test_existing_command_lines_parse_as_before(query_file):
    rc, out, log, reads = _run(["query-words", "-i", "idx", "-k", "2"])
    assert rc == 0 and out == "a: plain,plain\nb: plain,plain\n" and log == [] and reads == []
    rc, out, log, reads = _run(["query", "-i", "idx", query_file])
    assert rc == 0 and out == "x: plain\ny: plain\n" and log == [] and reads == []
    rc, out, _, _ = _run(["query-words", "-i", "idx", query_file])                     # the words of a file
    assert out.count("\n") == 3


def test_recall_command_passes_candidates_on():
    seen = []

    def stub(config, write, load):
        seen.append(config)
        return {}
    for argv in (["test", "-v", "v", "-i", "i"], ["test", "-v", "v", "-i", "i", "-c", "200"],
                 ["test", "-v", "v", "-i", "i", "--candidates", "5", "-s", "9", "-e", "0.5"]):
        assert cli.main(argv, stdout=io.BytesIO(), recall=stub) == 0
    assert [c.candidates for c in seen] == [None, 200, 5]
    assert seen[0] == cli.RecallConfig("v", "i", 1000, 0.0)                            # the old four-field form
    assert (seen[2].sample_size, float(seen[2].epsilon)) == (9, 0.5)
    with pytest.raises(SystemExit) as e:
        cli.main(["test", "-v", "v", "-i", "i", "-c", "0"], stdout=io.BytesIO(), recall=stub)
    assert e.value.code == 2
