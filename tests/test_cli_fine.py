"""build-fine and -f/--fine of query, query-words and test (gulon_amd/cli.py) against stubs: no GPU."""
import io

import pytest

from gulon_amd import cli


class _Result:
    def __init__(self, words):
        self.words = words


class StubIndex:
    """Answers with its tag; its refined forms answer with "refined" / "fine"."""

    def __init__(self, path, metric="l2", tag="plain", log=None):
        self.path, self.metric, self.tag, self.log = path, metric, tag, [] if log is None else log

    def refined(self, vectors, candidates):
        self.log.append(("refined", vectors, candidates))
        return StubIndex(self.path, self.metric, "refined", self.log)

    def fine_refined(self, fine, candidates):
        self.log.append(("fine", fine.path, candidates))
        return StubIndex(self.path, self.metric, "fine", self.log)

    def restrict(self, words):
        raise AssertionError("-r must not be reached")

    def batch_query_by_words(self, k, words):
        return [_Result([self.tag] * k) for _ in words]

    def batch_query_expressions(self, k, expressions):
        self.log.append(("expressions", len(expressions)))
        return [_Result([self.tag + "-x"] * k) for _ in expressions]

    def batch_query(self, k, vectors):
        return [_Result([self.tag] * k) for _ in vectors]


def _run(argv, metric="l2", stdin=b"a\nb\n"):
    out, log, loads, reads = io.BytesIO(), [], [], []

    def load(path):
        loads.append(path)
        return StubIndex(path, metric, log=log)

    def vectors(path, normalize):
        reads.append((path, normalize))
        return "vectors of " + path
    rc = cli.main(argv, stdin=io.BytesIO(stdin), stdout=out, load=load, vectors=vectors)
    return rc, out.getvalue().decode("utf-8"), log, loads, reads


@pytest.fixture()
def query_file(tmp_path):
    path = tmp_path / "q.txt"
    path.write_text("2 2\nx 0 1\ny 1 0\n")
    return str(path)


# ---- build-fine
def _build(argv):
    seen = []

    def stub(config, write, load):
        seen.append(config)
        write("built\n")
    out = io.BytesIO()
    rc = cli.main(argv, stdout=out, fine=stub, load=lambda path: None)
    return rc, out.getvalue().decode("utf-8"), seen


def test_build_fine_paths_and_defaults():
    rc, out, seen = _build(["build-fine", "-i", "idx", "-v", "vec.txt", "-o", "fine.idx"])
    assert rc == 0 and out == "built\n"
    assert seen == [cli.FineConfig("idx", "vec.txt", "fine.idx", 256, 25, 100)]          # build-index's defaults
    assert seen[0] == cli.FineConfig("idx", "vec.txt", "fine.idx")
    rc, _, seen = _build(["build-fine", "--index", "i", "--vectors", "v", "--output", "o", "--clusters", "1024",
                          "--quantizers", "32", "--max-iters", "7"])
    assert seen == [cli.FineConfig("i", "v", "o", 1024, 32, 7)]
    rc, _, seen = _build(["build-fine", "-i", "i", "-v", "v", "-o", "o", "-k", "16", "-m", "4", "-n", "2"])
    assert seen == [cli.FineConfig("i", "v", "o", 16, 4, 2)]


@pytest.mark.parametrize("argv,message", [
    (["-v", "v", "-o", "o"], "the following arguments are required: -i/--index"),
    (["-i", "i", "-o", "o"], "the following arguments are required: -v/--vectors"),
    (["-i", "i", "-v", "v"], "the following arguments are required: -o/--output"),
    (["-i", "i", "-v", "v", "-o", "o", "-k", "0"], "clusters must be at least 1"),
    (["-i", "i", "-v", "v", "-o", "o", "-k", "65537"], "too many clusters, must be at most 65536"),
    (["-i", "i", "-v", "v", "-o", "o", "-k", "x"], "invalid integer: 'x'"),
    (["-i", "i", "-v", "v", "-o", "o", "-m", "1.5"], "invalid integer: '1.5'"),
    (["-i", "i", "-v", "v", "-o", "o", "-n", "many"], "invalid integer: 'many'"),
])
def test_build_fine_validators_are_those_of_build_index(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        _build(["build-fine"] + argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_build_index_validators_say_the_same(capsys):
    for argv, message in ((["-k", "0"], "clusters must be at least 1"), (["-m", "1.5"], "invalid integer: '1.5'")):
        with pytest.raises(SystemExit):
            cli.main(["build-index", "-d", "l2", "-o", "o"] + argv + ["f"], stdout=io.BytesIO(), build=lambda c, w: None)
        assert message in capsys.readouterr().err


# ---- -f on the query commands
def test_fine_option_reaches_the_fine_refined_index():
    rc, out, log, loads, reads = _run(["query-words", "-i", "idx", "-k", "3", "-f", "fine.idx", "-c", "77"])
    assert rc == 0 and out == "a: fine,fine,fine\nb: fine,fine,fine\n"
    assert log == [("fine", "fine.idx", 77)] and loads == ["idx", "fine.idx"] and reads == []
    rc, out, log, loads, reads = _run(["query-words", "--index", "idx", "--neighbours", "2", "--fine", "f", "--candidates",
                                       "1"], metric="cosine")
    assert out == "a: fine,fine\nb: fine,fine\n" and log == [("fine", "f", 1)] and reads == []


def test_query_command_takes_the_same_option(query_file):
    rc, out, log, loads, reads = _run(["query", "-i", "idx", "-k", "2", "-f", "fine.idx", "-c", "9", query_file])
    assert rc == 0 and out == "x: fine,fine\ny: fine,fine\n"
    assert log == [("fine", "fine.idx", 9)] and loads == ["idx", "fine.idx"] and reads == []


def test_default_is_ten_candidates_per_neighbour(query_file):
    assert _run(["query-words", "-i", "idx", "-k", "7", "-f", "f"])[2] == [("fine", "f", 70)]
    assert _run(["query-words", "-i", "idx", "-f", "f"])[2] == [("fine", "f", 10)]                  # k = 1
    assert _run(["query", "-i", "idx", "-k", "25", "-f", "f", query_file])[2] == [("fine", "f", 250)]


def test_fine_works_with_expressions():
    rc, out, log, _, _ = _run(["query-words", "-i", "idx", "-k", "2", "-f", "f", "-c", "30", "-x"],
                              stdin=b"a - b + c\n+ a\nking\n")
    assert rc == 0
    assert out == "a - b + c: fine-x,fine-x\n+ a: invalid expression\nking: fine-x,fine-x\n"
    assert log == [("fine", "f", 30), ("expressions", 2)]


@pytest.mark.parametrize("command", ["query-words", "query"])
def test_fine_with_vectors_or_restrict_is_a_parser_error(command, query_file, capsys):
    for extra, message in ((["-v", "vec.txt"], "--fine is not applicable with --vectors"),
                           (["-r", "words.txt"], "--fine is not applicable with --restrict")):
        with pytest.raises(SystemExit) as e:
            _run([command, "-i", "idx", "-f", "fine.idx"] + extra + [query_file])
        assert e.value.code == 2
        assert message in capsys.readouterr().err
    for bad in ("0", "-4", "x"):
        with pytest.raises(SystemExit) as e:
            _run([command, "-i", "idx", "-f", "fine.idx", "-c", bad, query_file])
        assert e.value.code == 2
        capsys.readouterr()


@pytest.mark.parametrize("command", ["query-words", "query"])
def test_candidates_alone_keep_their_message(command, query_file, capsys):
    with pytest.raises(SystemExit) as e:
        _run([command, "-i", "idx", "-c", "50", query_file])
    assert e.value.code == 2
    assert "--candidates is only applicable with --vectors" in capsys.readouterr().err


def test_vectors_option_is_untouched():
    rc, out, log, loads, reads = _run(["query-words", "-i", "idx", "-k", "2", "-v", "vec.txt", "-c", "5"], metric="cosine")
    assert out == "a: refined,refined\nb: refined,refined\n"
    assert log == [("refined", "vectors of vec.txt", 5)] and loads == ["idx"] and reads == [("vec.txt", True)]
    rc, out, log, loads, reads = _run(["query-words", "-i", "idx"])
    assert out == "a: plain\nb: plain\n" and log == [] and loads == ["idx"]


# ---- -f on test
def test_recall_command_passes_the_fine_index_on(capsys):
    seen = []

    def stub(config, write, load):
        seen.append(config)
        return {}
    for argv in (["test", "-v", "v", "-i", "i"], ["test", "-v", "v", "-i", "i", "-c", "200"],
                 ["test", "-v", "v", "-i", "i", "-f", "fine.idx", "-c", "1000"],
                 ["test", "-v", "v", "-i", "i", "--fine", "f", "--candidates", "5", "-s", "9", "-e", "0.5"]):
        assert cli.main(argv, stdout=io.BytesIO(), recall=stub) == 0
    assert [(c.candidates, c.fine) for c in seen] == [(None, None), (200, None), (1000, "fine.idx"), (5, "f")]
    assert seen[0] == cli.RecallConfig("v", "i", 1000, 0.0)                            # the four-field form
    assert seen[1] == cli.RecallConfig("v", "i", 1000, 0.0, 200)                       # the five-field form
    assert seen[2] == cli.RecallConfig("v", "i", 1000, 0.0, 1000, "fine.idx")
    assert (seen[3].sample_size, float(seen[3].epsilon)) == (9, 0.5)
    with pytest.raises(SystemExit) as e:
        cli.main(["test", "-v", "v", "-i", "i", "-f", "fine.idx"], stdout=io.BytesIO(), recall=stub)
    assert e.value.code == 2
    assert "--fine needs --candidates" in capsys.readouterr().err


def test_run_recall_refines_against_the_fine_index(monkeypatch):
    """run_recall with a fine index: the loaded index's fine_refined form is what the harness queries; the vectors are
    read once, raw, for the exact neighbours."""
    from gulon_amd import tests_recall, word_vectors
    log, reads = [], []

    class Raw:
        size = 3

        def sorted(self):
            return "sorted raw"

    def read(path, normalize=False):
        reads.append((path, normalize))
        return Raw()

    class Harness:
        def recall_of(self, index, epsilon):
            log.append(("recall_of", index.tag, epsilon))
            return {}

    monkeypatch.setattr(word_vectors, "read_word2vec_device", read)
    monkeypatch.setattr(tests_recall.Tests, "sample", staticmethod(lambda raw, size: Harness()))
    config = cli.RecallConfig("vec.txt", "idx", 7, 0.25, 300, "fine.idx")
    out = cli.run_recall(config, lambda text: None, lambda path: StubIndex(path, "cosine", log=log))
    assert out == {} and reads == [("vec.txt", False)]
    assert log == [("fine", "fine.idx", 300), ("recall_of", "fine", 0.25)]
