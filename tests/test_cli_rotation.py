"""-R/--rotation of every command (gulon_amd/cli.py) against stubs: where it is accepted, in which order the loaded index
is wrapped and refined, and that without -R no call changes.  No GPU."""
import io

import numpy as np
import pytest

from gulon_amd import cli
from gulon_amd.rotation import RotatedWordIndex


class _Result:
    def __init__(self, words):
        self.words = words


class StubVectors:
    matrix, size = None, 3

    def __init__(self, path, dimension=2, rotated_by=None):
        self.path, self.dimension, self.rotated_by = path, dimension, rotated_by

    def sorted(self):
        return self


class StubRotation:
    def __init__(self, path, log, dimension=2):
        self.path, self.log, self.dimension = path, log, dimension

    def apply(self, x):
        self.log.append(("apply", self.path, np.asarray(x).shape))
        return x

    def rotate_word_vectors(self, vectors):
        self.log.append(("rotate", self.path, vectors.path))
        return StubVectors(vectors.path, vectors.dimension, self.path)


class StubIndex:
    """Answers with its tag; its restricted and refined forms answer with "restricted" / "refined" / "fine"."""
    dimension, ignored = 2, 0

    def __init__(self, path, metric="l2", tag="plain", log=None):
        self.path, self.metric, self.tag, self.log = path, metric, tag, [] if log is None else log

    def refined(self, vectors, candidates):
        self.log.append(("refined", vectors.path, vectors.rotated_by, candidates))
        return StubIndex(self.path, self.metric, "refined", self.log)

    def fine_refined(self, fine, candidates):
        self.log.append(("fine", fine.path, type(fine).__name__, candidates))
        return StubIndex(self.path, self.metric, "fine", self.log)

    def restrict(self, words):
        self.log.append(("restrict", tuple(words)))
        return StubIndex(self.path, self.metric, "restricted", self.log)

    def batch_query_by_words(self, k, words):
        self.log.append(("by_words", self.tag))
        return [_Result([self.tag] * k) for _ in words]

    def batch_query_expressions(self, k, expressions):
        self.log.append(("expressions", self.tag, len(expressions)))
        return [_Result([self.tag + "-x"] * k) for _ in expressions]

    def batch_query(self, k, vectors):
        self.log.append(("by_vectors", self.tag))
        return [_Result([self.tag] * k) for _ in vectors]


def _run(argv, metric="l2", stdin=b"a\nb\n"):
    out, log = io.BytesIO(), []

    def load(path):
        log.append(("load", path))
        return StubIndex(path, metric, log=log)

    def vectors(path, normalize):
        log.append(("read", path, normalize))
        return StubVectors(path)

    def rotation(path):
        log.append(("rotation", path))
        return StubRotation(path, log)
    rc = cli.main(argv, stdin=io.BytesIO(stdin), stdout=out, load=load, vectors=vectors, rotation=rotation)
    return rc, out.getvalue().decode("utf-8"), log


@pytest.fixture()
def query_file(tmp_path):
    path = tmp_path / "q.txt"
    path.write_text("2 2\nx 0 1\ny 1 0\n")
    return str(path)


# ---- the query commands
def test_rotation_wraps_the_loaded_index_before_anything_else():
    rc, out, log = _run(["query-words", "-i", "idx", "-k", "2", "-R", "r.rot"])
    assert rc == 0 and out == "a: plain,plain\nb: plain,plain\n"
    assert log == [("load", "idx"), ("rotation", "r.rot"), ("by_words", "plain")]        # by word: nothing is rotated
    rc, out, log = _run(["query-words", "--index", "idx", "--rotation", "r.rot"])
    assert out == "a: plain\nb: plain\n" and ("rotation", "r.rot") in log


def test_query_vectors_are_rotated_on_their_way_in(query_file):
    rc, out, log = _run(["query", "-i", "idx", "-k", "2", "-R", "r.rot", query_file])
    assert rc == 0 and out == "x: plain,plain\ny: plain,plain\n"
    assert log == [("load", "idx"), ("rotation", "r.rot"), ("apply", "r.rot", (2, 2)), ("by_vectors", "plain")]


def test_vectors_are_rotated_once_and_the_refined_form_is_wrapped_again(query_file):
    rc, out, log = _run(["query-words", "-i", "idx", "-k", "2", "-R", "r.rot", "-v", "vec.txt", "-c", "5"], metric="cosine")
    assert out == "a: refined,refined\nb: refined,refined\n"
    assert log == [("load", "idx"), ("rotation", "r.rot"), ("read", "vec.txt", True), ("rotate", "r.rot", "vec.txt"),
                   ("refined", "vec.txt", "r.rot", 5), ("by_words", "refined")]
    rc, out, log = _run(["query", "-i", "idx", "-R", "r.rot", "-v", "vec.txt", query_file])
    assert out == "x: refined\ny: refined\n"
    assert log == [("load", "idx"), ("rotation", "r.rot"), ("read", "vec.txt", False), ("rotate", "r.rot", "vec.txt"),
                   ("refined", "vec.txt", "r.rot", 10), ("apply", "r.rot", (2, 2)), ("by_vectors", "refined")]


def test_fine_index_is_used_as_it_is(query_file):
    rc, out, log = _run(["query", "-i", "idx", "-k", "2", "-R", "r.rot", "-f", "fine.idx", "-c", "9", query_file])
    assert out == "x: fine,fine\ny: fine,fine\n"
    assert log == [("load", "idx"), ("rotation", "r.rot"), ("load", "fine.idx"), ("fine", "fine.idx", "StubIndex", 9),
                   ("apply", "r.rot", (2, 2)), ("by_vectors", "fine")]


def test_restriction_and_expressions_follow_the_wrapping(tmp_path, capsys):
    words = tmp_path / "words.txt"
    words.write_text("a\nc\n")
    rc, out, log = _run(["query-words", "-i", "idx", "-R", "r.rot", "-r", str(words)])
    assert out == "a: restricted\nb: restricted\n"
    assert log == [("load", "idx"), ("rotation", "r.rot"), ("restrict", ("a", "c")), ("by_words", "restricted")]
    assert "0 of 2 restriction words are not in the index" in capsys.readouterr().err
    rc, out, log = _run(["query-words", "-i", "idx", "-k", "2", "-R", "r.rot", "-x", "-f", "f", "-c", "30"],
                        stdin=b"a - b + c\n+ a\n")
    assert out == "a - b + c: fine-x,fine-x\n+ a: invalid expression\n"
    assert log == [("load", "idx"), ("rotation", "r.rot"), ("load", "f"), ("fine", "f", "StubIndex", 30),
                   ("expressions", "fine", 1)]


def test_every_form_the_commands_query_is_a_rotated_index(monkeypatch, query_file):
    seen = []
    monkeypatch.setattr(cli, "query", lambda index, k, vectors, write: seen.append(index))
    for extra in ([], ["-v", "vec.txt"], ["-f", "fine.idx"]):
        _run(["query", "-i", "idx", "-R", "r.rot"] + extra + [query_file])
    assert [type(i) for i in seen] == [RotatedWordIndex] * 3
    assert [i.inner.tag for i in seen] == ["plain", "refined", "fine"] and {i.rotation.path for i in seen} == {"r.rot"}
    _run(["query", "-i", "idx", query_file])
    assert type(seen[-1]) is StubIndex


def test_a_rotation_of_another_dimension_is_refused():
    with pytest.raises(ValueError, match="rotation of dimension 3 for an index of dimension 2"):
        RotatedWordIndex(StubIndex("idx"), StubRotation("r", [], dimension=3))
    index = RotatedWordIndex(StubIndex("idx"), StubRotation("r", []))
    with pytest.raises(ValueError, match="vectors of dimension 5"):
        index.refined(StubVectors("v", dimension=5), 10)
    with pytest.raises(ValueError, match="query vectors of 3 numbers"):
        index.batch_query(1, np.zeros(3, np.float32))


def test_without_rotation_no_call_changes(query_file):
    rc, out, log = _run(["query-words", "-i", "idx", "-k", "2", "-v", "vec.txt", "-c", "5"], metric="cosine")
    assert out == "a: refined,refined\nb: refined,refined\n"
    assert log == [("load", "idx"), ("read", "vec.txt", True), ("refined", "vec.txt", None, 5), ("by_words", "refined")]
    rc, out, log = _run(["query", "-i", "idx", query_file])
    assert log == [("load", "idx"), ("by_vectors", "plain")]
    rc, out, log = _run(["query-words", "-i", "idx", "-f", "f"])
    assert log == [("load", "idx"), ("load", "f"), ("fine", "f", "StubIndex", 10), ("by_words", "fine")]


# ---- build-index
def _build(argv):
    seen = []
    rc = cli.main(["build-index"] + argv, stdout=io.BytesIO(), build=lambda config, write: seen.append(config))
    return rc, seen


def test_build_index_takes_the_rotation_file_and_its_rounds():
    rc, seen = _build(["-d", "l2", "-o", "out.idx", "vec.txt"])
    assert rc == 0 and seen == [cli.BuildConfig("l2", 256, 25, 100, None, "out.idx", "vec.txt")]    # the seven-field form
    assert (seen[0].rotation, seen[0].rotation_rounds) == (None, 4)
    rc, seen = _build(["-d", "cosine", "-o", "o", "-R", "r.rot", "vec.txt"])
    assert seen == [cli.BuildConfig("cosine", 256, 25, 100, None, "o", "vec.txt", "r.rot", 4)]
    rc, seen = _build(["-d", "l2", "-o", "o", "--rotation", "r.rot", "--rotation-rounds", "0", "-p", "vec.txt"])
    assert (seen[0].rotation, seen[0].rotation_rounds) == ("r.rot", 0) and seen[0].partitioned is not None


def test_rotation_rounds_need_a_rotation(capsys):
    with pytest.raises(SystemExit) as e:
        _build(["-d", "l2", "-o", "o", "--rotation-rounds", "2", "vec.txt"])
    assert e.value.code == 2
    assert "--rotation-rounds is only applicable with --rotation" in capsys.readouterr().err
    for bad in ("-1", "x"):
        with pytest.raises(SystemExit) as e:
            _build(["-d", "l2", "-o", "o", "-R", "r", "--rotation-rounds", bad, "vec.txt"])
        assert e.value.code == 2
        capsys.readouterr()


def test_build_index_help_says_what_partitioned_gets(capsys):
    with pytest.raises(SystemExit):
        cli.main(["build-index", "--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "the rotation is learned for the flat quantizer" in text


def test_run_build_index_learns_writes_rotates_then_builds(monkeypatch, tmp_path):
    from gulon_amd import build, index_file, rotation, word_vectors
    log = []

    class Matrix:
        def close(self):
            log.append("close the unrotated matrix")

    class Read(StubVectors):
        matrix = Matrix()

    class Learned(StubRotation):
        def save(self, path):
            log.append(("save", path))

    def train(matrix, pq_config, rounds, write):
        log.append(("train", type(matrix).__name__, pq_config.num_clusters, pq_config.num_quantizers, rounds))
        return Learned("learned", log), {}

    def build_index(vectors, metric, partitioned, pq_config, write):
        log.append(("build", vectors.rotated_by, metric, partitioned))
        return ["w"], "index"
    monkeypatch.setattr(word_vectors, "read_word2vec_device", lambda path, normalize=False: Read(path))
    monkeypatch.setattr(rotation, "train_rotation", train)
    monkeypatch.setattr(build, "build_index", build_index)
    monkeypatch.setattr(index_file, "dump_index", lambda index, words: b"bytes")
    out = tmp_path / "o.idx"
    cli.run_build_index(cli.BuildConfig("l2", 16, 4, 2, None, str(out), "vec.txt", "r.rot", 3), lambda text: None)
    assert log == [("train", "Matrix", 16, 4, 3), ("save", "r.rot"), ("rotate", "learned", "vec.txt"),
                   "close the unrotated matrix", ("build", "learned", "l2", None)]
    del log[:]
    cli.run_build_index(cli.BuildConfig("l2", 16, 4, 2, None, str(out), "vec.txt"), lambda text: None)
    assert log == [("build", None, "l2", None)] and out.read_bytes() == b"bytes"


# ---- test, inspect, build-fine, update: the vectors file is rotated, the index used as it is
def test_the_other_commands_pass_the_rotation_on():
    seen = []

    def keep(result):
        def stub(config, *rest):
            seen.append(config)
            return result
        return stub

    class Report:
        def lines(self):
            return []

    class Updated:
        added = replaced = removed = ignored = 0
    for rot in ([], ["-R", "r.rot"], ["--rotation", "r.rot"]):
        assert cli.main(["test", "-v", "v", "-i", "i"] + rot, stdout=io.BytesIO(), recall=keep({})) == 0
        assert cli.main(["inspect", "-i", "i", "-v", "v"] + rot, stdout=io.BytesIO(), inspect=keep(Report()),
                        load=None) == 0
        assert cli.main(["build-fine", "-i", "i", "-v", "v", "-o", "o"] + rot, stdout=io.BytesIO(), fine=keep(None)) == 0
        assert cli.main(["update", "-i", "i", "-o", "o", "-a", "v"] + rot, stdout=io.BytesIO(), update=keep(Updated())) == 0
    assert [c.rotation for c in seen] == [None] * 4 + ["r.rot"] * 8
    assert seen[:4] == [cli.RecallConfig("v", "i", 1000, 0.0), cli.InspectConfig("i", "v", 10),
                        cli.FineConfig("i", "v", "o"), cli.UpdateConfig("i", "o", "v", None)]    # the forms without -R


def test_rotation_without_the_vectors_it_rotates_is_a_parser_error(capsys):
    for argv, message in ((["inspect", "-i", "i", "-R", "r"], "--rotation is only applicable with --vectors"),
                          (["update", "-i", "i", "-o", "o", "-x", "w", "-R", "r"],
                           "--rotation is only applicable with --add")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv, stdout=io.BytesIO())
        assert e.value.code == 2
        assert message in capsys.readouterr().err


def test_run_recall_inspect_and_update_rotate_what_they_read(monkeypatch, tmp_path):
    from gulon_amd import index_file, rotation, tests_recall, word_vectors
    log = []

    class Harness:
        def recall_of(self, index, epsilon):
            log.append(("recall_of", index.tag))
            return {}

    class Inner(StubIndex):
        size = 0

        def inspect(self, vectors, worst):
            log.append(("inspect", vectors.rotated_by, worst))
            return "report"

        def update(self, add=None, remove=None):
            log.append(("update", add.rotated_by))
            out = Inner(self.path, log=log)
            out.index, out.words = None, []
            return out
    monkeypatch.setattr(word_vectors, "read_word2vec_device",
                        lambda path, normalize=False: log.append(("read", path, normalize)) or StubVectors(path))
    monkeypatch.setattr(rotation.Rotation, "load", staticmethod(lambda path: StubRotation(path, log)))
    monkeypatch.setattr(tests_recall.Tests, "sample",
                        staticmethod(lambda raw, size: log.append(("sample", raw.rotated_by)) or Harness()))
    monkeypatch.setattr(index_file, "dump_index", lambda index, words: b"")
    load = lambda path: Inner(path, "cosine", log=log)
    cli.run_recall(cli.RecallConfig("vec.txt", "idx", 7, 0.0, 50, None, "r.rot"), lambda text: None, load)
    assert log == [("read", "vec.txt", False), ("rotate", "r.rot", "vec.txt"), ("read", "vec.txt", True),
                   ("rotate", "r.rot", "vec.txt"), ("refined", "vec.txt", "r.rot", 50), ("sample", "r.rot"),
                   ("recall_of", "refined")]
    del log[:]
    cli.run_recall(cli.RecallConfig("vec.txt", "idx", 7, 0.0), lambda text: None, load)
    assert log == [("read", "vec.txt", False), ("sample", None), ("recall_of", "plain")]
    del log[:]
    vectors = lambda path, normalize: StubVectors(path)
    assert cli.run_inspect(cli.InspectConfig("idx", "vec.txt", 3, "r.rot"), load, vectors) == "report"
    assert cli.run_inspect(cli.InspectConfig("idx", "vec.txt", 3), load, vectors) == "report"
    assert log == [("rotate", "r.rot", "vec.txt"), ("inspect", "r.rot", 3), ("inspect", None, 3)]
    del log[:]
    out = str(tmp_path / "o.idx")
    cli.run_update(cli.UpdateConfig("idx", out, "add.txt", None, "r.rot"), lambda text: None, load)
    cli.run_update(cli.UpdateConfig("idx", out, "add.txt"), lambda text: None, load)
    assert log == [("read", "add.txt", True), ("rotate", "r.rot", "add.txt"), ("update", "r.rot"),
                   ("read", "add.txt", True), ("update", None)]
