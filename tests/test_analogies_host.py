"""The host side of the analogies command (gulon_amd/analogies.py, gulon_amd/cli.py): the question reader, the report's
arithmetic and lines, and the command against stubs.  No GPU."""
import io

import pytest

from gulon_amd import cli
from gulon_amd.analogies import AnalogyReport, SectionScore, question_expression, read_questions


def test_read_questions_sections_and_headers():
    lines = [": capital-common-countries", "Athens Greece Baghdad Iraq", "Athens Greece Bangkok Thailand",
             ":  gram1 adjective to adverb ", "amazing amazingly apparent apparently", ": empty"]
    assert read_questions(lines) == [
        ("capital-common-countries", [("Athens", "Greece", "Baghdad", "Iraq"), ("Athens", "Greece", "Bangkok", "Thailand")]),
        ("gram1 adjective to adverb", [("amazing", "amazingly", "apparent", "apparently")]),
        ("empty", [])]


def test_read_questions_without_a_header_and_lowercase():
    lines = ["A b C d", "  e\tf  g h  ", ": Named", "I J K L"]
    assert read_questions(lines) == [("", [("A", "b", "C", "d"), ("e", "f", "g", "h")]), ("Named", [("I", "J", "K", "L")])]
    assert read_questions(lines, lowercase=True) == [("", [("a", "b", "c", "d"), ("e", "f", "g", "h")]),
                                                     ("Named", [("i", "j", "k", "l")])]      # names keep their case
    assert read_questions([]) == []


@pytest.mark.parametrize("bad", ["a b c", "a b c d e", ""])
def test_read_questions_names_the_line_of_a_bad_question(bad):
    with pytest.raises(ValueError, match=r"line 3\b"):
        read_questions([": s", "a b c d", bad, "e f g h"])


def test_the_question_is_b_minus_a_plus_c_in_that_order():
    e = question_expression("man", "king", "woman")
    assert [(t.key, t.weight) for t in e] == [("king", 1.0), ("man", -1.0), ("woman", 1.0)]


def _report():
    return AnalogyReport((1, 5, 10), [SectionScore("family", 506, 12, {1: 370, 5: 410, 10: 431}),
                                      SectionScore("", 3, 0, {1: 0, 5: 1, 10: 3}),
                                      SectionScore("none asked", 0, 7, {1: 0, 5: 0, 10: 0})])


def test_report_totals_and_lines():
    r = _report()
    assert (r.asked, r.skipped, r.hits) == (509, 19, {1: 370, 5: 411, 10: 434})
    assert r.sections[0].accuracy(1) == 370 / 506 and r.sections[2].accuracy(5) == 0.0
    assert r.lines() == ["family: @1 0.7312 @5 0.8103 @10 0.8518 (n = 506, skipped 12)",
                         ": @1 0.0000 @5 0.3333 @10 1.0000 (n = 3, skipped 0)",
                         "none asked: @1 0.0000 @5 0.0000 @10 0.0000 (n = 0, skipped 7)",
                         "total: @1 0.7269 @5 0.8075 @10 0.8527 (n = 509, skipped 19)"]
    assert AnalogyReport((2,), []).lines() == ["total: @2 0.0000 (n = 0, skipped 0)"]


# ---- the command, against stubs ------------------------------------------------------------------------------------------

class StubIndex:
    metric = "cosine"

    def __init__(self, tag="plain", log=None):
        self.tag, self.log = tag, [] if log is None else log

    def exact(self, vectors):
        self.log.append(("exact", vectors))
        return StubIndex("exact", self.log)

    def refined(self, vectors, candidates):
        self.log.append(("refined", vectors, candidates))
        return StubIndex("refined", self.log)


def _run(argv, analogies=None, **kw):
    out, stub, seen = io.BytesIO(), StubIndex(), []

    def default(config, load, vectors):
        seen.append(config)
        return _report()
    rc = cli.main(["analogies"] + argv, stdout=out, load=lambda path: stub,
                  vectors=lambda path, normalize: ("vectors of " + path, normalize),
                  analogies=analogies if analogies is not None else default, **kw)
    return rc, out.getvalue().decode("utf-8"), seen, stub


def test_parser_defaults_and_options():
    rc, out, seen, _ = _run(["-i", "idx", "q.txt"])
    assert rc == 0 and seen == [cli.AnalogiesConfig("idx", "q.txt", (1, 5, 10), False, None, False, None)]
    assert out == "".join(line + "\n" for line in _report().lines()) and out.endswith("skipped 19)\n")
    rc, _, seen, _ = _run(["-i", "idx", "-k", "1,3,100", "--lowercase", "-v", "vec.txt", "-c", "40", "q.txt"])
    assert seen == [cli.AnalogiesConfig("idx", "q.txt", (1, 3, 100), True, "vec.txt", False, 40)]
    rc, _, seen, _ = _run(["-i", "idx", "-v", "vec.txt", "--exact", "q.txt"])
    assert seen == [cli.AnalogiesConfig("idx", "q.txt", (1, 5, 10), False, "vec.txt", True, None)]


@pytest.mark.parametrize("argv,message", [
    (["-i", "idx", "--exact", "q.txt"], "--exact needs -v/--vectors"),
    (["-i", "idx", "-c", "5", "q.txt"], "--candidates is only applicable with --vectors"),
    (["-i", "idx", "-v", "vec.txt", "--exact", "-c", "5", "q.txt"], "--candidates is not applicable with --exact"),
    (["-i", "idx", "-k", "5,1", "q.txt"], "ascending"), (["-i", "idx", "-k", "0,1", "q.txt"], "ascending"),
    (["-i", "idx", "-k", "1,,2", "q.txt"], "invalid list of integers"),
    (["-i", "idx", "-k", ",".join(str(i) for i in range(1, 18)), "q.txt"], "1 to 16"),
    (["-i", "idx", "-f", "fine.idx", "q.txt"], "unrecognized arguments"),
    (["-i", "idx", "-R", "rot.bin", "q.txt"], "unrecognized arguments"),
    (["-i", "idx", "-r", "words.txt", "q.txt"], "unrecognized arguments"),
    (["-i", "idx"], "required")])
def test_parser_rules(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        _run(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_the_help_text_says_what_is_outside_the_command(capsys):
    with pytest.raises(SystemExit):
        _run(["-h"])
    text = " ".join(capsys.readouterr().out.split())
    assert "Not for a rotated index" in text and "--exact" in text


def test_run_analogies_picks_the_target(tmp_path, monkeypatch):
    """run_analogies itself, with the evaluation stubbed: the index alone, refined (default 10 * the largest k, or -c),
    exact; the vectors read normalised for a cosine index."""
    from gulon_amd import analogies
    path = tmp_path / "q.txt"
    path.write_bytes(b": s\r\nA B C D\r\n")
    calls = []
    monkeypatch.setattr(analogies, "evaluate_analogies",
                        lambda target, sections, ks: calls.append((target.tag, sections, ks)) or _report())
    for extra, tag, log in (([], "plain", []),
                            (["-v", "vec.txt"], "refined", [("refined", ("vectors of vec.txt", True), 100)]),
                            (["-v", "vec.txt", "-c", "7"], "refined", [("refined", ("vectors of vec.txt", True), 7)]),
                            (["-v", "vec.txt", "--exact"], "exact", [("exact", ("vectors of vec.txt", True))])):
        rc, out, _, stub = _run(["-i", "idx", "--lowercase"] + extra + [str(path)], analogies=cli.run_analogies)
        assert rc == 0 and out.splitlines()[-1].startswith("total: ")
        assert stub.log == log
        assert calls.pop() == (tag, [("s", [("a", "b", "c", "d")])], (1, 5, 10))


def test_errors_are_reported_not_raised(tmp_path, capsys):
    bad = tmp_path / "bad.txt"
    bad.write_text(": s\na b c d\na b c\n")
    rc, out, _, _ = _run(["-i", "idx", str(bad)], analogies=cli.run_analogies)
    err = capsys.readouterr().err
    assert rc == 1 and out == "" and err.startswith("error: ") and "bad.txt: line 3" in err
    rc, out, _, _ = _run(["-i", "idx", str(tmp_path / "absent.txt")], analogies=cli.run_analogies)
    err = capsys.readouterr().err
    assert rc == 1 and out == "" and err.startswith("error: ") and "absent.txt" in err

    def lacking(config, load, vectors):
        raise cli.AnalogiesError("the index holds the word 'x', the word vectors do not")
    rc, out, _, _ = _run(["-i", "idx", "-v", "vec.txt", "--exact", str(bad)], analogies=lacking)
    assert rc == 1 and out == "" and capsys.readouterr().err == \
        "error: the index holds the word 'x', the word vectors do not\n"
