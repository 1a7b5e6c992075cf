"""`python -m gulon_amd update`: argument handling (gulon_amd/cli.py) against a stub updater, and the word-merge planner
(gulon_amd/update.py) as a pure function: no GPU."""
import io
from types import SimpleNamespace

import pytest

from gulon_amd import cli
from gulon_amd.update import plan_update


def _run(argv, result=None):
    seen = []
    out = io.BytesIO()

    def update(config, write, load):
        seen.append(config)
        return result if result is not None else SimpleNamespace(added=0, replaced=0, removed=0, ignored=0)
    rc = cli.main(argv, stdout=out, update=update)
    return rc, seen, out.getvalue().decode()


def _fails(argv, capsys):
    with pytest.raises(SystemExit) as e:
        _run(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_paths_short_and_long():
    rc, seen, _ = _run(["update", "-i", "in.idx", "-o", "out.idx", "-a", "new.vec", "-x", "gone.txt"])
    assert rc == 0 and seen == [cli.UpdateConfig("in.idx", "out.idx", "new.vec", "gone.txt")]
    _, seen, _ = _run(["update", "--index", "i", "--output", "o", "--add", "a"])
    assert seen == [cli.UpdateConfig("i", "o", "a", None)]
    _, seen, _ = _run(["update", "-i", "i", "-o", "o", "--remove", "x"])
    assert seen == [cli.UpdateConfig("i", "o", None, "x")]


def test_add_or_remove_is_required(capsys):
    assert "at least one of --add and --remove is required" in _fails(["update", "-i", "i", "-o", "o"], capsys)
    _fails(["update", "-o", "o", "-a", "a"], capsys)            # index
    _fails(["update", "-i", "i", "-a", "a"], capsys)            # output


def test_last_line_carries_the_counters():
    rc, _, text = _run(["update", "-i", "i", "-o", "o", "-a", "a"],
                       SimpleNamespace(added=40, replaced=10, removed=20, ignored=3))
    assert rc == 0 and text.splitlines()[-1] == "40 added, 10 replaced, 20 removed, 3 ignored"


def test_update_errors_are_reported_not_raised(capsys):
    def update(config, write, load):
        raise cli.UpdateError("i: update is not supported by the grouped index")
    assert cli.main(["update", "-i", "i", "-o", "o", "-a", "a"], stdout=io.BytesIO(), update=update) == 1
    assert "update is not supported by the grouped index" in capsys.readouterr().err


def _counters(p):
    return p.added, p.replaced, p.removed, p.ignored


OLD = ["apple", "bear", "cat", "dog", "eel"]


def test_plan_add_only_sorts_the_new_words_in():
    p = plan_update(OLD, ["zebra", "ant", "cow"])
    assert p.words == ["ant", "apple", "bear", "cat", "cow", "dog", "eel", "zebra"]
    assert p.take.tolist() == [-2, 0, 1, 2, -3, 3, 4, -1] and p.take.dtype.name == "int32"
    assert _counters(p) == (3, 0, 0, 0)


def test_plan_replacement_takes_the_new_row():
    p = plan_update(OLD, ["cat", "fox"])
    assert p.words == OLD + ["fox"]
    assert p.take.tolist() == [0, 1, -1, 3, 4, -2]
    assert _counters(p) == (1, 1, 0, 0)


def test_plan_remove_then_add_of_the_same_word_is_an_addition():
    p = plan_update(OLD, ["dog"], ["dog", "bear"])
    assert p.words == ["apple", "cat", "dog", "eel"]
    assert p.take.tolist() == [0, 2, -1, 4]
    assert _counters(p) == (1, 0, 2, 0)


def test_plan_absent_removals_are_ignored_and_counted_once():
    p = plan_update(OLD, [], ["nope", "cat", "nope", "", "cat"])
    assert p.words == ["apple", "bear", "dog", "eel"] and p.take.tolist() == [0, 1, 3, 4]
    assert _counters(p) == (0, 0, 1, 2)
    p = plan_update(OLD, ["nope"], ["nope"])                   # absent, removed, then added
    assert p.words == OLD + ["nope"] and _counters(p) == (1, 0, 0, 1)


def test_plan_duplicate_in_add_raises():
    with pytest.raises(ValueError, match="twice"):
        plan_update(OLD, ["fox", "gnu", "fox"])


def test_plan_everything_removed_and_nothing_to_do():
    p = plan_update(OLD, [], OLD)
    assert p.words == [] and p.take.shape == (0,) and _counters(p) == (0, 0, 5, 0)
    p = plan_update([], [], ["a"])
    assert p.words == [] and _counters(p) == (0, 0, 0, 1)
    p = plan_update(OLD)
    assert p.words == OLD and p.take.tolist() == [0, 1, 2, 3, 4]


def test_plan_orders_by_utf16_code_units():
    """String.compareTo: U+1F600 is the surrogate pair D83D DE00 and sorts BEFORE U+FF5E, which code-point order puts
    first."""
    old = ["a", "～"]
    p = plan_update(old, ["\U0001F600", "b"])
    assert p.words == ["a", "b", "\U0001F600", "～"]
    assert p.take.tolist() == [0, -2, -1, 1]
    assert sorted(p.words) != p.words                          # code-point order differs
