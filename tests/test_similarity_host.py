"""The host side of the similarity command (gulon_amd/similarity.py, gulon_amd/cli.py): the pairs reader, the numpy
references of the rank sums against a plain average-rank Spearman, the report over stub targets, and the command against
stubs.  No GPU."""
import io
import math

import numpy as np
import pytest

from gulon_amd import cli, similarity
from gulon_amd.similarity import (SectionRho, SimilarityReport, evaluate_pairs, pair_distance_reference,
                                  rank_sums_reference, read_pairs, spearman)


# ---- the reader --------------------------------------------------------------------------------------------------------

def test_read_pairs_sections_comments_and_lowercase():
    lines = ["# WordSim-353", "", "Tiger Cat 7.35", "  tiger\ttiger  10 ", ": SimLex 999 ", "   ", "old New 1.58",
             "#smart intelligent 9.2", ": empty", ":", "a b -1e0"]
    assert read_pairs(lines) == [("", [("Tiger", "Cat", 7.349999904632568), ("tiger", "tiger", 10.0)]),
                                 ("SimLex 999", [("old", "New", 1.5800000429153442)]), ("empty", []),
                                 ("", [("a", "b", -1.0)])]
    low = read_pairs(lines, lowercase=True)
    assert low[0][1][0][:2] == ("tiger", "cat") and low[1] == ("SimLex 999", [("old", "new", 1.5800000429153442)])
    assert read_pairs([]) == [] and read_pairs(["# nothing", ""]) == []


@pytest.mark.parametrize("bad", ["tiger cat", "tiger cat 7.35 x", "tiger cat nan", "tiger cat inf", "tiger cat -Infinity",
                                 "tiger cat 1e39", "tiger cat seven"])
def test_read_pairs_names_the_line_of_a_bad_pair(bad):
    with pytest.raises(ValueError, match=r"line 4\b"):
        read_pairs([": s", "a b 1", "", bad, "c d 2"])


# ---- the references ------------------------------------------------------------------------------------------------------

def test_pair_distance_reference_is_one_running_float32_sum():
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal((5, 37)).astype(np.float32), rng.standard_normal((5, 37)).astype(np.float32)
    got = pair_distance_reference(a, b)
    for i in range(5):
        acc = np.float32(0)
        for e in range(37):
            t = np.float32(a[i, e] - b[i, e])
            acc = np.float32(acc + np.float32(t * t))
        assert got[i].view(np.uint32) == acc.view(np.uint32)
    assert pair_distance_reference(a[0], b[0]).view(np.uint32) == got[0].view(np.uint32)
    assert pair_distance_reference(a, a).view(np.uint32).tolist() == [0] * 5          # +0, not -0
    assert pair_distance_reference(np.zeros((3, 0)), np.zeros((3, 0))).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        pair_distance_reference(a, b[:4])


def _average_ranks(v):
    """1-based ranks, ties sharing the mean of the places they take: plain Python"""
    order = sorted(range(len(v)), key=lambda i: v[i])
    ranks, i = [0.0] * len(v), 0
    while i < len(order):
        j = i
        while j + 1 < len(order) and v[order[j + 1]] == v[order[i]]:
            j += 1
        for t in range(i, j + 1):
            ranks[order[t]] = (i + j) / 2 + 1
        i = j + 1
    return ranks


def _plain_spearman(x, y):
    """Pearson's correlation of the average ranks, in float64; nan for a constant list"""
    rx, ry = _average_ranks(x), _average_ranks(y)
    n = len(x)
    mx, my = sum(rx) / n, sum(ry) / n
    sxy = sum((a - mx) * (b - my) for a, b in zip(rx, ry))
    sxx, syy = sum((a - mx) ** 2 for a in rx), sum((b - my) ** 2 for b in ry)
    return math.nan if sxx * syy == 0 else sxy / math.sqrt(sxx * syy)


def test_rank_sums_and_spearman_against_plain_average_ranks():
    rng = np.random.default_rng(2)
    n = 400
    x = rng.integers(0, 11, n).astype(np.float32)                 # integer scores 0 to 10: ties everywhere
    y = (x + rng.integers(-3, 4, n)).astype(np.float32)
    section = rng.integers(0, 3, n).astype(np.int32)              # interleaved sections 0, 1, 2
    section[rng.choice(n, 7, replace=False)] = 3                  # 3: a constant x
    x[section == 3] = 4.0
    section[0] = 4                                                # 4: one pair
    x[[10, 11]], y[12] = np.nan, np.nan                           # dropped where they stand
    x[13], section[13] = np.inf, 1                                # an infinity ranks last
    section[14], section[15] = 7, -1                              # two pairs of no section
    out = rank_sums_reference(x, y, section, 6)
    assert out.dtype == np.int64 and out.shape == (6, 5)
    live = ~(np.isnan(x) | np.isnan(y))
    for s in range(6):
        at = np.flatnonzero((section == s) & live)
        assert out[s, 0] == len(at) and out[s, 4] == int(((section == s) & ~live).sum())
        want = _plain_spearman(x[at].tolist(), y[at].tolist()) if len(at) else math.nan
        got = spearman(*out[s, 1:4])
        if s in (3, 4, 5):
            assert math.isnan(got) and math.isnan(want)
        else:
            assert abs(got - want) < 1e-12
        # the sums themselves: twice the centred ranks, squared and multiplied
        if len(at):
            cx = [round(2 * (r - (len(at) + 1) / 2)) for r in _average_ranks(x[at].tolist())]
            cy = [round(2 * (r - (len(at) + 1) / 2)) for r in _average_ranks(y[at].tolist())]
            assert out[s, 1:4].tolist() == [sum(a * b for a, b in zip(cx, cy)), sum(a * a for a in cx),
                                            sum(b * b for b in cy)]
    assert out[:, 4].sum() == 3 and out[:, 0].sum() == n - 5 and out[4].tolist() == [1, 0, 0, 0, 0]
    pooled = rank_sums_reference(x, y, None, 1)
    assert pooled[0, 0] == n - 3 and abs(spearman(*pooled[0, 1:4]) - _plain_spearman(x[live].tolist(), y[live].tolist())) < 1e-12
    with pytest.raises(ValueError):
        rank_sums_reference(x, y, None, 2)


def test_zeros_tie_and_spearman_edges():
    out = rank_sums_reference([-0.0, 0.0, 1.0], [5.0, 5.0, 6.0], None, 1)[0]
    assert out.tolist() == [3, 6, 6, 6, 0] and spearman(*out[1:4]) == 1.0             # c = -1, -1, 2 on both sides
    assert math.isnan(spearman(0, 0, 5)) and math.isnan(spearman(0, 5, 0)) and spearman(-6, 4, 9) == -1.0
    big = (1 << 59) + 1                                           # the product is taken in Python integers
    assert spearman(big, big, big) == 1.0 and spearman(np.int64(-big), np.int64(big), np.int64(big)) == -1.0


# ---- the report ------------------------------------------------------------------------------------------------------------

def test_report_lines_negate_rho():
    r = SimilarityReport([SectionRho("wordsim", 353, 12, 0, -6532, 10000, 10000), SectionRho("", 2, 0, 1, 1, 1, 1),
                          SectionRho("flat", 5, 0, 0, 0, 0, 40), SectionRho("zero", 4, 0, 0, 0, 20, 20)],
                         SectionRho("total", 364, 12, 1, -1, 2, 2))
    assert r.lines() == ["wordsim: rho 0.6532 (n = 353, skipped 12, dropped 0)", ": rho -1.0000 (n = 2, skipped 0, dropped 1)",
                         "flat: rho nan (n = 5, skipped 0, dropped 0)", "zero: rho 0.0000 (n = 4, skipped 0, dropped 0)",
                         "total: rho 0.5000 (n = 364, skipped 12, dropped 1)"]


class StubTarget:
    """row_of and lookup over a dictionary of vectors"""

    def __init__(self, vectors):
        self.vectors = {w: np.asarray(v, np.float32) for w, v in vectors.items()}
        self.words = sorted(self.vectors)

    def row_of(self, word):
        return self.words.index(word) if word in self.vectors else None

    def lookup(self, word):
        return self.vectors.get(word)


def _stub_world(monkeypatch):
    """The two native calls behind evaluate_pairs replaced by their numpy references; -> (target, log of the route)."""
    target = StubTarget({"a": [0, 0], "b": [1, 0], "c": [0, 3], "d": [4, 4], "e": [np.nan, 0]})
    log = []

    def host_sums(x, y, section=None, nsections=1):
        log.append("generic")
        return rank_sums_reference(x, y, section, nsections)

    def device_sums(distances, a, b, y, sec, nsections):
        log.append("device")
        x = distances(a, b)
        return np.concatenate([rank_sums_reference(x, y, sec, nsections), rank_sums_reference(x, y, None, 1)])

    def device_distances(t):
        rows = np.stack([t.vectors[w] for w in t.words])
        return lambda a, b: pair_distance_reference(rows[a], rows[b])
    monkeypatch.setattr(similarity, "rank_sums", host_sums)
    monkeypatch.setattr(similarity, "_sums_on_device", device_sums)
    monkeypatch.setattr(similarity, "_device_distances", device_distances)
    return target, log


def test_evaluate_pairs_over_a_stub_target(monkeypatch):
    target, log = _stub_world(monkeypatch)
    sections = [("near is high", [("a", "b", 9.0), ("a", "c", 5.0), ("a", "d", 1.0), ("a", "zzz", 3.0), ("zzz", "a", 3.0)]),
                ("near is low", [("a", "b", 1.0), ("a", "c", 5.0), ("b", "d", 9.0), ("a", "e", 2.0)]),
                ("absent", [("x", "y", 1.0)]), ("empty", [])]
    device = evaluate_pairs(target, sections)
    generic = evaluate_pairs(target, iter(sections), route="generic")
    assert log == ["device", "generic", "generic"] and device == generic
    assert device.lines() == ["near is high: rho 1.0000 (n = 3, skipped 2, dropped 0)",
                              "near is low: rho -1.0000 (n = 3, skipped 0, dropped 1)",
                              "absent: rho nan (n = 0, skipped 1, dropped 0)", "empty: rho nan (n = 0, skipped 0, dropped 0)",
                              "total: rho 0.1231 (n = 6, skipped 3, dropped 1)"]       # 2 / sqrt(16.5 * 16)
    # distances 1, 9, 32 | 1, 9, 25 against scores 9, 5, 1 | 1, 5, 9: the pooled ranks by hand
    assert device.total.rho == 0.0 - similarity.spearman(*rank_sums_reference(
        [1, 9, 32, 1, 9, 25], [9, 5, 1, 1, 5, 9], None, 1)[0, 1:4])
    one = evaluate_pairs(target, sections[:1])                      # one section: the total is that section
    assert one.lines()[1] == "total: rho 1.0000 (n = 3, skipped 2, dropped 0)"
    none = evaluate_pairs(target, sections[2:])
    assert none.lines()[-1] == "total: rho nan (n = 0, skipped 1, dropped 0)" and evaluate_pairs(target, []).sections == []
    with pytest.raises(ValueError, match="unknown route"):
        evaluate_pairs(target, sections, route="device")


def test_only_a_plain_word_index_or_an_exact_one_takes_the_device_route():
    from gulon_amd.exact import ExactWordIndex
    from gulon_amd.word_index import RestrictedWordIndex, WordIndex

    class Inner:
        def pair_distances_dev(self, *args):
            return None
    for cls, device in ((WordIndex, True), (ExactWordIndex, True), (RestrictedWordIndex, False), (StubTarget, False)):
        target = object.__new__(cls)
        target.index = Inner()
        assert (similarity._device_distances(target) is not None) == device, cls


# ---- the command, against stubs ----------------------------------------------------------------------------------------------

def _report():
    return SimilarityReport([SectionRho("wordsim", 353, 12, 0, -6532, 10000, 10000)], SectionRho("total", 353, 12, 0, -1, 2, 2))


class StubIndex:
    metric = "cosine"

    def __init__(self, tag="plain", log=None):
        self.tag, self.log = tag, [] if log is None else log

    def exact(self, vectors):
        self.log.append(("exact", vectors))
        return StubIndex("exact", self.log)


def _run(argv, similarity=None, **kw):
    out, stub, seen = io.BytesIO(), StubIndex(), []

    def default(config, load, vectors):
        seen.append(config)
        return _report()
    rc = cli.main(["similarity"] + argv, stdout=out, load=lambda path: stub,
                  vectors=lambda path, normalize: ("vectors of " + path, normalize),
                  similarity=similarity if similarity is not None else default, **kw)
    return rc, out.getvalue().decode("utf-8"), seen, stub


def test_parser_defaults_and_options():
    rc, out, seen, _ = _run(["-i", "idx", "pairs.txt"])
    assert rc == 0 and seen == [cli.SimilarityConfig("idx", "pairs.txt", False, None, False)]
    assert out == "wordsim: rho 0.6532 (n = 353, skipped 12, dropped 0)\ntotal: rho 0.5000 (n = 353, skipped 12, dropped 0)\n"
    rc, _, seen, _ = _run(["-i", "idx", "--lowercase", "-v", "vec.txt", "--exact", "pairs.txt"])
    assert seen == [cli.SimilarityConfig("idx", "pairs.txt", True, "vec.txt", True)]
    with pytest.raises(Exception):
        seen[0].exact = False                                     # frozen


@pytest.mark.parametrize("argv,message", [
    (["-i", "idx", "--exact", "p.txt"], "--exact needs -v/--vectors"),
    (["-i", "idx", "-v", "vec.txt", "p.txt"], "--vectors is only applicable with --exact"),
    (["-i", "idx", "-R", "rot.bin", "p.txt"], "unrecognized arguments"),
    (["-i", "idx", "-c", "5", "p.txt"], "unrecognized arguments"),
    (["-i", "idx", "-k", "5", "p.txt"], "unrecognized arguments"),
    (["p.txt"], "required"), (["-i", "idx"], "required")])
def test_parser_rules(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        _run(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_run_similarity_picks_the_target(tmp_path, monkeypatch):
    path = tmp_path / "pairs.txt"
    path.write_bytes(b"# header\r\n: s\r\nTiger Cat 7.5\r\n")
    calls = []
    monkeypatch.setattr(similarity, "evaluate_pairs", lambda target, sections: calls.append((target.tag, sections)) or _report())
    for extra, tag, log in (([], "plain", []), (["-v", "vec.txt", "--exact"], "exact", [("exact", ("vectors of vec.txt", True))])):
        rc, out, _, stub = _run(["-i", "idx", "--lowercase"] + extra + [str(path)], similarity=cli.run_similarity)
        assert rc == 0 and out.splitlines()[-1].startswith("total: rho ")
        assert stub.log == log and calls.pop() == (tag, [("s", [("tiger", "cat", 7.5)])])


def test_errors_are_reported_not_raised(tmp_path, capsys):
    bad = tmp_path / "bad.txt"
    bad.write_text(": s\na b 1\na b\n")
    rc, out, _, _ = _run(["-i", "idx", str(bad)], similarity=cli.run_similarity)
    err = capsys.readouterr().err
    assert rc == 1 and out == "" and err.startswith("error: ") and "bad.txt: line 3" in err
    rc, out, _, _ = _run(["-i", "idx", str(tmp_path / "absent.txt")], similarity=cli.run_similarity)
    err = capsys.readouterr().err
    assert rc == 1 and out == "" and err.startswith("error: ") and "absent.txt" in err

    def lacking(config, load, vectors):
        raise cli.SimilarityError("the index holds the word 'x', the word vectors do not")
    rc, out, _, _ = _run(["-i", "idx", "-v", "vec.txt", "--exact", str(bad)], similarity=lacking)
    assert rc == 1 and out == "" and capsys.readouterr().err == "error: the index holds the word 'x', the word vectors do not\n"
