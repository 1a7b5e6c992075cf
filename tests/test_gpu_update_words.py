"""WordIndex.update and `python -m gulon_amd update`: words removed, replaced and added on the device (update.hip),
against the host route -- `oracle.pq_encode` of the added vectors, the codes merged with numpy, a natively created
SortedIndex over them -- down to the bytes of the index file."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, bits
from test_gpu_lookup import _word_indexes

pytestmark = pytest.mark.gpu

N_OLD, D, M, K_CENTS = 300, 16, 4, 32


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def _jkey(w):
    return w.encode("utf-16-be", "surrogatepass")               # String.compareTo


def _case(oracle, g, metric):
    """One update over a few hundred words: (old WordIndex, add, remove, expected words, expected codes [m][s], the
    added vectors as a file holds them, their words, their reference codes, the kept words, cents, pq)."""
    from gulon_amd.index_file import dump_index
    from gulon_amd.word_index import WordIndex
    rng = np.random.default_rng(len(metric))
    cents = rng.standard_normal(K_CENTS * D).astype(np.float32)
    pq = g.ProductQuantizer.from_flat(K_CENTS, D, M, cents)
    old_words = [f"w{2 * i:05d}" for i in range(N_OLD)]          # String order = row order
    old_codes = rng.integers(0, K_CENTS, (M, N_OLD)).astype(np.int32)
    coder = pq.coder_factory(N_OLD)
    srt = g.SortedIndex(g.PQIndex(pq, g.EncodedMatrix(coder, [coder.build_code(c) for c in old_codes])), metric)
    wi = WordIndex.load(dump_index(srt, old_words))
    srt.vector_index.close()
    removed = old_words[5:25]                                    # 20 present
    remove = removed[:7] + ["absent-1", "w00001"] + removed[7:] + ["", removed[0]]      # 3 absent, one listed twice
    replaced = old_words[100:110]                                # 10 replaced
    new = [f"w{2 * i + 1:05d}" for i in range(40, 70)] + ["a-first", "z-last", "\U0001F600", "～", "w", "w00010x",
                                                          "W00010", "w00598z", "é", "w00009"]     # 40 new
    add_words = [(replaced + new)[i] for i in rng.permutation(50)]
    raw = rng.standard_normal((50, D)).astype(np.float32)
    # for a cosine index `add` is the normalised reading, as build-index feeds; the CLI reads `raw` and normalises itself
    X = np.stack([oracle.normalize(r) for r in raw]) if metric == "cosine" else raw
    new_codes = oracle.pq_encode(X, M, K_CENTS, cents)
    gone = set(removed) | set(replaced)
    kept = [w for w in old_words if w not in gone]
    source = {w: old_codes[:, r] for r, w in enumerate(old_words) if w not in gone}
    source.update({w: new_codes[:, i] for i, w in enumerate(add_words)})
    words = sorted(source, key=_jkey)
    codes = np.ascontiguousarray(np.stack([source[w] for w in words], axis=1))
    add = g.DeviceWordVectors(add_words, g.DeviceMatrix.from_host(X))
    return wi, add, remove, words, codes, raw, add_words, new_codes, kept, cents, pq


def _host_route(g, pq, words, codes, metric):
    from gulon_amd.word_index import WordIndex
    coder = pq.coder_factory(len(words))
    enc = g.EncodedMatrix(coder, [coder.build_code(c) for c in codes])
    return WordIndex(words, g.SortedIndex(g.PQIndex(pq, enc), metric))


def _same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.words == y.words and x.rows.tolist() == y.rows.tolist() and x.flags == y.flags
            assert np.array_equal(bits(x.distances), bits(y.distances))


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_update_equals_the_host_route(oracle, g, metric, tmp_path):
    from gulon_amd.index_file import dump_index
    from gulon_amd.word_index import WordIndex
    wi, add, remove, words, codes, raw, add_words, new_codes, kept, cents, pq = _case(oracle, g, metric)
    Q = np.random.default_rng(3).standard_normal((6, D)).astype(np.float32)
    probe = [kept[0], add_words[0], "absent", kept[-1], add_words[-1], wi.words[7]]
    before = wi.batch_query(5, Q), wi.batch_query_by_words(5, probe), wi.index.lookup_rows(np.arange(N_OLD))
    up = wi.update(add=add, remove=remove)
    assert (up.added, up.replaced, up.removed, up.ignored) == (40, 10, 20, 3)
    assert up.words == words and len(set(up.words)) == len(up.words) == N_OLD - 20 + 40
    assert [_jkey(w) for w in up.words] == sorted(_jkey(w) for w in up.words)
    assert up.metric == metric and up.size == len(words) and not up._grouped
    # a kept word keeps its code: the same lookup, bit for bit
    old_rows, new_rows = [wi.row_of(w) for w in kept], [up.row_of(w) for w in kept]
    assert None not in old_rows and None not in new_rows
    assert np.array_equal(bits(up.index.lookup_rows(new_rows)), bits(before[2][old_rows]))
    for w in (kept[0], kept[131], kept[-1]):
        assert np.array_equal(bits(up.lookup(w)), bits(wi.lookup(w)))
    # an added or replaced word carries the reference's code of its vector, at its position in `add`
    got = up.index.vector_index.indices()
    assert np.array_equal(got[:, [up.row_of(w) for w in add_words]], new_codes)
    assert np.array_equal(got, codes)
    assert up.lookup("absent-1") is None and all(up.row_of(w) is None for w in remove if w not in add_words)
    # the host route: the same answers and the same file
    host = _host_route(g, pq, words, codes, metric)
    qwords = [kept[3], add_words[5], "nope", add_words[17], kept[200], "\U0001F600", wi.words[10]]
    _same_results(up.batch_query(10, Q), host.batch_query(10, Q))
    _same_results(up.batch_query_by_words(10, qwords), host.batch_query_by_words(10, qwords))
    assert up.query_by_word(3, wi.words[10]) is None             # removed
    data = dump_index(up.index, up.words)
    assert data == dump_index(host.index, host.words)
    loaded = WordIndex.load(data)
    _same_results(loaded.batch_query(10, Q), host.batch_query(10, Q))
    _same_results(loaded.batch_query_by_words(10, qwords), host.batch_query_by_words(10, qwords))
    loaded.close()
    # the original is untouched and usable
    _same_results(wi.batch_query(5, Q), before[0])
    _same_results(wi.batch_query_by_words(5, probe), before[1])
    assert wi.size == N_OLD and not hasattr(wi, "added")
    # the CLI over the same inputs writes the same bytes (cosine: it reads the vectors normalised itself)
    if metric == "cosine":
        index_path, out_path = tmp_path / "old.index", tmp_path / "new.index"
        index_path.write_bytes(dump_index(wi.index, wi.words))
        vec_path, gone_path = tmp_path / "add.vec", tmp_path / "gone.words"
        vec_path.write_text(f"{len(add_words)} {D}\n" + "".join(
            w + " " + " ".join(np.format_float_positional(x, unique=True) for x in v) + "\n"
            for w, v in zip(add_words, raw)), encoding="utf-8")
        gone_path.write_text("".join(w + "\n" for w in remove), encoding="utf-8")
        p = _run_cli(["update", "-i", str(index_path), "-o", str(out_path), "-a", str(vec_path), "-x", str(gone_path)])
        assert p.returncode == 0, p.stderr.decode(errors="replace")
        lines = p.stdout.decode().splitlines()
        assert lines[-1] == "40 added, 10 replaced, 20 removed, 3 ignored"
        assert any("RUNNING:" in l for l in lines) and any("SUCCESS:" in l for l in lines)
        assert out_path.read_bytes() == data
    host.close()
    up.close()
    wi.close()


def _run_cli(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "gulon_amd"] + args, capture_output=True, cwd=ROOT, env=env, timeout=300)


def test_update_edges(oracle, g):
    wi, add, remove, words, codes, raw, add_words, new_codes, kept, cents, pq = _case(oracle, g, "l2")
    only_removed = wi.update(remove=["w00000", "nope"])
    assert only_removed.words == wi.words[1:]
    assert (only_removed.added, only_removed.replaced, only_removed.removed, only_removed.ignored) == (0, 0, 1, 1)
    only_removed.close()
    same = wi.update()
    assert same.words == wi.words and np.array_equal(same.index.vector_index.indices(), wi.index.vector_index.indices())
    same.close()
    # an empty result is a valid index, and can grow again
    empty = wi.update(remove=wi.words)
    assert empty.size == 0 and empty.removed == N_OLD and empty.batch_query(3, np.zeros((2, D), np.float32))[0].words == []
    again = empty.update(add=add)
    assert again.words == sorted(add_words, key=_jkey) and again.added == 50
    assert np.array_equal(again.index.vector_index.indices()[:, [again.row_of(w) for w in add_words]], new_codes)
    again.close()
    empty.close()
    twice = g.DeviceWordVectors(["x", "y", "x"], g.DeviceMatrix.from_host(np.zeros((3, D), np.float32)))
    with pytest.raises(ValueError, match="twice"):
        wi.update(add=twice)
    wrong = g.DeviceWordVectors(["x"], g.DeviceMatrix.from_host(np.zeros((1, D + 2), np.float32)))
    with pytest.raises(ValueError, match="dimensions"):
        wi.update(add=wrong)
    ri = wi.restrict(wi.words[:10])
    with pytest.raises(NotImplementedError, match="restricted"):
        ri.update(remove=["w00000"])
    ri.close()
    wi.close()


def test_update_refuses_a_grouped_index(oracle, g, tmp_path):
    from gulon_amd.index_file import dump_index
    for kind, wx, _, _, _ in _word_indexes(g, oracle):
        if kind == "grouped":
            with pytest.raises(NotImplementedError, match="grouped"):
                wx.update(remove=["a"])
            path, gone = tmp_path / "grouped.index", tmp_path / "gone.words"
            path.write_bytes(dump_index(wx.index, wx.words))
            gone.write_text("a\n")
            p = _run_cli(["update", "-i", str(path), "-o", str(tmp_path / "out.index"), "-x", str(gone)])
            assert p.returncode != 0 and b"update is not supported by the grouped index" in p.stderr
            assert not (tmp_path / "out.index").exists()
        wx.close()
