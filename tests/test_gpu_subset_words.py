"""WordIndex.restrict and the -r option of the query commands: neighbours from a list of words only, over a view of
the index gathered on the device (subset.hip) -- against SortedIndex.select and the CPU oracle."""
import io

import numpy as np
import pytest

from conftest import bits
from test_gpu_lookup import _word_indexes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


@pytest.fixture(scope="module")
def indexes(g, oracle):
    out = {kind: (wi, words, look, oq) for kind, wi, words, look, oq in _word_indexes(g, oracle)}
    yield out
    for wi, _, _, _ in out.values():
        wi.close()


def _listed(words):
    """(the restriction as given: absent words, duplicates, no order; the rows it selects)"""
    rows = list(range(100, 1500, 7))
    given = [words[r] for r in reversed(rows)] + ["absent-1", words[107], words[100], "absent-2", ""]
    return given, np.asarray(rows)


def test_restrict_counts_ignored_words_and_answers_from_the_list(g, oracle, indexes):
    wi, words, look, oq = indexes["sorted"]
    given, rows = _listed(words)
    ri = wi.restrict(given)
    assert ri.ignored == 3 and ri.restricted_size == len(rows) and ri.size == wi.size
    assert ri.index.vector_index.rows.tolist() == rows.tolist()
    K = 5
    inside, outside = words[107], words[3]                   # row 3 is not listed
    assert 3 not in rows
    qwords = [outside, "nope", inside, words[1999]]
    got = ri.batch_query_by_words(K, qwords)
    assert got[1] is None and ri.query_by_word(K, "nope") is None
    assert np.array_equal(bits(ri.lookup(outside)), bits(look[3]))
    # SortedIndex.select over the same rows, queried with the parent's decoded vectors
    srt = wi.index.select(rows=rows)
    qrows = [3, 107, 1999]
    direct = srt.batch_query(K, look[qrows])
    # ... and the oracle on the gathered codes
    from test_gpu_subset import _oracle_view
    vi = wi.index.vector_index
    idx = vi.data.indices()
    pq = vi.product_quantizer
    oi, od, oc = _oracle_view(oracle, idx, rows, pq.dimension, pq.num_clusters, pq.flat_centroids(), look[qrows], K)
    for q, (r, e) in enumerate(zip([got[0], got[2], got[3]], direct)):
        assert set(r.rows.tolist()) <= set(rows.tolist())
        assert r.rows.tolist() == e.rows.tolist() and np.array_equal(bits(r.distances), bits(e.distances))
        assert r.words == [words[i] for i in r.rows.tolist()]
        assert np.array_equal(bits(r.distances), bits(od[q, :oc[q]]))
        if r.flags == 0 or (r.flags & 4):
            assert r.rows.tolist() == oi[q, :oc[q]].tolist()
    one = ri.query_by_word(K, outside)
    assert one.words == got[0].words
    # query by vector names the parent's words too
    byvec = ri.batch_query(K, look[qrows])
    assert [r.words for r in byvec] == [r.words for r in (got[0], got[2], got[3])]
    # a restriction of a restriction
    rr = ri.restrict([words[100], words[3], words[114], "absent-3"])
    assert rr.ignored == 2 and rr.index.vector_index.rows.tolist() == [100, 114]
    assert set(rr.query_by_word(2, outside).rows.tolist()) == {100, 114}
    rr.close()
    srt.vector_index.close()
    ri.close()
    assert wi.query_by_word(1, inside) is not None           # the parent is untouched


def test_restrict_limits(g, oracle, indexes):
    wg = indexes["grouped"][0]
    with pytest.raises(NotImplementedError, match="restrict is not supported by the grouped index"):
        wg.restrict(["a"])
    wi, words, look, oq = indexes["sorted"]
    ri = wi.restrict(words[:50])
    with pytest.raises(NotImplementedError, match="expressions"):
        ri.batch_query_expressions(3, [f"{words[1]} + {words[2]}"])
    with pytest.raises(NotImplementedError, match="expressions"):
        ri.query_expression(3, f"{words[1]} - {words[2]}")
    with pytest.raises(NotImplementedError, match="refined"):
        ri.refined(None, 10)
    empty = wi.restrict(["absent"])
    assert empty.ignored == 1 and empty.restricted_size == 0
    assert len(empty.query_by_word(3, words[0])) == 0
    empty.close()
    ri.close()


def test_cli_query_words_restricted(g, oracle, indexes, tmp_path, capsys):
    from gulon_amd import cli
    from gulon_amd.index_file import dump_index
    wi, words, look, oq = indexes["sorted"]
    given, rows = _listed(words)
    path = tmp_path / "sorted.index"
    path.write_bytes(dump_index(wi.index, words))
    rfile = tmp_path / "restrict.words"
    rfile.write_bytes("\n".join(given).encode() + b"\n")
    qwords = [words[3], "not-a-word", words[107]]
    K = 4
    ri = wi.restrict(given)
    want = "".join(f"{w}: not found\n" if r is None else f"{w}: {','.join(r.words)}\n"
                   for w, r in zip(qwords, ri.batch_query_by_words(K, qwords))).encode()
    ri.close()
    out = io.BytesIO()
    assert cli.main(["query-words", "-i", str(path), "-k", str(K), "-r", str(rfile)],
                    stdin=io.BytesIO("\n".join(qwords).encode()), stdout=out) == 0
    assert out.getvalue() == want
    assert "3 of " in capsys.readouterr().err
    listed = {words[r] for r in rows}
    for line in out.getvalue().decode().splitlines():
        if not line.endswith("not found"):
            assert set(line.split(": ")[1].split(",")) <= listed
    # query: vectors from a word2vec text file
    vecs = look[[1, 300]]
    vfile = tmp_path / "q.vec"
    vfile.write_text("2 16\n" + "".join(f"q{i} " + " ".join(np.format_float_positional(x, unique=True) for x in v) + "\n"
                                        for i, v in enumerate(vecs)))
    ri = wi.restrict(given)
    want = "".join(f"q{i}: {','.join(r.words)}\n" for i, r in enumerate(ri.batch_query(K, vecs))).encode()
    ri.close()
    out = io.BytesIO()
    assert cli.main(["query", "-i", str(path), "-k", str(K), "--restrict", str(rfile), str(vfile)], stdout=out) == 0
    assert out.getvalue() == want
