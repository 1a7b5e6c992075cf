"""The device ingest of word2vec text (csrc/ingest.hip, word_vectors.read_word2vec_device) against the host reader
(word_vectors.read_word2vec, pinned to Float.parseFloat by tests/test_word_vectors.py): the same words, the same
bits, the same errors -- whatever the chunking -- and WordVectors.sorted with the rows gathered on the device."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def W():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    from gulon_amd import word_vectors
    return word_vectors


def _same(W, tmp_path, text, normalize=False, chunk_bytes=0):
    data = text if isinstance(text, bytes) else text.encode("utf-8")
    path = tmp_path / "vectors.txt"
    path.write_bytes(data)
    want = W.read_word2vec(str(path), normalize)
    for source in (str(path), data):
        got = W.read_word2vec_device(source, normalize, chunk_bytes)
        assert got.words == want.words
        assert got.size == want.size and (got.dimension == want.dimension or want.size == 0)
        assert got.stats.rows == want.size and got.stats.tokens == want.size * got.dimension
        host = got.to_host()
        assert host.data.shape == want.data.shape
        assert np.array_equal(bits(host.data), bits(want.data))
    return got, want


CASES = {
    "header": "3 2\nb 1.5 -2\na 0.1 3e-2\nc 4 5\n",
    "no header, no final newline": "b 1.5 -2\na 0.1 3e-2\nc 4 5",
    "empty lines in the middle and at the end": "b 1.5 -2\n\n\na 0.1 3e-2\n\nc 4 5\n\n\n",
    "header, empty line first": "9 2\n\nb 1.5 -2\n",
    "header that is all there is": "0 7",
    "crlf": "b 1.5 -2\r\na 0.1 3e-2\r\nc 4 5\r\n",
    "crlf header is a data line": "3 2\r\nb 1.5\r\n",
    "extra fields": "3 2\nb 1.5 -2 7 8 9\na 0.1 3e-2 junk\nc 4 5 \n",
    "non-BMP and combining characters": "\U0001F600 1 2\né 3 4\n￿ 5 6\n\U00010000x 7 8\nété 9 10\n",
    "empty word": " 1 2\nx 3 4\n",
    "grammar corners": "a 5. .5 -0 +0.0 1e5 1E-5 0e99 16777217 3.4028235677973366e38 1e39 -1e-60 7.1e-46\n",
    "one column": "a 1\nb 2\n",
    "a long line among short ones": "a " + " ".join(["0.5"] * 3) + "\nb 1 2 3 " + "x" * 5000 + "\nc 4 5 6\n",
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_small_files(W, tmp_path, name):
    _same(W, tmp_path, CASES[name])
    _same(W, tmp_path, CASES[name], chunk_bytes=1)          # every line its own chunk


def test_empty_file(W, tmp_path):
    got, _ = _same(W, tmp_path, "")
    assert got.size == 0


def _rows(rng, n, d, words=None):
    x = rng.uniform(-10, 10, (n, d))
    words = words or [f"w{i}" for i in range(n)]
    return "".join(w + " " + " ".join("%.6f" % v for v in row) + "\n" for w, row in zip(words, x))


def test_many_rows_in_chunks_that_end_inside_lines(W, tmp_path):
    """20 000 x 300 %.6f rows (about 55 MB), copied in steps of 1 000 003 bytes: every step's border falls inside a
    line and is moved back to the line's end.  Nothing in such a file needs the host: no token may be flagged."""
    rng = np.random.default_rng(21)
    text = f"20000 300\n{_rows(rng, 20000, 300)}"
    got, _ = _same(W, tmp_path, text, chunk_bytes=1000003)
    assert got.size == 20000 and got.dimension == 300
    assert got.stats.flagged == 0


def test_flagged_tokens_are_converted_by_the_host(W, tmp_path):
    rng = np.random.default_rng(22)
    lines = _rows(rng, 400, 16).split("\n")[:-1]
    odd = ["NaN", "1e-50", "123456789012345678901234567890", "-Infinity", "0.1000000000000000055511151231257827",
           "1_0", "inf", "\t7", "1.00000005960464477539062500001", "16777217.000000000000000000001"]
    for i, tok in enumerate(odd * 6):
        parts = lines[(i * 7) % len(lines)].split(" ")
        parts[1 + (i * 5) % 16] = tok
        lines[(i * 7) % len(lines)] = " ".join(parts)
    text = "\n".join(lines) + "\n"
    got, _ = _same(W, tmp_path, text, chunk_bytes=4096)
    assert 0 < got.stats.flagged <= len(odd) * 6
    got, _ = _same(W, tmp_path, text.replace("\n", "\r\n"))          # the \r belongs to the last token of each line
    assert got.stats.flagged >= 400


def test_normalize(W, tmp_path):
    """normalize=True: MathUtils.normalize per row on the device = index.normalize on the host (which the host reader
    applies), flagged tokens patched in BEFORE the row is normalised, a zero row giving NaN as on the JVM."""
    from gulon_amd.index import normalize
    rng = np.random.default_rng(23)
    text = _rows(rng, 300, 50) + "zero " + " ".join(["0"] * 50) + "\nodd NaN " + " ".join(["1.5"] * 49) + "\nmid " + \
        " ".join(["123456789012345678901234567890e-29"] + ["0.25"] * 49) + "\n"
    got, want = _same(W, tmp_path, text, normalize=True, chunk_bytes=10000)
    raw = W.read_word2vec_text(text)
    assert np.array_equal(bits(want.data[5]), bits(normalize(raw.data[5])))
    assert got.stats.flagged == 2


@pytest.mark.parametrize("text", [
    "a 1 2 3\nb 4 5\nc 6 7 8\n",                 # too few components
    "a 1 2 3\nb 4 5 6\nc\n",                     # a word alone
    "2 3\na 1 2 3\nb 4 oops 5\nc 1\n",           # a bad token before the short line: the token's error comes first
    "a 1 2 3\nb 4 x\n",                          # a bad token IN the short line
    "a 1 2 3\nb  4 5\n",                         # an empty token
    "a 1 2 3\nb 4 5 NaN\nc 1 2\nd 1\n",
])
def test_errors_are_the_host_readers(W, tmp_path, text):
    with pytest.raises(ValueError) as want:
        W.read_word2vec_text(text)
    for chunk in (0, 1):
        with pytest.raises(ValueError) as got:
            W.read_word2vec_device(text.encode("utf-8"), chunk_bytes=chunk)
        assert str(got.value) == str(want.value) and type(got.value) is type(want.value)


def test_malformed_utf8_is_an_error_as_on_the_host(W, tmp_path):
    data = b"a 1 2\n\xff\xfe 3 4\n"
    (tmp_path / "bad.txt").write_bytes(data)
    with pytest.raises(UnicodeDecodeError):
        W.read_word2vec(str(tmp_path / "bad.txt"))
    with pytest.raises(UnicodeDecodeError):
        W.read_word2vec_device(data)


def test_sorted_on_the_device(W, tmp_path):
    """WordVectors.sorted: String.compareTo order (UTF-16 code units: U+10000 sorts before U+FFFF), rows gathered on
    the device."""
    rng = np.random.default_rng(24)
    words = ["￿", "b", "\U00010000", "a", "\U0001F600z", "", "é", "é", "B", ""] + \
            [f"w{i}" for i in rng.permutation(2000)]
    text = _rows(rng, len(words), 24, words)
    dev = W.read_word2vec_device(text.encode("utf-8"))
    want = W.read_word2vec_text(text).sorted()
    got = dev.sorted()
    assert got.words == want.words and got.words.index("\U00010000") < got.words.index("￿")
    assert np.array_equal(bits(got.to_host().data), bits(want.data))
    for i in (2, 7, 1500):
        assert got.key_index.lookup(want.words[i]) == i
    assert dev.words == words                                    # the unsorted vectors are untouched
