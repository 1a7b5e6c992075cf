"""Keys and word2vec text ingest: KeyIndex (KeyIndex.scala:9-62) and
WordVectors.readWord2Vec / sorted / grouped (WordVectors.scala:13-110,141-268).

Host-side conveniences: the native path works on row ids; these classes carry the words next to
them so that a caller of the reference's CLI finds `query(word)` / `(word, distance)` results.
Strings order as on the JVM: String.compareTo compares UTF-16 code units, which differs from
Python's code-point order for characters beyond the BMP."""
import bisect
import codecs
import ctypes as C
import io
import os
import re
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from . import native as N


def _jkey(s):
    """Sort key with java.lang.String.compareTo's order (UTF-16 code units)."""
    return s.encode("utf-16-be", "surrogatepass")


class KeyIndexSorted:
    """KeyIndex.Sorted (KeyIndex.scala:15-29): binary search over keys in String order."""

    def __init__(self, keys):
        self.keys = list(keys)
        self._jk = [_jkey(k) for k in self.keys]

    def __len__(self):
        return len(self.keys)

    def __getitem__(self, i):
        return self.keys[i]

    def lookup(self, key):
        i = bisect.bisect_left(self._jk, _jkey(key))
        return i if i < len(self._jk) and self._jk[i] == _jkey(key) else None


class KeyIndexGrouped:
    """KeyIndex.Grouped (KeyIndex.scala:31-61): keys sorted inside each group; groups tried in order."""

    def __init__(self, keys, group_offsets):
        self.keys = list(keys)
        self.group_offsets = [int(o) for o in group_offsets]
        self._jk = [_jkey(k) for k in self.keys]

    def __len__(self):
        return len(self.keys)

    def __getitem__(self, i):
        return self.keys[i]

    def lookup(self, key):
        jk, frm = _jkey(key), 0
        for to in self.group_offsets + [len(self.keys)]:
            i = bisect.bisect_left(self._jk, jk, frm, to)
            if i < to and self._jk[i] == jk:
                return i
            frm = to
        return None


def parse_float(token):
    """java.lang.Float.parseFloat for the decimal tokens of a word2vec file: the binary32 nearest to
    the decimal value.  float(token) is the nearest binary64; casting that down rounds a second time,
    which is wrong only when the binary64 sits exactly on a binary32 midpoint -- those tokens are
    rounded exactly."""
    x = float(token)
    f = np.float32(x)
    if x != x or x in (float("inf"), float("-inf")) or f in (np.float32("inf"), np.float32("-inf")):
        return f
    # bracket x by neighbouring binary32 values (differences of doubles this close are exact)
    with np.errstate(over="ignore"):
        lo = f if float(f) <= x else np.nextafter(f, np.float32("-inf"))
        hi = np.nextafter(lo, np.float32("inf"))
    if x - float(lo) != float(hi) - x:                 # not a binary32 midpoint: one rounding is enough
        return f
    try:
        exact = Fraction(token.strip())
    except (ValueError, ZeroDivisionError):
        return f
    dl, dh = exact - Fraction(float(lo)), Fraction(float(hi)) - exact
    if dl < dh:
        return np.float32(lo)
    if dh < dl:
        return np.float32(hi)
    return np.float32(lo) if (int(np.float32(lo).view(np.uint32)) & 1) == 0 else np.float32(hi)   # ties to even


_HEADER = re.compile(r"(\d+) (\d+)")


class WordVectors:
    """WordVectors.Unindexed / Sorted (WordVectors.scala:112-126): words[i] belongs to row i."""

    def __init__(self, words, data, key_index=None):
        self.words = list(words)
        self.data = N.f32(data).reshape(len(self.words), -1) if len(self.words) else np.zeros((0, 0), np.float32)
        self.key_index = key_index

    @property
    def size(self):
        return len(self.words)

    @property
    def dimension(self):
        return self.data.shape[1]

    def word(self, i):
        return self.words[i]

    def __getitem__(self, i):
        return self.data[i]

    def sorted(self):
        """WordVectors.sorted (WordVectors.scala:60-71): rows in String order of their words."""
        order = sorted(range(self.size), key=lambda i: _jkey(self.words[i]))
        words = [self.words[i] for i in order]
        return WordVectors(words, self.data[order] if self.size else self.data, KeyIndexSorted(words))

    def grouped(self, clustering):
        """WordVectors.grouped (WordVectors.scala:24-58): rows ordered by (cluster, word); returns
        (GroupedWordVectors, gulon_amd.grouped.GroupedVectors) -- the second is what Index.grouped takes."""
        from .grouped import group
        # parAssign over the rows as they are (:27), THEN the two stable sorts, by word and by cluster (:28-30)
        order = np.asarray(sorted(range(self.size), key=lambda i: _jkey(self.words[i])), np.int64)
        gv = group(self.data, clustering, word_order=order)
        words = [self.words[i] for i in gv.perm]
        return GroupedWordVectors(words, self.data[gv.perm], gv.centroids, gv.offsets), gv


class GroupedWordVectors(WordVectors):
    """WordVectors.Grouped (WordVectors.scala:96-139)."""

    def __init__(self, words, data, centroids, offsets):
        super().__init__(words, data, KeyIndexGrouped(words, offsets))
        self.centroids, self.offsets = centroids, np.asarray(offsets, np.int32)

    def cluster_of(self, i):                                 # WordVectors.scala:108-111
        return int(np.searchsorted(self.offsets, i, side="right"))


def read_word2vec(source, normalize=False):
    """WordVectors.readWord2Vec (WordVectors.scala:141-252): text format, one `word v0 v1 ...` per line,
    optionally preceded by a `count dimension` header line."""
    from .index import normalize as normalize_vec
    own = isinstance(source, (str, bytes))
    fh = open(source, "r", encoding="utf-8", newline="\n") if own else source
    try:
        first = fh.readline()
        if first == "":
            return WordVectors([], np.zeros((0, 0), np.float32))
        line = first[:-1] if first.endswith("\n") else first
        m = _HEADER.fullmatch(line)
        pending = []
        if m:
            dim = int(m.group(2))
        else:
            dim = len(line.split(" ")) - 1
            pending.append(line)
        words, rows = [], []

        def take(ln):
            if ln == "":                                     # an empty line still counts as read, adds nothing
                return
            parts = ln.split(" ")
            vec = np.array([parse_float(t) for t in parts[1:1 + dim]], np.float32)
            if len(vec) != dim:
                raise ValueError(f"expected {dim} components after {parts[0]!r}, found {len(vec)}")
            words.append(parts[0])
            rows.append(normalize_vec(vec) if normalize else vec)

        for ln in pending:
            take(ln)
        for raw in fh:
            take(raw[:-1] if raw.endswith("\n") else raw)
        data = np.stack(rows) if rows else np.zeros((0, dim), np.float32)
        return WordVectors(words, data)
    finally:
        if own:
            fh.close()


def read_word2vec_text(text, normalize=False):
    return read_word2vec(io.StringIO(text, newline="\n"), normalize)


@dataclass(frozen=True)
class IngestStats:
    """What the device ingest met: vector tokens, those of them the kernel flagged for the host, rows."""
    tokens: int
    flagged: int
    rows: int


class DeviceWordVectors:
    """WordVectors whose matrix stays in HBM (matrix.DeviceMatrix); words[i] belongs to row i."""

    def __init__(self, words, matrix, key_index=None, stats=None):
        self.words, self.matrix, self.key_index, self.stats = list(words), matrix, key_index, stats

    @property
    def size(self):
        return len(self.words)

    @property
    def dimension(self):
        return self.matrix.cols if self.matrix is not None else 0

    def word(self, i):
        return self.words[i]

    def _gather(self, order):
        from .matrix import DeviceMatrix
        if self.matrix is None:
            return None
        rows = N.i32(order)
        h = C.c_void_p()
        N.check(N.lib().gulon_dataset_gather(self.matrix._h, rows if rows.size else np.zeros(1, np.int32), rows.size,
                                             C.byref(h)))
        return DeviceMatrix(h, rows.size, self.matrix.cols)

    def _word_order(self):
        return sorted(range(self.size), key=lambda i: _jkey(self.words[i]))

    def sorted(self):
        """WordVectors.sorted (WordVectors.scala:60-71): the order on the host (String.compareTo), the rows gathered
        on the device.  file_rows[i] of the result is the row that sorted row i had here: for vectors as read, its
        line in the file, which in a word2vec file is its frequency rank."""
        order = self._word_order()
        words = [self.words[i] for i in order]
        out = DeviceWordVectors(words, self._gather(order), KeyIndexSorted(words), self.stats)
        out.file_rows = np.asarray(order, np.int64)
        return out

    def grouped(self, clustering, gather=True):
        """WordVectors.grouped (WordVectors.scala:24-58) over grouped.group: (the word vectors in grouped order,
        GroupedVectors with the residuals in HBM).  gather=False leaves the reordered raw rows out (an index build
        needs only the residuals)."""
        from .grouped import group
        gv = group(self.matrix, clustering, word_order=np.asarray(self._word_order(), np.int64))
        words = [self.words[i] for i in gv.perm]
        out = DeviceWordVectors(words, self._gather(gv.perm) if gather else None, KeyIndexGrouped(words, gv.offsets),
                                self.stats)
        out.centroids, out.offsets = gv.centroids, np.asarray(gv.offsets, np.int32)
        return out, gv

    def to_host(self):
        data = self.matrix.to_host() if self.matrix is not None else np.zeros((0, 0), np.float32)
        return WordVectors(self.words, data, self.key_index)


def _take_on_host(line, dim):
    """What read_word2vec does with one line that the device could not finish: its errors are the contract."""
    parts = line.split(" ")
    vec = [parse_float(t) for t in parts[1:1 + dim]]
    if len(vec) != dim:
        raise ValueError(f"expected {dim} components after {parts[0]!r}, found {len(vec)}")
    return vec


def read_word2vec_device(source, normalize=False, chunk_bytes=0):
    """read_word2vec with the per-token work on the device (csrc/ingest.hip): the same words, the same bits, the same
    errors, the matrix left in HBM.  source: a path, or the bytes of the text (bytes / bytearray / memoryview / uint8
    array).  The host keeps what is per FILE or per LINE: the header line, the strict UTF-8 check, the words, and the
    tokens the kernel flags (parse_float converts those; gulon_ingest_finish patches them in before it normalises).
    chunk_bytes: text copied per step (0: the library's 64 MiB); results do not depend on it."""
    from .matrix import DeviceMatrix
    if isinstance(source, (str, os.PathLike)):
        text = np.fromfile(os.fspath(source), dtype=np.uint8)
    else:
        text = np.frombuffer(source, dtype=np.uint8) if not isinstance(source, np.ndarray) else N.u8(source).reshape(-1)
    mv = memoryview(text)
    check = codecs.getincrementaldecoder("utf-8")()                  # the host reader decodes the whole file strictly
    for s in range(0, len(text), 1 << 24):
        check.decode(mv[s:s + (1 << 24)], final=s + (1 << 24) >= len(text))
    if len(text) == 0:
        return DeviceWordVectors([], None, None, IngestStats(0, 0, 0))
    nl = np.flatnonzero(text[:1 << 16] == 10)
    if len(nl) == 0 and len(text) > 1 << 16:
        nl = np.flatnonzero(text == 10)
    first_end = int(nl[0]) if len(nl) else len(text)
    line = str(mv[:first_end], "utf-8")
    m = _HEADER.fullmatch(line)
    dim, offset = (int(m.group(2)), min(first_end + 1, len(text))) if m else (len(line.split(" ")) - 1, 0)
    if dim < 1:
        raise ValueError("a word2vec text without vector components has no device matrix")
    L = N.lib()
    h = C.c_void_p()
    N.check(L.gulon_ingest_word2vec(text.ctypes.data, len(text), offset, dim, int(chunk_bytes), C.byref(h)))
    try:
        rows, flagged, short = C.c_int64(), C.c_int64(), C.c_int64()
        N.check(L.gulon_ingest_counts(h, C.byref(rows), C.byref(flagged), C.byref(short)))
        n, nf = rows.value, flagged.value
        begin, length = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32)
        N.check(L.gulon_ingest_words(h, begin, length))
        f_row, f_begin = np.zeros(max(nf, 1), np.int64), np.zeros(max(nf, 1), np.int64)
        f_field, f_len = np.zeros(max(nf, 1), np.int32), np.zeros(max(nf, 1), np.int32)
        N.check(L.gulon_ingest_flagged(h, f_row, f_field, f_begin, f_len))
        # in file order, as the host reader would meet them: flagged tokens, then the first line that is too short
        order = np.lexsort((f_field[:nf], f_row[:nf]))
        if short.value >= 0:
            order = order[f_row[:nf][order] < short.value]
        values = np.zeros(max(len(order), 1), np.float32)
        for j, i in enumerate(order):
            values[j] = parse_float(str(mv[f_begin[i]:f_begin[i] + f_len[i]], "utf-8"))
        if short.value >= 0:
            b = int(begin[short.value])
            e = b + int(np.argmax(text[b:] == 10)) if (text[b:] == 10).any() else len(text)
            _take_on_host(str(mv[b:e], "utf-8"), dim)
            raise AssertionError("the device found a short line the host reader accepts")
        ends = (begin + length).tolist()
        words = [str(mv[b:e], "utf-8") for b, e in zip(begin.tolist()[:n], ends[:n])]
        ds = C.c_void_p()
        N.check(L.gulon_ingest_finish(h, np.ascontiguousarray(f_row[:nf][order]) if len(order) else np.zeros(1, np.int64),
                                      np.ascontiguousarray(f_field[:nf][order]) if len(order) else np.zeros(1, np.int32),
                                      values, len(order), int(bool(normalize)), C.byref(ds)))
        return DeviceWordVectors(words, DeviceMatrix(ds, n, dim), None, IngestStats(n * dim, nf, n))
    finally:
        L.gulon_ingest_destroy(h)


class KeyedIndex:
    """An index whose results carry words: Index.query returns (word, distance) pairs
    (Index.scala:40-62 with keyIndex); `query_word` looks the vector up first (Index.lookup)."""

    def __init__(self, index, word_vectors):
        self.index, self.vectors = index, word_vectors

    def query(self, k, vector):
        r = self.index.query(k, vector)
        return [(self.vectors.word(int(i)), float(d)) for i, d in zip(r.rows, r.distances)]

    def query_word(self, k, word):
        """Queries with the word's RAW vector from the WordVectors.  The reference's Index.queryByWord
        (Index.scala:38-45) queries with the index's DECODED vector: that is gulon_amd.word_index.WordIndex.query_by_word."""
        i = self.vectors.key_index.lookup(word) if self.vectors.key_index is not None else None
        return None if i is None else self.query(k, self.vectors[i])
