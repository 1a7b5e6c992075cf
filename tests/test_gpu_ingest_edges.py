"""The device ingest (csrc/ingest.hip, csrc/ingest_parse.h, word_vectors.read_word2vec_device) at its edges.

Part one holds the DEVICE build of the one-token conversion -- the copy hipcc compiles into ingest_convert, with
__fdiv_rn, 64-bit carries on 32-bit limbs, __builtin_clz and the restoring division -- to what
tests/test_ingest_parse.py holds the host build to: the exact rounding on rationals of tests/ingest_tokens.py, the same
token families, the same caps on the flagged share; and to the host build itself, bits and flags.

Part two reaches the kernel paths around the conversion that small files do not reach (more than 1024 tiles in a chunk,
a flag list that overflows, a matrix that grows with rows to keep, line starts at tile borders, the field scan's
64-byte steps, normalize at other widths), each with the smallest text that gets there, against the host reader
(word_vectors.read_word2vec): the same words, shape, bits, stats and errors."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import bits
from ingest_tokens import (check, check_edges, convert, crafted_midpoints_of_forty_digits, edges,  # noqa: F401
                           fixed_six_decimals, long_significands, midpoints_of_eight_and_nine_digits,
                           outside_the_grammar, shortest_round_trip)
from test_gpu_ingest import W, _same  # noqa: F401

pytestmark = pytest.mark.gpu

TILE = 4096                     # ingest.hip: LS_TILE, bytes of text per workgroup of the line scan
FLAG_CAP = 1 << 16              # ingest.hip: flagged tokens kept per chunk before the list is regrown


# ---- the device converter, with the host converter's contract -------------------------------------------------------

def in_a_line(tokens):
    """Those of `tokens` that can stand between two blanks of a line."""
    return [t for t in tokens if t and " " not in t and "\n" not in t]


def device_convert(tokens, d=7, chunk_bytes=0):
    """ingest_convert as a converter: per token the binary32's bits, or None where the kernel flagged it.

    The tokens go row-major into lines `w<i> tok ... tok` (the last row padded with `0`) and through the entry points
    read_word2vec_device uses; nothing is patched and nothing normalised.  The flagged LIST decides what is None (the
    kernel stores 0 there, and 0 is also an answer); every entry of it must cut exactly its token's bytes out of the
    text, and no (row, field) may be listed twice."""
    from gulon_amd import native as N
    from gulon_amd.matrix import DeviceMatrix
    tokens = list(tokens)
    assert tokens and in_a_line(tokens) == tokens
    rows = -(-len(tokens) // d)
    padded = tokens + ["0"] * (rows * d - len(tokens))
    data, begin, length = bytearray(), [], []
    for r in range(rows):
        data += b"w%d" % r
        for t in padded[r * d:(r + 1) * d]:
            raw = t.encode("utf-8")
            data += b" "
            begin.append(len(data))
            length.append(len(raw))
            data += raw
        data += b"\n"
    text = np.frombuffer(bytes(data), dtype=np.uint8)
    L = N.lib()
    h = C.c_void_p()
    N.check(L.gulon_ingest_word2vec(text.ctypes.data, len(text), 0, d, int(chunk_bytes), C.byref(h)))
    try:
        n, flagged, short = C.c_int64(), C.c_int64(), C.c_int64()
        N.check(L.gulon_ingest_counts(h, C.byref(n), C.byref(flagged), C.byref(short)))
        assert (n.value, short.value) == (rows, -1)
        nf = flagged.value
        f_row, f_begin = np.zeros(max(nf, 1), np.int64), np.zeros(max(nf, 1), np.int64)
        f_field, f_len = np.zeros(max(nf, 1), np.int32), np.zeros(max(nf, 1), np.int32)
        N.check(L.gulon_ingest_flagged(h, f_row, f_field, f_begin, f_len))
        ds = C.c_void_p()
        N.check(L.gulon_ingest_finish(h, np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(1, np.float32), 0, 0,
                                      C.byref(ds)))
        x = DeviceMatrix(ds, rows, d).to_host()
    finally:
        L.gulon_ingest_destroy(h)
    f_row, f_field, f_begin, f_len = f_row[:nf], f_field[:nf], f_begin[:nf], f_len[:nf]
    assert ((f_row >= 0) & (f_row < rows) & (f_field >= 0) & (f_field < d)).all()
    at = f_row * d + f_field
    assert len(np.unique(at)) == nf, "a (row, field) is listed twice"
    assert np.array_equal(f_begin, np.asarray(begin, np.int64)[at]), "a flagged entry does not begin at its token"
    assert np.array_equal(f_len, np.asarray(length, np.int32)[at]), "a flagged entry is not as long as its token"
    out = bits(x).reshape(-1).tolist()
    for i in at.tolist():
        out[i] = None
    assert out[len(tokens):] == [0] * (len(padded) - len(tokens))
    return out[:len(tokens)]


# family -> (tokens, cap on the flagged share).  The caps are those of tests/test_ingest_parse.py: conditions, not
# measurements (the host build flags none of these tokens at four times the count).  A quarter of the host test's
# counts: the time goes into the Fractions of exact_bits.
@functools.lru_cache(maxsize=None)
def _families():
    _, sci, pos = shortest_round_trip(12, 30000)
    return {
        "%.6f": (fixed_six_decimals(11, 30000), 0),
        "shortest scientific": (sci, 1e-4),
        "shortest positional": (pos, 1e-4),
        "8/9-digit midpoints": (midpoints_of_eight_and_nine_digits(13, 30000), 1e-4),
        "crafted 40-digit midpoints": (crafted_midpoints_of_forty_digits(5, 3000), None),   # > 19 digits may be flagged
        "long significands": (long_significands(14, 16000), 1e-4),
        "edges": (edges()[0], None),
        "outside the grammar": (in_a_line(outside_the_grammar()), None),
    }


@functools.lru_cache(maxsize=None)
def _on_the_device(name):
    return device_convert(_families()[name][0])


NUMERIC = ["%.6f", "shortest scientific", "shortest positional", "8/9-digit midpoints", "crafted 40-digit midpoints",
           "long significands"]


@pytest.mark.parametrize("name", NUMERIC)
def test_device_conversion_is_the_exact_rounding(W, name):
    """Every token the device decides is the exact rounding; it flags no %.6f token and at most 1 in 10 000 of the
    shortest decimals, the 8/9-digit midpoints and the long significands."""
    tokens, cap = _families()[name]
    check(lambda toks: _on_the_device(name), name, tokens, cap)
    if name == "%.6f":
        assert None not in _on_the_device(name)


def test_shortest_decimals_come_back_as_their_patterns(W):
    pats, sci, pos = shortest_round_trip(12, 30000)
    for name, toks in (("shortest scientific", sci), ("shortest positional", pos)):
        assert toks == _families()[name][0]
        back = [(t, g, int(p)) for t, g, p in zip(toks, _on_the_device(name), pats) if g is not None and g != int(p)]
        assert not back, back[:5]


@pytest.mark.parametrize("d, chunk_bytes", [(1, 0), (16, 0), (16, 5000)])
def test_fixed_six_decimals_at_other_widths(W, d, chunk_bytes):
    """One token per row, and sixteen; in chunks too, where a flagged token's `begin` is an offset into the file and
    not into the chunk."""
    tokens = _families()["%.6f"][0]
    assert check(lambda toks: device_convert(toks, d, chunk_bytes), f"%.6f, d = {d}", tokens, 0) == 0
    mixed = tokens[:2000] + _families()["crafted 40-digit midpoints"][0][:2000]
    assert device_convert(mixed, d, chunk_bytes) == _on_the_device("%.6f")[:2000] + \
        _on_the_device("crafted 40-digit midpoints")[:2000]


@pytest.mark.parametrize("name", NUMERIC + ["edges", "outside the grammar"])
def test_device_and_host_builds_of_the_header_agree(W, convert, name):
    """One header gives one answer, bits and flags, under hipcc for gfx950 and under gcc."""
    tokens = _families()[name][0]
    got, want = _on_the_device(name), convert(tokens)
    differ = [(t, g, w) for t, g, w in zip(tokens, got, want) if g != w]
    assert not differ, (len(differ), differ[:5])
    if name == "outside the grammar":
        assert got == [None] * len(tokens)


def test_edges_on_the_device(W):
    """The must-decide tokens are decided, the four tokens of the undecided sliver under 2^128 are flagged."""
    check_edges(device_convert)


def test_a_file_of_every_family_end_to_end(W, tmp_path):
    """The user-visible contract: with the flagged tokens converted by the host and patched in, the matrix of
    read_word2vec_device is read_word2vec's bit for bit.  (Python's float() accepts some of the tokens outside the
    kernel's grammar -- NaN, Infinity, 1_000, non-ASCII digits, a tab in front: those stay in.)"""
    def host_accepts(t):
        try:
            float(t)
            return True
        except ValueError:
            return False
    rnd = np.random.default_rng(31)
    tokens = []
    for name in NUMERIC:
        toks = _families()[name][0]
        tokens += [toks[i] for i in rnd.choice(len(toks), 300, replace=False)]
    tokens += edges()[0] + [t for t in in_a_line(outside_the_grammar()) if host_accepts(t)]
    tokens = [tokens[i] for i in rnd.permutation(len(tokens))]
    tokens += ["0"] * (-len(tokens) % 7)
    text = "".join(f"w{r} " + " ".join(tokens[r * 7:r * 7 + 7]) + "\n" for r in range(len(tokens) // 7))
    got, _ = _same(W, tmp_path, text)
    assert got.stats.flagged >= 4
    _same(W, tmp_path, text, chunk_bytes=TILE)


# ---- the kernels around the converter -------------------------------------------------------------------------------

@pytest.mark.parametrize("long_line", [False, True])
def test_more_than_1024_tiles_in_one_chunk(W, tmp_path, long_line):
    """ingest_line_offsets gives each of its 1024 lanes (nb + 1023) / 1024 tiles: above 1024 tiles (4 MiB of text in
    one chunk; the default chunk is 64 MiB) a lane sums more than one.  A little over 4 MiB + one tile of lines of 27
    to 726 bytes (long words, two components: the host reader's time goes by the token), some eleven line starts to a
    tile; then the same with a line of 13 000 bytes in the middle, which leaves two or three tiles in a row, inside
    the lanes' segments, without any line start."""
    rng = np.random.default_rng(41)
    lines, size, i = [], 0, 0
    while size <= (4 << 20) + 2 * TILE:
        lines.append(f"w{i:06d}{'x' * (i % 700)} " + " ".join("%.6f" % v for v in rng.uniform(-10, 10, 2)) + "\n")
        size += len(lines[-1])
        i += 1
    if long_line:
        lines[len(lines) // 2] = "long 1 2 " + "y" * 13000 + "\n"
    text = "".join(lines)
    assert -(-len(text) // TILE) > 1024 + 1
    got, _ = _same(W, tmp_path, text)
    assert got.size == len(lines) and got.stats.flagged == 0


def _crlf(n):
    return "".join(f"w {i % 10} {i % 7}\r\n" for i in range(n))


@pytest.mark.parametrize("n", [FLAG_CAP, FLAG_CAP + 1])
def test_flag_list_full_and_overflowing(W, tmp_path, n):
    """A CRLF file flags the last token of every line (the \\r belongs to it).  65 536 lines in one chunk fill the flag
    list exactly (ingest_run: nflag <= capacity, no second pass); 65 537 overflow it: the list is regrown to the count
    and the chunk converted once more.  The number of passes cannot be seen from outside; what either gets wrong can:
    the count, and through the host's patch every flagged position.  A third text read after the overflowing one
    finds nothing of it (the list belongs to the call)."""
    got, _ = _same(W, tmp_path, _crlf(n))
    assert got.size == n and got.stats.flagged == n
    got, _ = _same(W, tmp_path, "a 1 2\r\nb 3 4\r\nc NaN 6\r\n")
    assert got.stats.flagged == 4


def test_the_matrix_grows_with_rows_to_keep(W, tmp_path):
    """grow() with rows to keep: the device-to-device copy of what is already converted.  ingest_run sizes the matrix
    at a chunk that is not the last one as total * len / end * 1.02 + 1024 rows (total: rows so far, end: bytes so
    far), so the text must get denser twice.  chunk_bytes = 65 536, no header, d = 2:
      ten lines of 6 549 bytes (an extra field of junk), 65 490 bytes; then 20 000 lines of 20 bytes; len = 465 490.
      chunk 1 ends at 65 530 with 12 rows:            capacity 12 * 465490 / 65530 * 1.02 + 1024 = 1 110 rows;
      chunk 2 ends at 131 050, total 3 288 > 1 110:   grow keeps 12 rows, capacity 3288 * 465490 / 131050 * 1.02 + 1024
                                                      = 12 936 rows;
      chunks 3, 4: totals 6 564 and 9 840 fit;
      chunk 5 ends at 327 610, total 13 116 > 12 936: grow keeps 9 840 rows, capacity 20 032 >= the file's 20 010."""
    junk = "".join(f"j{k} {k} -{k} " + "x" * 6540 + "\n" for k in range(10))
    short = [f"w{i:05d} {i:05d} -{i:05d}\n" for i in range(20000)]
    text = short[0] + junk + "".join(short[1:])                      # the first line sets d = 2
    assert len(junk) == 65490 and len(text) == 465490
    got, _ = _same(W, tmp_path, text, chunk_bytes=65536)
    assert got.size == 20010


def _line(n, k):
    """A line of two components and exactly n bytes, its \\n included."""
    assert n >= 6
    return ("f" * (n - 5) + f" {k % 10} {k % 7}\n").encode()


def _fill(buf, target):
    """Whole lines appended to buf up to byte `target` exactly."""
    assert target - len(buf) >= 80
    while target - len(buf) >= 80:
        buf += _line(23 + len(buf) % 17, len(buf))
    if target > len(buf):
        buf += _line(target - len(buf), len(buf))
    assert len(buf) == target and buf[-1] == 10


def test_line_starts_at_every_offset_of_a_tile(W, tmp_path):
    """4 100 lines of 11 bytes and no header: 11 is odd, so the line starts run through every residue mod 4096 -- the
    first byte of a tile, where line_start_mask reads the previous workgroup's last byte, every byte of a 16-byte
    group, and the last byte of a tile."""
    text = "".join(f"w{i:04d} {i % 10} -{i % 7}\n" for i in range(4100))
    assert len(text) == 4100 * 11 and {i * 11 % TILE for i in range(4100)} == set(range(TILE))
    got, _ = _same(W, tmp_path, text)
    assert got.size == 4100


def test_line_starts_around_tile_borders(W, tmp_path):
    """At eight tile borders b in turn, twice each: a line starts exactly at b; b is the second \\n of an empty line
    (the line before ends at b - 1); b is the first \\n of an empty line (the line before ends AT b); the blank in
    front of the last token is the last byte of a tile."""
    buf, borders = bytearray(), []
    for k in range(1, 9):
        b, kind = k * TILE, (k - 1) % 4
        if kind == 0:
            _fill(buf, b)
        elif kind == 1:
            _fill(buf, b)
            buf += b"\n"
        elif kind == 2:
            _fill(buf, b + 1)
            buf += b"\n"
        else:
            _fill(buf, b - 4)
            buf += b"x 3 4\n"
        borders.append((b, kind))
    _fill(buf, len(buf) + 200)
    nl, sp = 10, 32
    for b, kind in borders:
        if kind == 0:
            assert buf[b - 1] == nl and buf[b] != nl
        elif kind == 1:
            assert buf[b - 2] != nl and buf[b - 1] == nl and buf[b] == nl and buf[b + 1] != nl
        elif kind == 2:
            assert buf[b - 1] != nl and buf[b] == nl and buf[b + 1] == nl and buf[b + 2] != nl
        else:
            assert buf[b - 1] == sp and bytes(buf[b:b + 2]) == b"4\n"
    got, _ = _same(W, tmp_path, bytes(buf))
    assert got.size == bytes(buf).count(b"\n") - 4              # the empty lines take no row
    _same(W, tmp_path, bytes(buf), chunk_bytes=3 * TILE)


@pytest.mark.parametrize("size, final_newline", [(2 * TILE, False), (2 * TILE + 1, False), (2 * TILE + 1, True)])
def test_a_text_that_ends_at_a_tile_border(W, tmp_path, size, final_newline):
    """Two whole tiles and no final newline: the last line ends at the padding.  One byte more, as the last token's
    last digit and as the final newline: a third tile of one byte."""
    buf = bytearray()
    tail = 30 if final_newline else 29
    _fill(buf, size - tail)
    buf += _line(30, 7)[:tail]
    assert len(buf) == size and (buf[-1] == 10) == final_newline
    got, _ = _same(W, tmp_path, bytes(buf))
    assert got.words[-1] == "f" * 25


def _token(rng, n):
    """A decimal token of n bytes, 1 <= n <= 9."""
    digits = "".join(str(x) for x in rng.integers(0, 10, n))
    if n == 1:
        return digits
    if n == 2:
        return "-" + digits[1]
    if n >= 4 and rng.integers(0, 2):
        return "-" + digits[1] + "." + digits[3:]
    return digits[0] + "." + digits[2:]


def _field_scan_text(d, lines=280):
    """Lines for ingest_field_scan (one wavefront per line, 64 bytes a step): the word of line i is i % 70 bytes long,
    the empty word included, and the tokens are of 1 to 9 bytes, so the blanks sweep every lane of a step; every third
    line carries 1 to 4 extra fields (the scan stops at the (d+1)-th blank, in the d-th blank's step or in a later
    one); one word is 5 000 bytes long.  The asserts say that the text has what it is built for."""
    rng = np.random.default_rng(1000 + d)
    out = []
    blank_lanes, newline_lanes, steps_apart = set(), set(), set()
    for i in range(lines):
        word = "w" * (5000 if i == 100 else i % 70)
        line = word + "".join(" " + _token(rng, int(rng.integers(1, 10))) for _ in range(d))
        at = [j for j, c in enumerate(line) if c == " "]             # the line's first d blanks
        blank_lanes |= {j % 64 for j in at}
        if i % 3 == 1:
            steps_apart.add(len(line) // 64 - at[-1] // 64)          # the (d+1)-th blank comes at len(line)
            blank_lanes.add(len(line) % 64)
            line += "".join(" " + "x" * n for n in (1, 30, 1, 100)[:1 + i % 4])
        else:
            newline_lanes.add(len(line) % 64)
        out.append(line + "\n")
    assert blank_lanes == set(range(64)) and 0 in newline_lanes and 63 in newline_lanes
    assert steps_apart == {0, 1}
    return "".join(out)


@pytest.mark.parametrize("d", [1, 64, 65, 130])
def test_field_scan_at_its_64_byte_steps(W, tmp_path, d):
    """d = 64, 65: the d + 1 = 65, 66 positions of a short line no longer fit one stride of the fill loop; d = 130:
    three strides."""
    text = _field_scan_text(d)
    got, _ = _same(W, tmp_path, text)
    assert got.dimension == d and got.size == 280
    _same(W, tmp_path, text, chunk_bytes=TILE)


def _row(word, components):
    return word + "".join(" " + c for c in components) + "\n"


GOOD = _row("g", ["1.5"] * 130)
BAD = _row("bad", ["1"] * 64 + ["oops"] + ["1"] * 65)
SHORT_LINES = {f"{c} components": GOOD * 3 + _row("short", ["2"] * c) + GOOD for c in (0, 63, 64, 65, 129)}
SHORT_LINES["after a bad token"] = GOOD + BAD + GOOD + _row("short", ["2"] * 5) + GOOD
SHORT_LINES["before a bad token"] = GOOD + _row("short", ["2"] * 5) + GOOD + BAD + GOOD


@pytest.mark.parametrize("name", list(SHORT_LINES))
def test_short_lines_of_wide_rows_raise_what_the_host_raises(W, name):
    """d = 130: a line with too few components leaves more positions to fill than a wavefront has lanes.  The error is
    the host reader's, text and type; with a bad token in an earlier line (an earlier chunk, at one line per chunk) it
    is the token's error, with one in a later line it is the short line's."""
    text = SHORT_LINES[name]
    with pytest.raises(ValueError) as want:
        W.read_word2vec_text(text)
    assert ("oops" in str(want.value)) == (name == "after a bad token")
    for chunk in (0, 1):
        with pytest.raises(ValueError) as got:
            W.read_word2vec_device(text.encode("utf-8"), chunk_bytes=chunk)
        assert str(got.value) == str(want.value) and type(got.value) is type(want.value)


@pytest.mark.parametrize("d", [1, 63, 64, 65, 300])
def test_normalize_at_other_widths(W, tmp_path, d):
    """normalize_rows_kernel: one wavefront per row, lanes striding over d.  Each file has a zero row (NaN, as on the
    JVM), two rows with a flagged token (patched in BEFORE the row is normalised), a row whose sum of squares is
    subnormal (components k e-22, squares of 1e-44 to 5e-43, at most 300 of them: below 2^-126; the norm itself, a
    square root, is not) and a row of subnormal components, whose squares all vanish."""
    rng = np.random.default_rng(50 + d)
    text = "".join(f"r{i} " + " ".join("%.6f" % v for v in rng.uniform(-10, 10, d)) + "\n" for i in range(12))
    text += _row("zero", ["0"] * d)
    text += _row("odd", ["NaN"] + ["1.5"] * (d - 1))
    text += _row("mid", ["123456789012345678901234567890e-29"] + ["0.25"] * (d - 1))
    text += _row("tiny", [f"{1 + j % 7}e-22" for j in range(d)])
    text += _row("sub", [f"{1 + j % 5}e-40" for j in range(d)])
    text += "".join(f"s{i} " + " ".join("%.6f" % v for v in rng.uniform(-1, 1, d)) + "\n" for i in range(3))
    raw = W.read_word2vec_text(text)
    tiny = raw.data[raw.words.index("tiny")]
    total = np.float32(0)
    for v in tiny:
        total = np.float32(total + np.float32(v * v))
    assert 0 < total < np.float32(2.0 ** -126)
    got, want = _same(W, tmp_path, text, normalize=True)
    assert got.stats.flagged == 2
    assert np.isnan(want.data[want.words.index("zero")]).all()
    for word in ("tiny", "mid"):
        assert np.isfinite(want.data[want.words.index(word)]).all()
    _same(W, tmp_path, text, normalize=True, chunk_bytes=1)
