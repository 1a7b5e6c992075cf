"""The launch arithmetic of the exact scan (scan.hip, scan.hpp, index_handle.hip) restated in plain Python, without the
library: which form an index takes, how a launch is cut into chunks of row blocks, how often a wave trades its
thresholds with the other workgroups, and where a row has to sit to be walked before or after such a trade.  The GPU
tests of the shared thresholds (test_gpu_scan_thresholds.py) assert on these numbers that a case reaches the exchange;
test_scan_ref_host.py checks them against values worked out by hand."""
from collections import namedtuple

import numpy as np

LDS_BUDGET = 144 * 1024          # index_handle.hip
EXCHANGE_EVERY = 32              # scan_body: a wave 0 trades when (its iteration & 31) == 31

Layout = namedtuple("Layout", "vec ng m_pad w nsub qt")
Shape = namedtuple("Shape", "ntiles nchunks rb_per_chunk iterations_per_wave exchanges_per_wave rb_begin rb_total waves")


def _ceil_div(a, b):
    return -(-a // b)


def layout(m):
    """gulon_index_create for k <= 256: 16-byte code words when m is a multiple of 16, else 4-byte ones; as many queries
    per table entry (w) and sub-tables per workgroup (nsub) as 144 KiB of LDS hold.  qt = queries of one tile."""
    vec = 16 if m % 16 == 0 else 4
    ng = _ceil_div(m, vec)
    m_pad = ng * vec
    w = 4
    while w > 1 and m_pad * 256 * w * 4 > LDS_BUDGET:
        w //= 2
    per_sub = m_pad * 256 * w * 4
    assert per_sub <= LDS_BUDGET, m
    nsub = 1 if w < 4 else 4 if 4 * per_sub <= LDS_BUDGET else 2 if 2 * per_sub <= LDS_BUDGET else 1
    return Layout(vec, ng, m_pad, w, nsub, w * nsub)


def scan_shape(n_from, n_until, B, w, nsub, target_blocks, threads=1024):
    """ScanShape + scan_chunks: the tiles of B queries, the chunks of the row blocks of [n_from, n_until), and for the
    wave with the most row blocks (wave 0 of a full chunk) its iterations and how many of them end in an exchange."""
    waves = threads // 64
    qt = w * nsub
    ntiles = _ceil_div(B, qt)
    rb_begin = n_from // 64
    rb_total = _ceil_div(n_until, 64) - rb_begin
    want = _ceil_div(target_blocks, ntiles)
    nchunks = max(1, min(want, rb_total // (2 * waves)))
    per = _ceil_div(rb_total, nchunks)
    nchunks = _ceil_div(rb_total, per)
    iterations = _ceil_div(per, waves)
    exchanges = sum(1 for i in range(iterations) if i & (EXCHANGE_EVERY - 1) == EXCHANGE_EVERY - 1)
    return Shape(ntiles, nchunks, per, iterations, exchanges, rb_begin, rb_total, waves)


def chunk_blocks(shape, c):
    """The row blocks [first, end) of chunk c, as block numbers of the index."""
    first = shape.rb_begin + c * shape.rb_per_chunk
    return first, min(shape.rb_begin + shape.rb_total, first + shape.rb_per_chunk)


def exchanges_of_chunk(shape, c):
    """Exchanges wave 0 of chunk c makes (the last chunk may be shorter than the others)."""
    first, end = chunk_blocks(shape, c)
    return _ceil_div(end - first, shape.waves) // EXCHANGE_EVERY


def blocks_after_exchange(shape, c, nth=1):
    """The last row blocks of chunk c: those every wave walks after wave 0's nth exchange (1 = the first).  Iteration i
    of wave v is block first + v + waves * i, and the nth exchange ends iteration 32 * nth - 1."""
    first, end = chunk_blocks(shape, c)
    start = first + shape.waves * EXCHANGE_EVERY * nth
    assert start < end, ("chunk", c, "has no row block after exchange", nth)
    return list(range(start, end))


def wave_slot_blocks(shape, c, slot, count):
    """`count` row blocks of chunk c that ONE wave walks in its first iterations, before any exchange: slot s belongs to
    wave s % waves, the slots of one wave follow each other."""
    first, end = chunk_blocks(shape, c)
    v, nth = slot % shape.waves, slot // shape.waves
    out = [first + v + shape.waves * (nth * count + i) for i in range(count)]
    assert out[-1] < min(end, first + shape.waves * EXCHANGE_EVERY), ("slot", slot, "leaves the first 32 iterations")
    return out


def rows_of_blocks(blocks, n_from, n_until):
    """The rows of [n_from, n_until) in the given 64-row blocks, ascending."""
    rows = (np.asarray(blocks, np.int64)[:, None] * 64 + np.arange(64)[None, :]).reshape(-1)
    return rows[(rows >= n_from) & (rows < n_until)]


def last_rows_of_chunk(shape, c, count, n_from, n_until, nth=1):
    """The last `count` rows of chunk c, all of them behind wave 0's nth exchange."""
    rows = rows_of_blocks(blocks_after_exchange(shape, c, nth), n_from, n_until)
    assert len(rows) >= count, (len(rows), count)
    return rows[len(rows) - count:]


def pairwise_cover(blocks, prunes, froms):
    """A pairwise cover of blocks x prunes x froms for two prune values: every (blocks, from) pair, and with it every
    (blocks, prune) and (prune, from) pair as long as there are two or more values on the other axis."""
    assert len(prunes) == 2 and len(blocks) >= 2 and len(froms) >= 2
    return [(b, prunes[(bi + fi) % 2], f) for bi, b in enumerate(blocks) for fi, f in enumerate(froms)]


# The shapes of test_gpu_scan_thresholds.py: name -> (d, m, k, rows, GULON_SCAN_BLOCKS per query tile).  The smallest
# that reach the exchange: a chunk needs 512 row blocks (32 768 rows) for wave 0 to trade once.
THRESHOLD_CASES = {
    "one_word": (128, 16, 256, 200000, 3),      # one 16-byte word: three chunks of 1042 row blocks, two exchanges
    "two_words": (64, 32, 256, 70000, 2),       # ng = 2
    "words_of_4": (100, 25, 256, 70000, 2),     # 4-byte words
    "w2": (128, 64, 256, 70000, 2),             # two queries per table entry
    "w1": (200, 100, 256, 70000, 2),            # one query per table entry
    "codes_of_4_bits": (12, 4, 5, 70000, 2),    # 4-bit codes
}
RESIDENCY_CASE = (128, 16, 256, 150000, 130)    # d, m, k, rows, B at the default GULON_SCAN_BLOCKS
