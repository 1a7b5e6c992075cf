"""scan_ref.py (the exact scan's launch arithmetic restated) against values worked out by hand from scan.hpp's
scan_chunks, scan.hip's ScanShape and gulon_index_create's choice of the kernel form.  No GPU."""
import numpy as np
import pytest

import scan_ref as R


@pytest.mark.parametrize("m,expect", [
    (16, (16, 1, 16, 4, 2, 8)),        # 64 KiB per sub-table: two fit into 144 KiB -> 8 queries per tile
    (32, (16, 2, 32, 4, 1, 4)),        # 128 KiB: one
    (25, (4, 7, 28, 4, 1, 4)),         # 4-byte words, m_pad = 28: 112 KiB
    (64, (16, 4, 64, 2, 1, 2)),        # 256 KiB at w = 4 -> w = 2
    (100, (4, 25, 100, 1, 1, 1)),      # w = 1: 100 KiB
    (4, (4, 1, 4, 4, 4, 16)),          # 16 KiB per sub-table: four
    (8, (4, 2, 8, 4, 4, 16)),          # 32 KiB: four
    (36, (4, 9, 36, 4, 1, 4)),         # 144 KiB exactly
])
def test_layout(m, expect):
    assert tuple(R.layout(m)) == expect


def test_largest_exact_scan_of_the_older_suite_never_trades():
    """200 000 rows, B = 64 at the default 4096 workgroups: 3125 row blocks, 8 tiles, 512 chunks wanted but only
    3125 // 32 = 97 allowed; ceil(3125 / 97) = 33 blocks per chunk and so ceil(3125 / 33) = 95 chunks.  A wave walks
    at most ceil(33 / 16) = 3 row blocks: no exchange."""
    s = R.scan_shape(0, 200000, 64, 4, 2, 4096)
    assert (s.ntiles, s.rb_total, s.nchunks, s.rb_per_chunk) == (8, 3125, 95, 33)
    assert (s.iterations_per_wave, s.exchanges_per_wave) == (3, 0)
    assert R.chunk_blocks(s, 94) == (3102, 3125)


def test_benchmark_shape_trades_nine_times():
    """10 M rows, B = 1024: 156 250 row blocks, 128 tiles, ceil(4096 / 128) = 32 chunks of ceil(156250 / 32) = 4883
    blocks; wave 0 walks ceil(4883 / 16) = 306 of them and trades after iterations 31, 63, ..., 287."""
    s = R.scan_shape(0, 10_000_000, 1024, 4, 2, 4096)
    assert (s.ntiles, s.rb_total, s.nchunks, s.rb_per_chunk) == (128, 156250, 32, 4883)
    assert (s.iterations_per_wave, s.exchanges_per_wave) == (306, 9)


def test_one_word_case_three_chunks_two_exchanges():
    """200 000 rows at GULON_SCAN_BLOCKS = 3 * ntiles: three chunks of ceil(3125 / 3) = 1042 row blocks (the last one
    1041), 66 iterations, exchanges after iterations 31 and 63 -- for any B."""
    d, m, k, n, per_tile = R.THRESHOLD_CASES["one_word"]
    lay = R.layout(m)
    for B, ntiles in ((1, 1), (9, 2), (19, 3), (64, 8)):
        s = R.scan_shape(0, n, B, lay.w, lay.nsub, per_tile * ntiles)
        assert (s.ntiles, s.nchunks, s.rb_per_chunk, s.iterations_per_wave, s.exchanges_per_wave) == (ntiles, 3, 1042, 66, 2)
    assert [R.chunk_blocks(s, c) for c in range(3)] == [(0, 1042), (1042, 2084), (2084, 3125)]
    assert [R.exchanges_of_chunk(s, c) for c in range(3)] == [2, 2, 2]
    assert R.blocks_after_exchange(s, 0, 2) == list(range(1024, 1042))
    assert R.blocks_after_exchange(s, 2, 1) == list(range(2084 + 512, 3125))
    # a range that cuts the first and the last 64-row block keeps the blocks
    assert R.scan_shape(37, n - 29, 9, lay.w, lay.nsub, 6)[:5] == (2, 3, 1042, 66, 2)
    # the two halves scanned as partial lists: 1563 and 1562 blocks in two chunks, one exchange each
    assert R.scan_shape(0, 100032, 9, lay.w, lay.nsub, 4)[:5] == (2, 2, 782, 49, 1)
    assert R.scan_shape(100032, n, 9, lay.w, lay.nsub, 4)[:5] == (2, 2, 781, 49, 1)


@pytest.mark.parametrize("name,qt", [("two_words", 4), ("words_of_4", 4), ("w2", 2), ("w1", 1), ("codes_of_4_bits", 16)])
def test_other_layouts_two_chunks_one_exchange(name, qt):
    """70 000 rows are 1094 row blocks: at two workgroups per tile two chunks of 547, 35 iterations, one exchange (after
    iteration 31); the 35 blocks 512 .. 546 of a chunk come after it."""
    d, m, k, n, per_tile = R.THRESHOLD_CASES[name]
    lay = R.layout(m)
    assert lay.qt == qt
    for B in (qt + 1, 2 * qt + 3):
        ntiles = -(-B // qt)
        s = R.scan_shape(0, n, B, lay.w, lay.nsub, per_tile * ntiles)
        assert (s.ntiles, s.nchunks, s.rb_per_chunk, s.iterations_per_wave, s.exchanges_per_wave) == (ntiles, 2, 547, 35, 1)
        assert R.scan_shape(37, n - 29, B, lay.w, lay.nsub, per_tile * ntiles)[:5] == s[:5]
    assert R.blocks_after_exchange(s, 0) == list(range(512, 547))
    assert R.blocks_after_exchange(s, 1) == list(range(547 + 512, 1094))
    rows = R.last_rows_of_chunk(s, 1, 100, 0, n)
    assert rows[0] == 69900 and rows[-1] == 69999           # the last block holds 48 rows
    # partial lists over [0, 66048) and the rest: 1032 blocks in two chunks of 516 reach the exchange, 62 blocks do not
    assert R.scan_shape(0, 66048, qt + 1, lay.w, lay.nsub, 4)[:5] == (2, 2, 516, 33, 1)
    assert R.scan_shape(66048, n, qt + 1, lay.w, lay.nsub, 4)[:5] == (2, 1, 62, 4, 0)


def test_other_knob_values_of_the_grid():
    """GULON_SCAN_BLOCKS = 1 and = ntiles give one chunk; 4096 as many as two row blocks per wave allow."""
    lay = R.layout(16)
    assert R.scan_shape(0, 200000, 9, lay.w, lay.nsub, 1)[:5] == (2, 1, 3125, 196, 6)
    assert R.scan_shape(0, 200000, 9, lay.w, lay.nsub, 2)[:5] == (2, 1, 3125, 196, 6)
    assert R.scan_shape(0, 200000, 9, lay.w, lay.nsub, 4096)[:5] == (2, 95, 33, 3, 0)
    assert R.scan_shape(0, 70000, 5, 4, 1, 4096)[:5] == (2, 34, 33, 3, 0)      # 1094 // 32 = 34; ceil(1094 / 34) = 33


def test_residency_case():
    """150 000 rows, B = 130 on the one-word layout: 17 tiles of 8 queries; ceil(4096 / 17) = 241 chunks wanted,
    2344 // 32 = 73 allowed, ceil(2344 / 73) = 33 blocks each and so 72 chunks: 1224 workgroups of 128 KiB of LDS."""
    d, m, k, n, B = R.RESIDENCY_CASE
    lay = R.layout(m)
    s = R.scan_shape(0, n, B, lay.w, lay.nsub, 4096)
    assert (s.ntiles, s.rb_total, s.nchunks, s.rb_per_chunk, s.exchanges_per_wave) == (17, 2344, 72, 33, 0)
    assert s.ntiles * s.nchunks == 1224 > 256          # more than one workgroup per compute unit of an MI355X


def test_slots_and_rows():
    s = R.scan_shape(0, 70000, 5, 4, 1, 4)
    assert R.wave_slot_blocks(s, 0, 0, 2) == [0, 16]                   # wave 0's first two row blocks
    assert R.wave_slot_blocks(s, 1, 3, 2) == [547 + 3, 547 + 19]
    assert R.wave_slot_blocks(s, 0, 17, 2) == [1 + 32, 1 + 48]         # wave 1 again: its third and fourth
    with pytest.raises(AssertionError):
        R.wave_slot_blocks(s, 0, 16 * 16, 2)                           # iteration 32 is behind the exchange
    with pytest.raises(AssertionError):
        R.blocks_after_exchange(s, 0, 2)                               # there is no second exchange
    assert R.rows_of_blocks([1, 3], 70, 200).tolist() == list(range(70, 128)) + list(range(192, 200))
    assert np.array_equal(R.rows_of_blocks([1093], 0, 70000), np.arange(69952, 70000))


def test_pairwise_cover_covers_every_pair():
    blocks, prunes, froms = [1, 2, 6, 4096], [0, 1], [-1, 0, 4, 8, 12, 16, 116]
    cover = R.pairwise_cover(blocks, prunes, froms)
    assert len(cover) == 28
    assert {(b, f) for b, p, f in cover} == {(b, f) for b in blocks for f in froms}
    assert {(b, p) for b, p, f in cover} == {(b, p) for b in blocks for p in prunes}
    assert {(p, f) for b, p, f in cover} == {(p, f) for p in prunes for f in froms}
