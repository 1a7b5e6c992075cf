"""batch_seams_ref.py against values worked by hand: the production shapes that make the seams matter, and every shape
tests/test_gpu_batch_seams.py and the 2^24-row cases of tests/test_gpu_kmeans.py use.  No GPU, no library."""
import batch_seams_ref as S


def test_wide_sub_batches_at_production_size():
    # 10 M rows, m = 16, k = 4096: a table is 16 * 4096 * 4 = 256 KiB, eight quantizers (128 KiB) per launch, two launches,
    # so the parked sums count: 2^30 / (10 000 000 * 4) = 26.8
    assert 10_000_000 % 64 == 0
    assert S.wide_passes(16, 4096) == (True, 8, 2) and S.wide_form(16, 4096) == "sliced"
    assert S.wide_sub_batch(1024, 16, 4096, 10_000_000) == 26
    assert S.wide_sub_batch(20, 16, 4096, 10_000_000) == 20
    # m = 16, k = 1024: 64 KiB, in LDS; 2^30 / 2^16 = 16 384 queries, whatever the rows
    assert S.wide_form(16, 1024) == "lds" and S.wide_sub_batch(20000, 16, 1024, 10_000_000) == 16384
    # (what tests/test_gpu_peel_ties.py states about its own shapes)
    assert S.wide_sub_batch(37, 16, 1024, S.ceil_div(20000, 64) * 64) == 37
    assert S.wide_sub_batch(37, 112, 65536, 64) == 36


def test_wide_shapes_of_the_gpu_cases():
    # table in LDS: 2 * 16384 * 4 = 128 KiB exactly; 2^30 / 2^17 = 8192
    assert S.wide_form(2, 16384) == "lds" and S.wide_sub_batch(8197, 2, 16384, 256) == 8192
    assert S.sub_batches(8197, 8192) == [(0, 8192), (8192, 5)] and S.seams(8197, 8192) == [8192]
    # gathered: one quantizer is 256 KiB; a table 512 KiB; 2^30 / 2^19 = 2048
    assert S.wide_form(2, 65536) == "gathered" and S.wide_passes(2, 65536) == (False, 2, 1)
    assert S.wide_sub_batch(2053, 2, 65536, 256) == 2048
    assert S.sub_batches(2053, 2048) == [(0, 2048), (2048, 5)]
    # its tie replay: 256 MiB / 512 KiB = 512 flagged queries per round
    assert S.wide_replay_round(2053, 2, 65536) == 512
    assert S.wide_replay_round(2053, 16, 1024) == 1024 and S.wide_replay_round(37, 16, 1024) == 37
    # sliced: one quantizer (128 KiB) per launch, two launches; tables allow 4096, the parked sums 2^30 / 2^20 = 1024
    assert S.wide_passes(2, 32768) == (True, 1, 2) and S.wide_form(2, 32768) == "sliced"
    assert S.wide_sub_batch(1029, 2, 32768, 262144) == 1024
    assert S.wide_sub_batch(1029, 2, 32768, 262144 - 64) == 1024                  # 4095 row blocks: 1024.25
    # (4096 row blocks are 8 * 512, the default GULON_FILTER_MIN_RB: the wide filter would take the K <= 63 batch)
    assert S.wide_filter_eligible(1029, 10, 2, 32768, 4096) and not S.wide_filter_eligible(1029, 10, 2, 32768, 4095)
    assert S.sub_batches(1029, 1024) == [(0, 1024), (1024, 5)]
    assert S.wide_sub_batch(1029, 2, 32768, 64) == 1029        # few rows: only the tables count (4096)


def test_wide_filter_hand_over():
    # m = 2, k = 16384: 4 queries per 8-bit entry (2 * 16384 * 8 = 256 KiB > 144 KiB; 16384 * 4 = 64 KiB fits), whole table
    assert S.wf_qw(2, 16384) == 4 and S.wf_slice(2, 16384) == 2
    # 2048 rows = 32 row blocks = 8 * GULON_FILTER_MIN_RB at 4; B * 128 KiB <= 1 GiB up to 8192
    assert S.wide_filter_eligible(8192, 10, 2, 16384, 32, min_rb=4)
    assert not S.wide_filter_eligible(8193, 10, 2, 16384, 32, min_rb=4)
    assert not S.wide_filter_eligible(8192, 10, 2, 16384, 31, min_rb=4)
    assert not S.wide_filter_eligible(8192, 10, 2, 16384, 32)               # the default: 4096 row blocks
    assert not S.wide_filter_eligible(8192, 64, 2, 16384, 32, min_rb=4)
    assert not S.wide_filter_eligible(8192, 10, 2, 16384, 32, min_rb=4, filter_on=False)
    # the filter's scans of that index: the table in LDS
    assert S.wide_range_form(8192, 2, 16384, 16) == "lds"
    # m = 2, k = 65536: one quantizer's 8-bit entries for four queries are 256 KiB: refused
    assert S.wf_qw(2, 65536) == 0 and not S.wide_filter_eligible(1, 10, 2, 65536, 1 << 14)
    # production, m = 16, k = 4096: 8-bit tables sliced by 8 quantizers (144 KiB / 16 KiB = 9, at most 8)
    assert S.wf_qw(16, 4096) == 4 and S.wf_slice(16, 4096) == 8
    # sliced 8-bit tables: the parked byte sums, B * rows <= 2^31 -- 2^31 / 10^7 = 214.7; at 2^19 rows the fp32 tables
    # (4096 * 256 KiB = 1 GiB) and the byte sums (4096 * 2^19 = 2^31) give out together
    assert S.wide_filter_eligible(214, 10, 16, 4096, 156250) and not S.wide_filter_eligible(215, 10, 16, 4096, 156250)
    assert not S.wide_filter_eligible(1024, 10, 16, 4096, 156250)
    assert S.wide_filter_eligible(4096, 10, 16, 4096, 8192) and not S.wide_filter_eligible(4097, 10, 16, 4096, 8192)
    assert not S.wide_filter_eligible(4096, 10, 16, 4096, 8193) and S.wide_filter_eligible(4095, 10, 16, 4096, 8193)
    # its fallback over 10 M rows: parked fp32 sums of 256 MiB hold 6.7 queries
    assert S.wide_range_form(6, 16, 4096, 156250) == "sliced" and S.wide_range_form(7, 16, 4096, 156250) == "gathered"


def test_wide_filter_fallback_case():
    # m = 2, k = 32768, 2^20 rows, B = 70: 8-bit tables in slices of one quantizer; eligible at the default knobs
    assert S.wf_qw(2, 32768) == 4 and S.wf_slice(2, 32768) == 1
    assert S.wide_filter_eligible(70, 10, 2, 32768, 16384)
    # sample: 17 * sqrt(2^20) / 64 = 272 row blocks; 70 * 272 * 64 * 4 B = 4.6 MiB of parked sums: sliced
    assert S.wide_filter_sample_blocks(16384) == 272 and S.wide_range_form(70, 2, 32768, 272) == "sliced"
    # fallback over every row: 70 * 4 MiB = 280 MiB > 256 MiB: gathered (64 queries are exactly 256 MiB)
    assert S.wide_range_form(70, 2, 32768, 16384) == "gathered" and S.wide_range_form(64, 2, 32768, 16384) == "sliced"


def test_exact_sub_batches():
    # default capacity, range inside it: 32768 * 8 B = 256 KiB per query: 4096
    assert S.exact_sample(1000, 300) == 0 and S.exact_sub_batch(100000, 64, 300) == 4096
    assert S.exact_sub_batch(33, 1000, 5000) == 48                 # (whole tiles of the batch itself)
    assert S.sub_batches(65537, 4096)[-1] == (65536, 1) and len(S.sub_batches(65537, 4096)) == 17
    # the largest capacity, 2^22 entries = 32 MiB: 32 queries
    assert S.exact_sub_batch(40, 64, 300, cap=1 << 22) == 32 and S.sub_batches(40, 32) == [(0, 32), (32, 8)]
    # 10 M rows at K = 1000: S = ceil(2 * 1001 * 10^7 / 32768) = 610 962 rows, 2 443 848 + 262 144 B per query: 396 -> 384
    assert S.exact_sample(1000, 10_000_000) == 610962 and S.exact_sub_batch(1024, 1000, 10_000_000) == 384
    # the sampled GPU case: 40 000 rows all sampled (the knob), capacity 2048: 160 000 + 16 384 B: 6087 -> 6080
    assert S.exact_sample(64, 40000, cap=2048, knob_sample=40000) == 40000
    assert S.exact_sample(64, 40000, cap=2048, knob_sample=10 ** 6) == 40000
    assert S.exact_sub_batch(6088, 64, 40000, cap=2048, knob_sample=40000) == 6080
    assert S.exact_sub_batch(6088, 1000, 40000, cap=2048, knob_sample=40000) == 6080
    assert S.sub_batches(6088, 6080) == [(0, 6080), (6080, 8)]
    # the sample is never shorter than K + 1 nor longer than the automatic maximum
    assert S.exact_sample(1000, 40000, cap=39999, knob_sample=5) == 1001
    assert S.exact_sample(8191, 1 << 30, cap=16) == 1 << 22


def test_grouped_sub_batches():
    # the `test` command on a -p index: 1000 groups, LimitVectors, K = 1000: 2^28 / 10^6 = 268
    assert S.grouped_big_k_sub(1000, 1000, 1000, 1, 10000) == 268
    assert S.grouped_big_k_sub(6, 1000, 1000, 1, 10000) == 6
    # 64 groups, LimitVectors, K = 2048: 2^28 / 2^17 = 2048
    assert S.grouped_big_k_sub(2051, 2048, 64, 1, 1500) == 2048
    assert S.sub_batches(2051, 2048) == [(0, 2048), (2048, 3)]
    # LimitGroups(2048) of 2048 groups at K = 1024: 2^28 / 2^21 = 128; of 2000 groups: 2^28 / 2 048 000 = 131
    assert S.grouped_big_k_sub(131, 1024, 2048, 0, 2048) == 128
    assert S.grouped_big_k_sub(140, 1024, 2000, 0, 2048) == 131
    assert S.grouped_big_k_sub(500, 1024, 2048, 0, 3) == 500       # three groups per query: 87 381 would fit
    assert S.grouped_big_k_sub(500, 1024, 2048, 0, 0) == 500
    # a grid's y extent
    assert S.by_group_takes_batch(65535, 8, 8) and not S.by_group_takes_batch(65536, 8, 8)
    assert not S.by_group_takes_batch(1 << 15, 1 << 14, 8) and not S.by_group_takes_batch(1 << 15, 8, 1 << 13)


def test_stream_redo_chunks():
    # one cluster of 2^24 + 2^20 rows in row order: chunk t ends at 8192 (t + 1) rows; 2^24 / 8192 = 2048 chunks
    n = (1 << 24) + (1 << 20)
    chunks = [S.STREAM_CH] * (n // S.STREAM_CH)
    assert S.stream_redo_chunks(chunks) == list(range(2047, 2048 + 128))
    assert S.stream_redo_chunks([S.STREAM_CH] * 2047 + [8191]) == []
    assert S.stream_redo_chunks([S.STREAM_CH] * 2047 + [8191, 0, 1]) == [2049]
