"""The host-side arithmetic that decides, from a batch's size, how the library cuts it up: restated in plain Python with
no library import, so that a GPU case can assert that it really crosses the seam it is named after
(tests/test_gpu_batch_seams.py) and so that the restatement itself can be held against values worked by hand
(tests/test_batch_seams_ref_host.py).

  wide.hip          run_wide_query: sub-batches of queries whose fp32 tables (and parked sums) fit 1 GiB;
                    launch_scan_wide_range: the three forms of the filter's exact scans
  wide_filter.hip   wf_qw, wf_slice, wide_filter_eligible
  replay.hip        run_tie_replay: flagged queries per round of a wide index
  exact.hip         large_k_dev: queries per sub-batch of the one-pass path
  grouped.hip       run_grouped_query: queries per sub-batch at k_nn > 63
  kmeans_stream.hip the chunks of a cluster that are redone with the plain division"""

GIB = 1 << 30
MAX_K = 63                         # GULON_MAX_K
WIDE_LDS_TABLE = 128 * 1024        # wide.hip
WF_LDS_BUDGET = 144 * 1024         # wide_filter.hip
FILTER_MIN_RB = 512                # ScanTuning's default GULON_FILTER_MIN_RB
RP_MAXF = 1024                     # replay.hip
KNN_QT = 16                        # exact.hpp: queries per tile
EXACT_SAMPLE_MAX = 1 << 22         # exact.hip
EXACT_QUEUE_CAP = 32768            # exact.hip: the default GULON_EXACT_QUEUE_CAP
GRID_Y_MAX = 65535                 # the y extent of a grid
STREAM_CH = 8192                   # kmeans_stream.hip: rows per chunk
EXACT_COUNT = 1 << 24              # a float holds every count below it


def ceil_div(a, b):
    return -(-a // b)


def sub_batches(B, sub):
    """[(q0, nq)] of a `for (q0 = 0; q0 < B; q0 += sub)` loop."""
    return [(q0, min(sub, B - q0)) for q0 in range(0, B, sub)]


def seams(B, sub):
    """The first query of every sub-batch but the first."""
    return list(range(sub, B, sub))


# ---- wide.hip ----------------------------------------------------------------------------------------------------------

def wide_passes(m, k):
    """run_wide_query: (table in LDS?, quantizers per launch, launches per sub-batch)."""
    jp_fit = WIDE_LDS_TABLE // (k * 4)
    lds_t = jp_fit >= 1
    jp = min(jp_fit, m) if lds_t else m
    return lds_t, jp, ceil_div(m, jp)


def wide_form(m, k):
    """'lds': the whole table in LDS; 'sliced': in slices, the sums parked in between; 'gathered': through L2."""
    lds_t, _, passes = wide_passes(m, k)
    return "gathered" if not lds_t else "lds" if passes == 1 else "sliced"


def wide_sub_batch(B, m, k, rows_pad):
    """run_wide_query: the queries whose tables (and, with a sliced table, parked sums) fit in 1 GiB."""
    table_bytes = m * k * 4
    cap = GIB // table_bytes
    if wide_passes(m, k)[2] > 1:
        cap = min(cap, GIB // (rows_pad * 4))
    return max(1, min(B, cap))


def wide_range_form(B, m, k, rb_total):
    """launch_scan_wide_range (the filter's sample scan and its fallback): 'lds', 'sliced' while the parked sums of the
    batch stay within 256 MiB, else 'gathered'."""
    if m * k * 4 <= WIDE_LDS_TABLE:
        return "lds"
    jp = WIDE_LDS_TABLE // (k * 4)
    if jp >= 1 and B * rb_total * 64 * 4 <= (256 << 20):
        return "sliced"
    return "gathered"


def wide_replay_round(B, m, k):
    """run_tie_replay on a wide index: queries per round -- at most 256 MiB of fp32 tables."""
    return max(1, min(B, RP_MAXF, (256 << 20) // (m * k * 4)))


# ---- wide_filter.hip ---------------------------------------------------------------------------------------------------

def wf_qw(m, k):
    """Queries per 8-bit table entry; 0: not even one quantizer's entries fit."""
    if m * k * 8 <= WF_LDS_BUDGET:
        return 8
    if k * 4 <= WF_LDS_BUDGET:
        return 4
    return 0


def wf_slice(m, k):
    """Quantizers per launch of the filter (m: the whole table fits)."""
    qw = wf_qw(m, k)
    if qw == 0:
        return 0
    fit = WF_LDS_BUDGET // (k * qw)
    return m if fit >= m else min(fit, 8)


def wide_filter_eligible(B, K, m, k, rb_total, min_rb=FILTER_MIN_RB, filter_on=True):
    sliced = wf_slice(m, k) < m
    return (filter_on and k > 256 and 1 <= K <= MAX_K and wf_qw(m, k) != 0 and B * m * k * 4 <= GIB
            and rb_total >= 8 * min_rb and (not sliced or B * rb_total * 64 <= 2 * GIB))


def wide_filter_sample_blocks(rb_total):
    """WideFilterBatch::plan: the row blocks of the sample scan."""
    import math
    return min(rb_total // 2, max(256, int(17.0 * math.sqrt(rb_total * 64)) // 64))


# ---- exact.hip ---------------------------------------------------------------------------------------------------------

def exact_sample(K, rng, cap=EXACT_QUEUE_CAP, knob_sample=0):
    """large_k_dev: sample rows S (0: the queue holds the range)."""
    if rng <= cap:
        return 0
    s = knob_sample if knob_sample > 0 else min(ceil_div(2 * (K + 1) * rng, cap), EXACT_SAMPLE_MAX)
    return min(max(s, K + 1), rng)


def exact_sub_batch(B, K, rng, cap=EXACT_QUEUE_CAP, knob_sample=0):
    """large_k_dev: queries per sub-batch -- whole tiles whose sample distances and queues fit 1 GiB."""
    per_query = exact_sample(K, rng, cap, knob_sample) * 4 + cap * 8
    sub = min(GIB // per_query, 1 << 20) // KNN_QT * KNN_QT
    sub = max(sub, KNN_QT)
    return min(sub, ceil_div(B, KNN_QT) * KNN_QT)


# ---- grouped.hip -------------------------------------------------------------------------------------------------------

def grouped_big_k_sub(B, K, g, strategy, limit):
    """run_grouped_query at k_nn > 63: queries whose per-group heaps stay under 2^28 entries.  strategy 0 = LimitGroups,
    1 = LimitVectors (which may search every group)."""
    per_query = max(1, min(g if strategy == 1 else limit, g)) * K
    return max(1, min(B, (1 << 28) // max(1, per_query)))


def by_group_takes_batch(B, nn_stride, g):
    """The batch-size terms of by_group_applies."""
    return B <= GRID_Y_MAX and B * nn_stride <= (1 << 28) and B * g <= (1 << 27)


# ---- kmeans_stream.hip -------------------------------------------------------------------------------------------------

def stream_redo_chunks(counts_per_chunk):
    """stream_chains: of the rows a cluster has in each chunk, the chunks redone because the count reaches 2^24."""
    out, cnt = [], 0
    for t, c in enumerate(counts_per_chunk):
        cnt += c
        if c > 0 and cnt >= EXACT_COUNT:
            out.append(t)
    return out
