"""One stage of the quantized lower-bound filters on its own: the SET of rows it keeps, against float64.

Every other filter test compares final answers with the oracle, and two kinds of error leave those unchanged: a stage
that drops a row between the true K-th distance and its (loose) production bound, and a stage that stopped filtering
(levels too low, a wrapped byte sum, a byte lane of the wrong query) and only sends more work to the exact kernels.
Here the test hooks gulon_selftest_filter_stage (filter_query.hip) and gulon_selftest_wide_filter_stage (wide_filter.hip)
run the production kernels of ONE stage -- bound_tables / qt_quantize / filter_kernel, wf_table_mins / wf_quantize /
wf_filter -- over every row block of a range against bounds the test chooses, and report the queued rows, the
sub-queue counters, the flags and the 8-bit levels.  tests/filter_stage_ref.py holds the reference, the derivation of
every margin and the checks (soundness without slack, levels neither too high nor needlessly low, survivors not
needlessly many, well-formed queues); its preconditions are asserted without a GPU in test_oracle_cross.py.

Data: value_regimes.query_case, n = 9037 (a ragged last block and a ragged last 256-row window), B = 37 (two full
16-query groups and a partial one), the whole range and value_regimes.sub_range; tau rotates over the batch: the
(K+1)-th smallest D (K = 10), the smallest, the float below the smallest, the 64th smallest.  DESIGN.md 9o lists which
case runs which kernel instantiation.  Each hook call prints a `STAGE` line (run with -s): per tau mode the largest
number of queued rows next to the rows with D <= tau and the upper set."""
import ctypes as C

import numpy as np
import pytest

import filter_stage_ref as fs
import value_regimes as vr

pytestmark = pytest.mark.gpu

WIDE_REFUSED = 77
PLAIN, ORDERED, SORTED = 0, 1, 2
COPY_NAMES = ("plain", "window-ordered", "key-sorted")
WHOLE, SUB = fs.ranges()


class Hooks:
    def __init__(self):
        import gulon_amd
        from gulon_amd import native as N
        assert N.device_count() >= 1
        self.g = gulon_amd
        L = C.CDLL(N.HOOKS_LIB_PATH)
        p, i = C.c_void_p, C.c_int32
        self._flat = L.gulon_selftest_filter_stage
        self._flat.restype = i
        self._flat.argtypes = [p, i, i, i, i, p, p, i, i, i, p, i, i, i, i, p, p, p, p, p]
        self._wide = L.gulon_selftest_wide_filter_stage
        self._wide.restype = i
        self._wide.argtypes = [p, i, i, i, i, p, p, i, i, i, p, i, p, p, p, p, p]
        L.gulon_last_error.restype = C.c_char_p
        self._err = L.gulon_last_error

    def _packed(self, ref):
        if getattr(ref, "packed", None) is None:
            ref.packed = ref.pack(self.g)
        return ref.packed

    def _out(self, ref, cap):
        return (np.full((ref.b, 16 * cap), -7, np.int32), np.full((ref.b, 16), -7, np.int32), np.full(ref.b, -7, np.int32),
                np.full((ref.b, ref.m, ref.k), 0xEE, np.uint8), np.full(8, -7, np.int32))

    def flat(self, ref, frm, until, tau, copy=PLAIN, nadd=4, cap=fs.CAP, main=1):
        rows, counts, flagged, levels, info = self._out(ref, cap)
        tau = np.ascontiguousarray(tau, np.float32)
        rc = self._flat(self._packed(ref).ctypes.data, ref.n, ref.d, ref.m, ref.k, ref.cents.ctypes.data, ref.Q.ctypes.data,
                        ref.b, frm, until, tau.ctypes.data, copy, nadd, cap, main, rows.ctypes.data, counts.ctypes.data,
                        flagged.ctypes.data, levels.ctypes.data, info.ctypes.data)
        assert rc == 0, (rc, self._err())
        assert info[0] == 255 // nadd and info[1] == ref.m_pad
        return rows, counts, flagged, levels, info

    def wide(self, ref, frm, until, tau, cap=fs.CAP, expect=0):
        rows, counts, flagged, levels, info = self._out(ref, cap)
        tau = np.ascontiguousarray(tau, np.float32)
        rc = self._wide(self._packed(ref).ctypes.data, ref.n, ref.d, ref.m, ref.k, ref.cents.ctypes.data, ref.Q.ctypes.data,
                        ref.b, frm, until, tau.ctypes.data, cap, rows.ctypes.data, counts.ctypes.data, flagged.ctypes.data,
                        levels.ctypes.data, info.ctypes.data)
        assert rc == expect, (rc, self._err())
        assert expect != 0 or info[0] == 63
        return rows, counts, flagged, levels, info


@pytest.fixture(scope="module")
def hooks():
    return Hooks()


def _report(ref, what, frm, stats):
    s = np.array([t[:3] for t in stats])
    per_mode = " | ".join("%s %d/%d/%d" % (fs.TAU_MODES[mode], *s[mode::4].max(axis=0)) for mode in range(4))
    print(f"STAGE {ref.form} {ref.regime} {what} from={frm}: queued/D<=tau/upper set, largest per tau mode: {per_mode}")


def _flat_run(hooks, ref, rng_, copy, nadd, main, tau=None, cap=fs.CAP, **kw):
    frm, until = rng_
    tau = ref.taus(frm, until) if tau is None else tau
    rows, counts, flagged, levels, info = hooks.flat(ref, frm, until, tau, copy, nadd, cap, main)
    stats = fs.check_stage(ref, frm, until, tau, 255 // nadd, cap, rows, counts, flagged, levels, qt=int(info[2]), **kw)
    _report(ref, f"{COPY_NAMES[copy]} nadd={nadd} qw={info[3]} nqg={info[4]} chunks={info[5]}", frm, stats)
    return info


def _wide_run(hooks, ref, rng_, tau=None, cap=fs.CAP, **kw):
    frm, until = rng_
    tau = ref.taus(frm, until) if tau is None else tau
    rows, counts, flagged, levels, info = hooks.wide(ref, frm, until, tau, cap)
    stats = fs.check_stage(ref, frm, until, tau, 63, cap, rows, counts, flagged, levels, **kw)
    _report(ref, f"wide qw={info[1]} slice={info[2]} chunks={info[3]}", frm, stats)
    return info


# (copy, nadd, range, main stage tag) of a flat case: both NADD values, both ranges; the one-word form (m16, nadd = 4)
# through each of its three code copies, the key-sorted one over the whole range only
# (the tag also shapes the hook's launch: 1 = two long chunks over the whole range, every wave at work; 0 = many short ones)
M16_RUNS = [(PLAIN, 4, WHOLE, 1), (PLAIN, 4, SUB, 0), (PLAIN, 2, WHOLE, 0), (PLAIN, 2, SUB, 1),
            (ORDERED, 4, WHOLE, 1), (ORDERED, 4, SUB, 0), (SORTED, 4, WHOLE, 1), (SORTED, 4, WHOLE, 0)]
OTHER_RUNS = [(PLAIN, 4, WHOLE, 1), (PLAIN, 2, SUB, 0), (PLAIN, 2, WHOLE, 0), (PLAIN, 4, SUB, 1)]
# queries per entry, entry groups per workgroup (filter_qw / filter_nqg)
FLAT_SHAPE = {"m16": (16, 1), "m8": (16, 2), "m25": (16, 1), "m32": (16, 1), "m36": (16, 1), "m64": (8, 1), "m100": (4, 1),
              "k5": (16, 2), "m40": (8, 1), "m48": (8, 1), "m80": (4, 1)}


@pytest.mark.parametrize("form,regime", [c for c in fs.CASES if c[0] in fs.FLAT_FORMS])
def test_flat_stage_keeps_the_right_rows(oracle, hooks, form, regime):
    ref = fs.reference(oracle, form, regime)
    for copy, nadd, rng_, main in (M16_RUNS if form == "m16" else OTHER_RUNS):
        info = _flat_run(hooks, ref, rng_, copy, nadd, main)
        assert (info[3], info[4]) == FLAT_SHAPE[form] and (info[5] > 1 or rng_ == SUB)   # the instantiation DESIGN.md 9o names; several chunks


# queries per entry, quantizers per launch (wf_qw / wf_slice: below m = the sliced walk)
WIDE_SHAPE = {"w1024": (8, 16), "w4096": (4, 8), "w5000": (4, 7), "w16384": (4, 2), "w1024m8": (8, 8), "w1024m17": (8, 17),
              "w2048m12": (4, 12), "w1500m20": (4, 20)}


@pytest.mark.parametrize("form,regime", [c for c in fs.CASES if c[0] in fs.WIDE_FORMS])
def test_wide_stage_keeps_the_right_rows(oracle, hooks, form, regime):
    ref = fs.reference(oracle, form, regime)
    for rng_ in (WHOLE, SUB):
        info = _wide_run(hooks, ref, rng_)
        assert (info[1], info[2]) == WIDE_SHAPE[form] and (info[3] > 1 or rng_ == SUB)


def test_wide_hook_reports_a_refused_code_book(hooks):
    """wf_qw refuses a code book of which not even one quantizer's four-query entries fit LDS (k > 36 864): the hook
    answers with its own code, not with an empty result.  Every form of value_regimes.WIDE_FORMS is accepted (above)."""
    rng = np.random.default_rng(5)
    ref = fs.Ref.__new__(fs.Ref)
    ref.n, ref.b, ref.d, ref.m, ref.k = 300, 2, 4, 2, 40000
    ref.cents = rng.standard_normal(ref.k * ref.d).astype(np.float32)
    ref.idx = rng.integers(0, ref.k, (ref.m, ref.n)).astype(np.int32)
    ref.Q = rng.standard_normal((ref.b, ref.d)).astype(np.float32)
    hooks.wide(ref, 0, ref.n, np.ones(ref.b, np.float32), cap=64, expect=WIDE_REFUSED)


@pytest.mark.parametrize("kind", ["plain", "window-ordered", "key-sorted", "wide"])
def test_unusable_bounds_are_flagged(oracle, hooks, kind):
    """tau = +inf / NaN for the first 16 queries (whole flag tiles), finite for the rest: those are flagged, queue nothing
    and have every level at qmax; the others are filtered as ever."""
    ref = fs.reference(oracle, "w1024" if kind == "wide" else "m16", "mixed_mild")
    tau = ref.taus(*WHOLE)
    tau[0:16:2], tau[1:16:2] = np.inf, np.nan
    if kind == "wide":
        _wide_run(hooks, ref, WHOLE, tau)
    else:
        _flat_run(hooks, ref, WHOLE, COPY_NAMES.index(kind), 4, 1, tau)


def _decoded_rows_case(oracle, form):
    """`tight` with queries that ARE decoded rows and a second copy of each such row elsewhere: D = 0 twice per query"""
    base = fs.reference(oracle, form, "tight")
    rng = np.random.default_rng(11)
    pick = rng.permutation(fs.N)[: 2 * fs.B]
    rows, twins = pick[: fs.B], pick[fs.B:]
    idx = base.idx.copy()
    idx[:, twins] = idx[:, rows]
    Q = vr.decode(base.cents, idx[:, rows], base.d, base.m, base.k)
    ref = fs.Ref(oracle, form, "tight", data=(base.cents, idx, Q))
    assert (ref.D[np.arange(fs.B), rows] == 0).all() and (ref.D[np.arange(fs.B), twins] == 0).all() and (ref.sum_min == 0).all()
    return ref


@pytest.mark.parametrize("kind", ["plain", "window-ordered", "key-sorted", "wide"])
def test_budget_zero_keeps_the_rows_at_distance_zero(oracle, hooks, kind):
    ref = _decoded_rows_case(oracle, "w1024" if kind == "wide" else "m16")
    tau = np.zeros(fs.B, np.float32)
    assert ((ref.D <= 0).sum(axis=1) >= 2).all() and (ref.delta(tau, 63) == 0).all()
    if kind == "wide":
        _wide_run(hooks, ref, WHOLE, tau)
    else:
        _flat_run(hooks, ref, WHOLE, COPY_NAMES.index(kind), 4, 1, tau)
        if kind == "plain":
            _flat_run(hooks, ref, WHOLE, PLAIN, 2, 0, tau)


@pytest.mark.parametrize("kind", ["plain", "key-sorted", "wide"])
def test_overflowing_queues_are_flagged(oracle, hooks, kind):
    """64 entries per sub-queue against the 2000th smallest D: a query may be flagged only where an upper set exceeds the 64
    (here all do), must be once its D <= tau rows exceed 16 x 64 (all do), and an unflagged query is still sound."""
    ref = fs.reference(oracle, "w1024" if kind == "wide" else "m16", "mixed_mild")
    tau = np.sort(ref.D, axis=1)[:, 1999].copy()
    if kind == "wide":
        _wide_run(hooks, ref, WHOLE, tau, cap=64, overflow_case=True)
    else:
        _flat_run(hooks, ref, WHOLE, COPY_NAMES.index(kind), 4, 1, tau, cap=64, overflow_case=True)


@pytest.mark.parametrize("regime,nadd", [("large", 4), ("mixed_mild", 4), ("mixed_mild", 2)])
def test_flat_levels_where_the_reciprocal_is_on_its_edge(oracle, hooks, regime, nadd):
    """Bounds chosen (filter_stage_ref.reciprocal_edge_taus) so that some entry's quotient sits within 2^-23 below a whole
    level: without the 2^-21 shrink of 1 / delta in qt_quantize that entry comes out one level too high."""
    ref = fs.reference(oracle, "m16", regime)
    tau, found = fs.reciprocal_edge_taus(ref, 255 // nadd, *WHOLE, queries=12)
    assert found.sum() >= 6
    _flat_run(hooks, ref, WHOLE, PLAIN, nadd, 1, tau)
