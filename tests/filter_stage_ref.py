"""The float64 side of test_gpu_filter_stage.py: cases, reference quantities and the checks of one filter stage.

A stage of the quantized lower-bound filters (filter.hip, wide_filter.hip) promises a SET of rows per query.  With
T = Index.prepareQuery's float32 tables, min_j = min_c T_j[c], sum_min = sum_j min_j and a bound tau the kernels quantize

    level_j[c] = min(qmax, floor((T_j[c] - min_j) / delta)),     delta = max(tau' - sum_min, 0) / (qmax - 1)

and keep a row exactly when its levels sum to qmax - 1 or less.  tau' widens tau for the rounding of the reference's
sequential float32 sum D against the real sum R: all terms are >= 0, so D >= R (1 - m u), u = 2^-24, and
tau' = tau (1 + 2 m u) >= tau / (1 - m u) makes  R > tau'  imply  D > tau  (the header comment of filter.hip).  The
kernels evaluate it in float64 with m and u rounded up and a margin for that arithmetic,

    tau' = tau * (1 + 2 * m_pad * 5.97e-8) * (1 + 1e-9)          (m_pad = m for wide codes),

and the reference below takes exactly this value: under `tight` the budget tau' - sum_min is a few 1e-6 of tau, so
1e-9 tau more or less is 1e-3 of a level -- far more than the 2^-19 the level checks resolve.

What check_stage asserts for every query with a finite tau (x = T - min_j, ratio = x / delta, all in float64):
  soundness      every row of the range with D <= tau is queued and the query is not flagged.  No slack.  (A flag is
                 accepted only behind a sub-queue that really overflowed, in a case that does not meet the
                 preconditions below: LOOSE.)
  not too high   level * delta <= x (1 + 1e-12) for every entry (float64 rounding only); a NaN entry has qmax.
  not too low    where float32 has room (delta >= 2^-100 and x >= 2^-100): the kernel's level is floor(r) of an r that
                 misses ratio by at most ratio * 2^-20 (a reciprocal shrunk by 2^-21 and four float32 roundings), so
                 frac(ratio) >= qmax 2^-19 gives floor(ratio) exactly and otherwise floor(ratio) or one less; by the
                 same loss an entry with ratio >= qmax (1 + 2^-19) has qmax, one within [qmax, qmax (1 + 2^-19)) qmax or
                 qmax - 1.  (A saturated entry that comes out lower is too LOW, never too high: that is why this rule
                 stands here and shares the range -- where 1 / delta overflows float32, qt_quantize falls to low levels
                 on purpose, under `subnormal` and `straddle`.)
  not too many   for queries with room: a queued row's levels sum to at most qmax - 1, and entry j lost less than
                 1 + ratio_j 2^-20 of a step, so with S = sum_j ratio_j: S < qmax - 1 + m_pad + S 2^-20, hence
                 R <= sum_min + delta (qmax - 1 + m_pad) (1 + 2^-19).  The rows under this bound are the `upper set`.
  queues         no duplicates, every row inside [from, until), counts equal list lengths.
The preconditions (checked without a GPU, test_oracle_cross.py): the upper set of every query with room holds at most a
quarter of the range's rows and at most the sub-queue capacity -- so `not too many` says something and no queue can
overflow even if every survivor lands in one sub-queue."""
import functools

import numpy as np

import value_regimes as vr

N, B, K, CAP, SEED = 9037, 37, 10, 2048, 3
ROOM = 2.0 ** -100
TAU_MODES = ("K+1-th", "smallest", "below smallest", "64th")

# name: (d, m, k).  The forms of value_regimes and the kernel instantiations they leave out
FLAT_FORMS = {f: s[1:] for f, s in vr.BYTE_FORMS.items()}
FLAT_FORMS.update({"m40": (80, 40, 256), "m48": (96, 48, 256), "m80": (160, 80, 256)})
WIDE_FORMS = {f: s[1:] for f, s in vr.WIDE_FORMS.items()}
WIDE_FORMS.update({"w1024m8": (32, 8, 1024), "w1024m17": (68, 17, 1024), "w2048m12": (48, 12, 2048), "w1500m20": (40, 20, 1500)})
FORMS = {**FLAT_FORMS, **WIDE_FORMS}
SOME_REGIMES = ("tight", "offset", "subnormal")


def regimes_of(form):
    if form in ("m16", "w1024"):
        return vr.FINITE_REGIMES
    return SOME_REGIMES if form in vr.FORMS else ("tight",)


CASES = [(form, regime) for form in FORMS for regime in regimes_of(form)]

# Where the data does not meet the preconditions, by tau mode (CPU figures, n = 9037, whole range, 6-bit levels; the
# oracle and value_regimes alone).  Under `tight` a query's cluster holds ~50 rows, so its 64th smallest distance
# belongs to ANOTHER cluster, the budget is no longer a few 1e-6 of tau and the upper set grows with m: 2070 rows on
# m16, 4800-6400 on m25 / m32 / m36, nearly every row from m40 on, 2409 on w1024m17.  `offset` has uniform codes, and
# from m = 25 on the m_pad steps the bound allows on top of the budget let thousands of rows in at every tau (3462
# of 9037 on m25, all on m64 and m100).  For these queries every check still runs -- each holds whatever the size of
# the upper set -- but a query may be flagged where a sub-queue really overflowed (check_stage).
_WIDER = ("m25", "m32", "m36", "m64", "m100")
LOOSE = {**{(f, "tight"): (3,) for f in ("m16", "m40", "m48", "m80", "w1024m17") + _WIDER},
         **{(f, "offset"): (0, 1, 2, 3) for f in _WIDER}}


def m_pad_of(m, k):
    if k > 256:
        return m
    vec = 16 if m % 16 == 0 else 4
    return -(-m // vec) * vec


def qmax_of(form, nadd=4):
    return 63 if form in WIDE_FORMS else 255 // nadd


def ranges():
    return ((0, N), vr.sub_range(N))


class Ref:
    """cents, idx, Q of one case and T [B][m][k], D [B][n] (float32, j ascending), R [B][n], mins [B][m], sum_min [B] (float64)"""

    def __init__(self, oracle, form, regime, n=N, b=B, data=None):
        self.form, self.regime, self.n, self.b = form, regime, n, b
        self.d, self.m, self.k = FORMS[form]
        self.m_pad = m_pad_of(self.m, self.k)
        with np.errstate(all="ignore"):
            self.cents, self.idx, self.Q = data or vr.query_case(oracle, regime, n, self.d, self.m, self.k, b, seed=SEED)
            self.T = oracle.prepare_query(self.cents, self.d, self.m, self.k, self.Q)
            D = np.zeros((b, n), np.float32)
            R = np.zeros((b, n), np.float64)
            for j in range(self.m):
                t = self.T[:, j, :][:, self.idx[j]]
                D = (D + t).astype(np.float32)
                R += t
            self.D, self.R = D, R
            self.mins = np.fmin.reduce(self.T, axis=2).astype(np.float64)      # NaN entries ignored, as fminf does
            self.sum_min = np.zeros(b, np.float64)
            for j in range(self.m):
                self.sum_min += self.mins[:, j]

    def taus(self, frm, until):
        """the bounds of the batch, rotating: the (K+1)-th smallest D of the range, the smallest, the float below it, the 64th"""
        s = np.sort(self.D[:, frm:until], axis=1)
        tau = np.empty(self.b, np.float32)
        for q in range(self.b):
            mode = q % 4
            tau[q] = (s[q, K], s[q, 0], np.nextafter(s[q, 0], np.float32(-np.inf)), s[q, 63])[mode]
        return tau

    def delta(self, tau, qmax):
        with np.errstate(all="ignore"):
            taup = tau.astype(np.float64) * (1.0 + 2.0 * self.m_pad * 5.97e-8) * (1.0 + 1e-9)
            return np.maximum(taup - self.sum_min, 0.0) / (qmax - 1)

    def upper_bound(self, tau, qmax):
        """R of a queued row is at most this, for a query with room"""
        return self.sum_min + self.delta(tau, qmax) * (qmax - 1 + self.m_pad) * (1.0 + 2.0 ** -19)

    def figures(self, frm, until, tau, qmax):
        """per query: has room, rows with D <= tau, rows of the upper set"""
        room = np.isfinite(tau) & (self.delta(tau, qmax) >= ROOM)
        with np.errstate(invalid="ignore"):
            near = (self.D[:, frm:until] <= tau[:, None]).sum(axis=1)
            upper = (self.R[:, frm:until] <= self.upper_bound(tau, qmax)[:, None]).sum(axis=1)
        return room, near, upper

    def binding(self):
        """[B]: the queries (by their tau mode) for which this case is built to meet the preconditions"""
        return ~np.isin(np.arange(self.b) % 4, LOOSE.get((self.form, self.regime), ()))

    def preconditions(self, frm, until, tau, qmax, cap=CAP):
        room, near, upper = self.figures(frm, until, tau, qmax)
        ok = room & self.binding()
        assert (upper[ok] * 4 <= until - frm).all(), (self.form, self.regime, frm, qmax, int(upper[ok].max()))
        assert (upper[ok] <= cap).all(), (self.form, self.regime, frm, qmax, int(upper[ok].max()))
        # (a bound at or above the smallest distance keeps at least that row: soundness has something to find)
        assert (near[np.arange(self.b) % 4 != 2] >= 1).all() and (near[2::4] == 0).all()
        # at least the three tight bounds of every case bind, but for uniform codes under `offset` on the wider forms
        assert ok.sum() * 4 >= 3 * (self.b - 1) or not room.any() or LOOSE.get((self.form, self.regime)) == (0, 1, 2, 3)
        return room, near, upper

    def pack(self, g):
        """the code arrays as gulon_index_create takes them"""
        pq = g.ProductQuantizer.from_flat(self.k, self.d, self.m, self.cents)
        coder = pq.coder_factory(self.n)
        return np.ascontiguousarray(g.EncodedMatrix(coder, [coder.build_code(self.idx[j]) for j in range(self.m)]).packed())


@functools.lru_cache(maxsize=2)
def reference(oracle, form, regime):
    return Ref(oracle, form, regime)


def check_levels(ref, tau, qmax, levels):
    """levels [B][m][k] against the float64 ideal, for the queries with a finite tau"""
    delta = ref.delta(tau, qmax)
    for q in np.flatnonzero(np.isfinite(tau)):
        lv = levels[q].astype(np.float64)
        T = ref.T[q].astype(np.float64)
        nan = np.isnan(T)
        assert (levels[q][nan] == qmax).all(), (q, "NaN entry below qmax")
        x = np.where(nan, 0.0, T - ref.mins[q][:, None])
        dq = delta[q]
        high = ~nan & (lv * dq > x * (1.0 + 1e-12))
        assert not high.any(), (ref.form, ref.regime, q, "level too high", np.argwhere(high)[:4].tolist(),
                                lv[high][:4].tolist(), (x[high][:4] / dq).tolist())
        if not dq >= ROOM:
            continue
        room = ~nan & (x >= ROOM)
        ratio = x[room] / dq
        fl = np.floor(ratio)
        got = lv[room]
        sat = ratio >= qmax
        want_hi = np.where(sat, qmax, fl)
        exact = np.where(sat, ratio >= qmax * (1.0 + 2.0 ** -19), ratio - fl >= qmax * 2.0 ** -19)
        want_lo = np.where(exact, want_hi, np.maximum(want_hi - 1, 0))
        low = (got < want_lo) | (got > want_hi)
        assert not low.any(), (ref.form, ref.regime, q, "level off the ideal", got[low][:4].tolist(), ratio[low][:4].tolist())


def check_stage(ref, frm, until, tau, qmax, cap, rows, counts, flagged, levels, qt=1, overflow_case=False):
    """One stage's outputs: rows [B][16 cap] (ascending, -1 padded), counts [B][16], flagged [B] (one flag per qt queries),
    levels [B][m][k].  A finite-tau query is not flagged unless a sub-queue of its flag tile overflowed, which the
    preconditions rule out (an upper set within the capacity cannot overflow); an unflagged query is sound and tight.
    Returns per query (queued, D <= tau, upper set, has room) for the baseline table."""
    room, near, upper = ref.figures(frm, until, tau, qmax)
    ub = ref.upper_bound(tau, qmax)
    check_levels(ref, tau, qmax, levels)
    stats = []
    for q in range(ref.b):
        got = rows[q][rows[q] >= 0]
        kept = np.minimum(counts[q], cap)
        assert kept.sum() == len(got) and (counts[q] >= 0).all(), (q, "counts and list length")
        assert (np.diff(got) > 0).all(), (q, "duplicate rows")
        assert len(got) == 0 or (got[0] >= frm and got[-1] < until), (q, "row outside the range")
        stats.append((len(got), int(near[q]), int(upper[q]), bool(room[q])))
        if not np.isfinite(tau[q]):
            assert flagged[q] and len(got) == 0 and (levels[q] == qmax).all(), (q, "unusable bound")
            continue
        if flagged[q]:
            # only after a real overflow in the query's flag tile, and never where the preconditions rule one out
            tile = slice(q // qt * qt, min(ref.b, q // qt * qt + qt))
            over = (counts[tile] > cap).any(axis=1)
            assert over.any(), (ref.form, ref.regime, q, "flagged without an overflow", counts[q].tolist())
            fits = room[tile] & (upper[tile] <= cap)
            assert not (over & fits).any(), (ref.form, ref.regime, q, "overflow with an upper set of", upper[tile].tolist())
            assert overflow_case or not fits.all(), (ref.form, ref.regime, q, "flagged")
            continue
        assert (counts[q] <= cap).all(), (q, "overflow without a flag")
        assert not (overflow_case and near[q] > 16 * cap), (q, "more rows than the queue holds and no flag")
        must = frm + np.flatnonzero(ref.D[q, frm:until] <= tau[q])
        missing = np.setdiff1d(must, got)
        assert len(missing) == 0, (ref.form, ref.regime, q, "dropped rows with D <= tau", missing[:4].tolist(),
                                   ref.D[q, missing[:4]].tolist(), float(tau[q]))
        if room[q]:
            far = got[ref.R[q, got] > ub[q]]
            assert len(far) == 0, (ref.form, ref.regime, q, "queued rows beyond the bound", len(far), len(got), int(upper[q]))
    return stats


# ---- a numpy model of the kernels' arithmetic: what the checks say about a faithful stage and about broken ones ----------
def model_levels(ref, tau, qmax, wide=False, widen=True, shrink=True):
    """qt_quantize's float32 levels (wide: wf_quantize's guarded float64 ones); widen / shrink = False: the two mutations"""
    f32 = np.float32
    out = np.full((ref.b, ref.m, ref.k), qmax, np.uint8)
    with np.errstate(all="ignore"):
        for q in range(ref.b):
            if not tau[q] < np.inf:
                continue
            taup = float(tau[q]) * ((1.0 + 2.0 * ref.m_pad * 5.97e-8) if widen else 1.0) * (1.0 + 1e-9)
            dq = max(max(taup - ref.sum_min[q], 0.0) / (qmax - 1), 1e-290)
            T = ref.T[q]
            mn = ref.mins[q].astype(f32)[:, None]
            if wide:
                x = np.maximum((T.astype(np.float64) - mn.astype(np.float64)) * (1.0 - 8.9e-16), 0.0)
                r = x * (1.0 / dq)
                lv = np.where(r < qmax, np.floor(np.minimum(r, qmax)), qmax)
                for _ in range(3):
                    lv = np.where((lv < qmax) & (lv > 0) & (lv * dq > x), lv - 1, lv)
            else:
                inv = f32(1.0 / dq)
                inv = f32(inv * f32(1.0 - 4.76837158e-7)) if (np.isfinite(inv) and shrink) else (inv if np.isfinite(inv) else f32(3.0e38))
                x = (T - mn).astype(f32)
                x = np.where(x > 0, x, f32(0))
                r = (x * inv).astype(f32)
                lv = np.where(r < f32(qmax), np.floor(np.minimum(r, f32(qmax))), qmax)
            out[q] = np.where(np.isnan(T), qmax, lv).astype(np.uint8)
    return out


def model_stage(ref, frm, until, levels, qmax, extra=0):
    """the rows a stage with these levels queues (extra: added to every sum, a budget test off by that much), as the hooks report them"""
    total = np.zeros((ref.b, until - frm), np.int64)
    for j in range(ref.m):
        total += levels[:, j, :][:, ref.idx[j, frm:until]]
    rows = np.full((ref.b, 16 * CAP), -1, np.int32)
    counts = np.zeros((ref.b, 16), np.int32)
    for q in range(ref.b):
        got = frm + np.flatnonzero(total[q] + extra <= qmax - 1)
        assert len(got) <= 16 * CAP
        rows[q, :len(got)] = got
        counts[q] = [len(got[s::16]) for s in range(16)]
    return rows, counts, np.zeros(ref.b, np.int32)


def reciprocal_edge_taus(ref, qmax, frm, until, queries=12, span=1500):
    """Bounds at which qt_quantize's reciprocal is on its edge: per query the first float32 tau at or above the (K+1)-th
    smallest D for which some entry's quotient x / delta lies so closely below a whole level that a float32 reciprocal
    of delta WITHOUT the 2^-21 shrink carries x * (1 / delta) onto that level -- one level too high.  (Any tau is a
    legitimate bound for a stage; the search uses the numpy model only and looks at the first `queries` queries, the others
    keep the (K+1)-th smallest D.)  Returns (tau [B], found [B])."""
    f32 = np.float32
    start = np.sort(ref.D[:, frm:until], axis=1)[:, K]
    tau, found = start.copy(), np.zeros(ref.b, bool)
    steps = np.arange(span, dtype=np.uint32)
    with np.errstate(all="ignore"):
        for q in range(min(queries, ref.b)):
            cand = (start[q:q + 1].view(np.uint32) + steps).view(f32)                       # consecutive floats (positive)
            taup = cand.astype(np.float64) * (1.0 + 2.0 * ref.m_pad * 5.97e-8) * (1.0 + 1e-9)
            dq = np.maximum(np.maximum(taup - ref.sum_min[q], 0.0) / (qmax - 1), 1e-290)
            inv = (1.0 / dq).astype(f32)
            x = (ref.T[q] - ref.mins[q].astype(f32)[:, None]).astype(f32).reshape(-1)
            x = x[(x > 0) & np.isfinite(x)]
            r = (x[None, :] * inv[:, None]).astype(f32)
            lv = np.where(r < f32(qmax), np.floor(r), 0.0).astype(np.float64)
            bad = (lv * dq[:, None] > x[None, :].astype(np.float64) * (1.0 + 1e-12)).any(axis=1) & np.isfinite(inv)
            if bad.any():
                tau[q], found[q] = cand[np.argmax(bad)], True
    return tau, found
