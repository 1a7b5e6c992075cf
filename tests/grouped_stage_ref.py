"""The float64 side of test_gpu_grouped_stage.py: cases, reference quantities, checks and a numpy model of the grouped pre-selection.

The grouped index (grouped.hip) answers a query from 64 candidate rows: the rows of the searched groups with the smallest

    D~ = (|q|^2 - 2 q.g) + |x^|^2 + sum_j P[j][code_j],     P[j][c] = -2 q_j . c_j[c],    x^ = g + decode(codes),

whose real-number value is D(q, row) = |q - x^|^2.  gq_rerank re-scores the 64 with the reference's arithmetic and
certifies the answer when the (K+1)-th exact distance lies below a_last - margin (a_last = the 64th listed D~),

    margin = E = 4 (d + 2 m + 16) 2^-24 (|q| + sqrt(xnmax))^2 .

That rests on two promises nothing else tests: the list IS the 64 smallest (D~, row) of all searched rows, and
|D~ - D| <= E.  The hook gulon_selftest_grouped_stage runs the pre-selection alone, both ways on the same nn lists --
by group (grouped_filter.hip: gf_quant, gf_tiles, gf_filter, gf_survivors) and gq_ptables + gq_approx_scan + merge -- and
gq_rerank on each list, and returns every intermediate (`out`, a dict; stage_model() below produces the same dict in numpy).

Data (Case): synthesized in numpy, no training.  Group centroids uniform in [-S, S]^d (+ a shift), group sizes from a
multinomial (or as the case prescribes), unit-variance residuals, PQ centroids sampled from the residuals' sub-vectors,
codes by nearest centroid, offsets from the sizes; a query = the centroid of a random row's group + a fresh unit-variance
residual.  All inputs are float32; every reference quantity is float64 arithmetic on them, u = 2^-24.

What check_stage asserts (each bound is derived where it is used; "dev" = as the device returned it):
  index state   xnlo[c] = the smallest dev xnorm of the group, bit for bit (0 for an empty group); gnmax / xnmax = the maxima,
                bit for bit; xn_step = fl(max_c fl(hi_c - lo_c) / 255), bit for bit; xnlo + xcode xn_step <= xnorm for every
                row and xcode is floor((xnorm - xnlo) / xn_step) or one less (the reciprocal is shrunk by 2^-20 and rounded
                three times: 255 (2^-20 + 3 u) < 1 code lost at most); |xnorm - real| <= (d + 4) u real: v = fl(g + c) has u,
                v^2 another 2 u + u, a sequential sum of d terms >= 0 at most (d - 1) u; |gnorm - real| <= (d + 2) u real (any
                summation order of d squares); |P - real| <= 2 (s + 1) u sum_t |q_t c_t| for an s-wide sub-vector, 0 beyond k
                and on padding quantizers.
  pairs, tiles  gcnt[c] = the queries with c in their nn list, c not empty; the tiles list every (query, non-empty searched
                group) pair exactly once, groups ascending, ceil(gcnt / 16) tiles per group with nq = 16 but in the last,
                r0 / r1 / xl the group's bounds and xnlo, padding slots = the last query, pad = 0; meta = {tiles, pairs}.
  threshold     (check_threshold; check_budget replays budget0 bit-near from the dev values)  gf_quant's sample: groups in nn order while fewer than 256 rows are sampled, at most 16 groups, at most 2048
                rows.  tq = the 64th smallest D~ of it; the 64th order statistic moves by at most max |D~ - D| <= E, so
                budget0 + sumlo - margin lies within E of the 64th smallest D of that sample, up to the float32 rounding of
                (tq + margin) - sumlo and of sumlo: 4 u (|tq| + E + m sum_j |lo_j|).  Fewer than 64 sampled rows (or
                non-finite inputs): 1 / step = 0.  Otherwise 1 / step = 252 / (1.001 (budget0 - minbase)) within 1e-4
                (minbase from the dev cdist, gnorm, xnlo; |q|^2 is a wave sum whose order is not modelled).
  levels        with x = P[j][c] - lo_j (exact in float64) and r = x / step: level <= r (never too high: three roundings
                of u against the 2^-20 shrink), level = min(255, floor(r)) or one less, and exactly that when
                frac(r) >= r 2^-19; 255 for c >= k on real quantizers, 0 on padding quantizers; the same for the norm
                table with x = c xn_step.  1 / step = 0: every real level is 0.
  soundness     query with 1 / step != 0 and qcnt <= GF_CAP: every searched row with D <= T64 - 2 E is queued (T64 = the
                64th smallest D over ALL its searched rows: the sample's rows are searched rows, so tq >= the 64th smallest
                D~ >= T64 - E, and such a row has D~ <= T64 - E).  No slack beyond E itself.  1 / step = 0: every searched
                row.  Always: no row twice, no row outside the searched groups, qcnt = entries; a pair's base is one bit
                pattern and within (d + 3) u (|q|^2 + 2 sum |q_e g_e|) of |q|^2 - 2 q.g.
  tightness     a row is queued when its 17 levels sum to less than lim = floor(A) + 2, A = (budget0 - base - xl) / step,
                so sum <= A + 1.  A real table's level is > r_j - 1 - r_j 2^-19, the norm level > (c xn_step) / step - 1
                with c xn_step > xnorm - xl - xn_step: the sum exceeds (D~ - sumlo - base - xl - xn_step) / step - (m + 1).
                Hence D <= budget0 + sumlo + (m + 2) step + xn_step + E (c1 = m + 2: one step per real table, one for the
                norm table, one in lim -- the second unit of `+ 2` turns "below" into "at most"), widened by 0.01 step and
                8 u (|base| + |xl| + |budget0|) for A's own roundings.  The rows under this bound are the `upper set`.
  lists         (each path) ascending by (value, row), rows distinct and searched, padded with (+inf, INT_MAX) behind
                min(64, searched rows); unflagged: every searched row with D < L - 2 E listed, every listed row has
                D <= L + 2 E (L = T64), and |lv - D| <= E for every listed value -- the margin's own claim.  Both lists equal
                the 64 smallest (D~, row) under approx_row_sum's float32 arithmetic replayed in numpy from the dev base,
                xnorm and P (over the queued rows / over every searched row), bit for bit; hence each other.
  flags         by group: anan[q][0] = a NaN D~ among the queued rows, or qcnt > GF_CAP, or more than GF_PLACED entries at
                or below the 64th smallest; nothing else.  Scan: a NaN D~ among the searched rows.
  certificate   from the dev list, margin in float32 and the reference's arithmetic on the listed rows (gq_rerank's =
                oracle.grouped_query's): redone iff flagged, or a NaN exact distance, or equal neighbours among the K + 1
                best, or 64 candidates and not ek < a_last - margin.  |ek - (a_last - margin)| <= 2^-21 (|a_last| + margin)
                is not judged (the float32 sqrt and |q|^2 may round either way): at most one query in ten, none on the
                CPU figures.  Not redone: out_idx / out_dist / out_count = oracle.grouped_query's.
The preconditions (test_oracle_cross.py, no GPU): every query's upper set holds at most a third of its searched rows and
fewer than GF_CAP rows, and every regular case has a query with 64 or more searched rows; LOOSE names the cases that
cannot meet the first (every check still runs on them)."""
import functools

import numpy as np

U = 2.0 ** -24
N, B, G, LIMIT, S, K, SEED = 9037, 37, 48, 20, 10.0, 10, 7
GF_CAP, GF_PLACED, GF_QT, GF_NT, GF_SAT, GF_LEVELS = 16384, 512, 16, 17, 255, 252.0
GF_SHRINK = np.float32(0.99999905)
SAMPLE_GROUPS, SAMPLE_ROWS, LIST = 16, 2048, 64
INT_MAX = 2 ** 31 - 1
f32 = np.float32

BASE = dict(n=N, b=B, g=G, limit=LIMIT, s=S, kk=K, d=32, m=16, k=256, strategy=0, shift=0.0, sizes=None, queries=None, bad=None)
# name: what differs from BASE (DESIGN.md 9p lists the instantiation each case runs)
CASES = {
    "m16": {},
    "m8": dict(m=8, k=64), "m5": dict(d=20, m=5, k=16), "m12": dict(d=24, m=12, k=64), "m3": dict(d=9, m=3, k=40),
    "d128": dict(d=128, m=8, k=64), "d129": dict(d=129, m=5, k=64), "d200": dict(d=200, m=8, k=64), "d5": dict(d=5, m=5, k=64),
    "g90": dict(g=90, sizes="ragged"),
    # (the 2500-row group has residuals of twice the spread, its queries too: with unit spread the 64 nearest of 2500 rows
    # lie 18 steps from nearly all of the group, and the upper set would be the whole group)
    "big_group": dict(sizes="one2500", queries="third_in_big"),
    "b16": dict(b=16, queries="one_group"), "b17": dict(b=17, queries="one_group"), "b1": dict(b=1, queries="one_group"),
    "rows8": dict(g=1130, limit=17), "rows3": dict(g=3012, limit=17),
    "vectors1500": dict(strategy=1, limit=1500),
    "k1": dict(kk=1), "k63": dict(kk=63),
    "s3": dict(s=3.0), "s30": dict(s=30.0), "shifted": dict(shift=1000.0),
    "nan": dict(bad="nan"), "inf": dict(bad="inf"), "huge": dict(bad="huge"),
    "copies600": dict(sizes="one700", queries="copies", copies=600),
    "copies17000": dict(n=20000, sizes="one17500", queries="copies", copies=17000),
}
REGULAR = [c for c in CASES if c not in ("rows3", "nan", "inf", "huge", "copies600", "copies17000")]
FINITE = [c for c in CASES if c not in ("nan", "inf", "huge")]
# cases that cannot keep the upper set within a third of the searched rows (CPU figures, test_oracle_cross.py):
#   shifted    |g| ~ 1000: xn_step, the in-group range of |x^|^2 / 255, is ~ 4 |g| |r| 2 / 255 ~ 100 against in-group distances of
#              ~ 2 d = 64, so one norm level swallows the group (the issue expects this)
#   rows8      a query searches ~ 136 rows and 64 of them are listed
#   rows3      fewer than 64 searched rows: every row is kept by design
#   copies*    the copies ARE the 64 smallest and far more than a third of what their queries search
LOOSE = ("shifted", "rows8", "rows3", "copies600", "copies17000")
BIG_GROUP = 5           # the group the size recipes enlarge and the `one_group` / `copies` queries sit in


def m_pad_of(m):
    return m if m % 16 == 0 else -(-m // 4) * 4


class Case:
    """One case's inputs (float32 / int32) and float64 reference quantities: D [b][n], xn [n], P [b][m][k], E [b], ..."""

    def __init__(self, oracle, name):
        p = {**BASE, **CASES[name]}
        self.name, self.p = name, p
        self.n, self.b, self.g, self.limit, self.kk = p["n"], p["b"], p["g"], p["limit"], p["kk"]
        self.d, self.m, self.k, self.strategy = p["d"], p["m"], p["k"], p["strategy"]
        self.m_pad = m_pad_of(self.m)
        n, b, g, d, m, k = self.n, self.b, self.g, self.d, self.m, self.k
        rng = np.random.default_rng(SEED + sum(map(ord, name)))
        fr, un = oracle.subvectors(d, m)
        self.fr, self.un = fr.astype(int), un.astype(int)
        self.gcent = (rng.uniform(-p["s"], p["s"], (g, d)) + p["shift"] / np.sqrt(d)).astype(f32)
        self.sizes = self._sizes(rng, p["sizes"])
        assert self.sizes.sum() == n and len(self.sizes) == g
        self.bounds = np.r_[0, np.cumsum(self.sizes)].astype(np.int64)
        self.offsets = self.bounds[1:-1].astype(np.int32)
        self.group_of = np.repeat(np.arange(g), self.sizes)
        R = rng.standard_normal((n, d)).astype(f32)
        wide = f32(3.0 if p["sizes"] == "one2500" else 1.0)    # (see CASES: the 2500-row group)
        R[self.bounds[BIG_GROUP]:self.bounds[BIG_GROUP + 1]] *= wide
        self.cents = np.zeros(k * d, f32)                      # quantizer j: [k][s_j] at k * from_j
        self.idx = np.zeros((m, n), np.int32)
        dec = np.zeros((n, d), np.float64)
        for j in range(m):
            f, u_ = self.fr[j], self.un[j]
            cj = R[rng.choice(n, k, replace=n < k), f:u_].astype(np.float64)
            self.cents[k * f:k * u_] = cj.astype(f32).reshape(-1)
            sub = R[:, f:u_].astype(np.float64)
            d2 = (sub ** 2).sum(1)[:, None] - 2.0 * sub @ cj.T + (cj ** 2).sum(1)[None, :]
            self.idx[j] = np.argmin(d2, axis=1)
        copies = p.get("copies", 0)
        r0 = int(self.bounds[BIG_GROUP])
        if copies:                                              # rows r0 .. r0 + copies - 1 of one group are one row
            self.idx[:, r0:r0 + copies] = self.idx[:, r0:r0 + 1]
        for j in range(m):
            f, u_ = self.fr[j], self.un[j]
            dec[:, f:u_] = self.cents[k * f:k * u_].reshape(k, u_ - f).astype(np.float64)[self.idx[j]]
        self.xhat = self.gcent.astype(np.float64)[self.group_of] + dec
        self.xn = (self.xhat ** 2).sum(1)
        # queries
        rows = rng.integers(0, n, b)
        if p["queries"] == "one_group":
            rows = rng.integers(r0, self.bounds[BIG_GROUP + 1], b)
        elif p["queries"] == "copies":                          # (the others: rows of other groups)
            rows = (rng.integers(0, n - self.sizes[BIG_GROUP], b) + self.bounds[BIG_GROUP + 1]) % n
        elif p["queries"] == "third_in_big":
            rows[::3] = rng.integers(r0, self.bounds[BIG_GROUP + 1], len(rows[::3]))
        Q = (self.gcent[self.group_of[rows]] + rng.standard_normal((b, d)) * np.where(self.group_of[rows] == BIG_GROUP, wide, 1)[:, None]).astype(f32)
        if p["queries"] == "copies":                            # every third query AT the copied row (to float32)
            Q[::3] = self.xhat[r0].astype(f32)
        if p["bad"]:
            Q[3, d // 2] = {"nan": np.nan, "inf": np.inf, "huge": Q[3, d // 2]}[p["bad"]]
            if p["bad"] == "huge":
                Q[3] *= f32(1e20)
        self.Q = Q
        self.bad_q = np.array([3]) if p["bad"] else np.array([], int)
        with np.errstate(all="ignore"):
            q64 = Q.astype(np.float64)
            self.qq = (q64 ** 2).sum(1)
            self.D = self.qq[:, None] - 2.0 * q64 @ self.xhat.T + self.xn[None, :]
            self.D = np.where(np.isfinite(self.D), np.maximum(self.D, 0.0), self.D)
            self.P = np.zeros((b, m, k))
            for j in range(m):
                f, u_ = self.fr[j], self.un[j]
                cj = self.cents[k * f:k * u_].reshape(k, u_ - f).astype(np.float64)
                self.P[:, j, :] = -2.0 * q64[:, f:u_] @ cj.T
            self.qg = q64 @ self.gcent.astype(np.float64).T                       # [b][g]
            self.qg_abs = np.abs(q64) @ np.abs(self.gcent.astype(np.float64)).T
            self.E = 4.0 * (d + 2 * m + 16) * U * (np.sqrt(self.qq) + np.sqrt(self.xn.max())) ** 2
            # |q|^2 and |q|^2 - 2 q.g as every kernel here forms them: lane l adds the products of coordinates l, l + 64, ...
            # in float32, wave_sum folds the 64 partial sums by xor 32, 16, .. 1 -- one bit pattern, replayed
            self.qq32 = self.wave_dot(Q, Q[:, None, :])[:, 0]
            self.base32 = (self.qq32[:, None] - f32(2.0) * self.wave_dot(Q, self.gcent[None, :, :])).astype(f32)

    @staticmethod
    def wave_dot(A, Bm):
        """[b][x] float32 dot products of A [b][d] with Bm [b or 1][x][d], in the kernels' wave order"""
        b, d = A.shape
        part = np.zeros((b, Bm.shape[1], 64), f32)
        for e0 in range(0, d, 64):
            w = min(64, d - e0)
            part[:, :, :w] = (part[:, :, :w] + (A[:, None, e0:e0 + w] * Bm[:, :, e0:e0 + w]).astype(f32)).astype(f32)
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            part = (part + part[:, :, lanes ^ o]).astype(f32)
        return part[:, :, 0]

    def _sizes(self, rng, recipe):
        n, g = self.n, self.g
        if recipe is None:
            return rng.multinomial(n, np.full(g, 1.0 / g))
        if recipe == "ragged":                                  # sizes 1 .. 200, groups 0, 17, 18 and 63 empty
            sz = rng.integers(1, 201, g)
            sz[[0, 17, 18, 63]] = 0
            live = np.flatnonzero(sz)
            while sz.sum() != n:
                c = rng.choice(live)
                step = int(np.sign(n - sz.sum()))
                if 1 <= sz[c] + step <= 200:
                    sz[c] += step
            return sz
        big = {"one2500": 2500, "one700": 700, "one17500": 17500}[recipe]
        sz = rng.multinomial(n - big, np.full(g - 1, 1.0 / (g - 1)))
        return np.insert(sz, BIG_GROUP, big)

    def pack(self, gulon):
        """the code bytes as gulon_grouped_index_create takes them"""
        pq = gulon.ProductQuantizer.from_flat(self.k, self.d, self.m, self.cents)
        coder = pq.coder_factory(self.n)
        return np.ascontiguousarray(gulon.EncodedMatrix(coder, [coder.build_code(self.idx[j]) for j in range(self.m)]).packed())

    def searched(self, nn, nn_cnt, q):
        """the rows query q searches, ascending, and the group of each"""
        cs = [int(c) for c in nn[q, :nn_cnt[q]]]
        rows = np.concatenate([np.arange(self.bounds[c], self.bounds[c + 1]) for c in cs] + [np.zeros(0, np.int64)]).astype(np.int64)
        rows.sort()
        return rows

    def approx32(self, base, xnorm, P, q, rows):
        """approx_row_sum in numpy float32: (base + xnorm[row]) + P[0][code_0] + ... in quantizer order (padding adds +0)"""
        with np.errstate(all="ignore"):
            acc = (base.astype(f32) + xnorm[rows]).astype(f32)
            for j in range(self.m_pad):
                acc = (acc + (P[q, j, self.idx[j, rows]] if j < self.m else f32(0))).astype(f32)
        return acc

    def exact32(self, q, rows):
        """gq_rerank's distance of the rows: MathUtils.subtract, Index.prepareQuery and PQIndex.distances in float32"""
        grp = np.searchsorted(self.bounds[:self.g], rows, side="right") - 1
        with np.errstate(all="ignore"):
            res = (self.Q[q][None, :] - self.gcent[grp]).astype(f32)
            Dv = np.zeros(len(rows), f32)
            for j in range(self.m):
                f, u_ = self.fr[j], self.un[j]
                cj = self.cents[self.k * f:self.k * u_].reshape(self.k, u_ - f)[self.idx[j, rows]]
                tj = np.zeros(len(rows), f32)
                for t in range(u_ - f):
                    dd = (res[:, f + t] - cj[:, t]).astype(f32)
                    tj = (tj + (dd * dd).astype(f32)).astype(f32)
                Dv = (Dv + tj).astype(f32)
        return Dv

    def oracle_answer(self, oracle):
        if getattr(self, "_answer", None) is None:
            with np.errstate(all="ignore"):
                self._answer = oracle.grouped_query(self.idx, self.d, self.k, self.cents, self.gcent, self.offsets, self.Q, self.kk,
                                                    self.strategy, self.limit)
        return self._answer


@functools.lru_cache(maxsize=4)
def case(oracle, name):
    return Case(oracle, name)


def ordered_key(v):
    """select.hpp's order-preserving key of a float32 (NaN never reaches it: the kernels replace it by +inf)"""
    bits = np.asarray(v, f32).view(np.uint32).astype(np.int64)
    return np.where(bits & 0x80000000, 0xFFFFFFFF - bits, bits | 0x80000000)


def smallest64(vals, rows):
    """the LIST smallest (value, row), ascending, padded; NaN counts as +inf"""
    v = np.where(np.isnan(vals), f32(np.inf), vals).astype(f32)
    order = np.lexsort((rows, ordered_key(v)))[:LIST]
    lv = np.full(LIST, np.inf, f32)
    li = np.full(LIST, INT_MAX, np.int64)
    lv[:len(order)], li[:len(order)] = v[order], rows[order]
    return lv, li


def sample_rows(cs, nn, nn_cnt, q):
    """gf_quant's threshold sample: groups in nn order while fewer than 256 rows, <= 16 groups, <= 2048 rows"""
    out, total = [], 0
    for t in range(min(int(nn_cnt[q]), SAMPLE_GROUPS)):
        if total >= 256:
            break
        c = int(nn[q, t])
        cnt = min(int(cs.sizes[c]), SAMPLE_ROWS - total)
        if cnt <= 0:
            continue
        out.append(np.arange(cs.bounds[c], cs.bounds[c] + cnt))
        total += cnt
    return np.concatenate(out + [np.zeros(0, np.int64)]).astype(np.int64)


def upper_bound(cs, out, q):
    """D of a queued row is at most this (the docstring's tightness bound), for a query with 1 / step != 0"""
    bud, inv = float(out["qs"][q, 0]), float(out["qs"][q, 1])
    lo = out["P"][q, :cs.m, :cs.k].astype(np.float64).min(axis=1)
    step = 1.0 / inv
    big = np.abs(cs.qq[q]) + 2.0 * cs.qg_abs[q].max() + float(out["xnlo"].max()) + abs(bud)
    return bud + lo.sum() + (cs.m + 2.01) * step + float(out["scalars"][1]) * 1.00001 + cs.E[q] + 8.0 * U * big


def figures(cs, out, q):
    """(searched rows, rows that must be kept, upper set) of a query with 1 / step != 0"""
    rows = cs.searched(out["nn"], out["nn_cnt"], q)
    Dq = cs.D[q, rows]
    t64 = np.sort(Dq)[LIST - 1] if len(rows) >= LIST else np.inf
    return len(rows), int((Dq <= t64 - 2.0 * cs.E[q]).sum()), int((Dq <= upper_bound(cs, out, q)).sum())


def preconditions(cs, out):
    """what the data must give for the tightness check to say something and no queue to overflow (see the docstring)"""
    most = 0
    for q in range(cs.b):
        if q in cs.bad_q or out["qs"][q, 1] == 0:
            continue
        nrows, must, upper = figures(cs, out, q)
        most = max(most, nrows)
        copies_query = cs.p["queries"] == "copies" and q % 3 == 0
        assert upper < GF_CAP or (cs.name == "copies17000" and copies_query), (cs.name, q, upper)
        assert cs.name in LOOSE or upper * 3 <= nrows, (cs.name, q, "upper set", upper, "of", nrows, "must keep", must)
    assert cs.name not in REGULAR or most >= LIST, (cs.name, "no query with 64 searched rows")


def check_index_state(cs, out):
    n, g, d, m, k = cs.n, cs.g, cs.d, cs.m, cs.k
    xnorm, xnlo, xcode, gnorm = out["xnorm"], out["xnlo"], out["xcode"], out["gnorm"]
    xnmax, xn_step, gnmax = out["scalars"][:3]
    assert (np.abs(xnorm.astype(np.float64) - cs.xn) <= (d + 4) * U * cs.xn).all(), "xnorm"
    gn = (cs.gcent.astype(np.float64) ** 2).sum(1)
    assert (np.abs(gnorm.astype(np.float64) - gn) <= (d + 2) * U * gn).all(), "gnorm"
    assert xnmax.view(np.uint32) == xnorm.max().view(np.uint32) and gnmax.view(np.uint32) == gnorm.max().view(np.uint32), "maxima"
    rng_ = f32(0)
    for c in range(g):
        seg = xnorm[cs.bounds[c]:cs.bounds[c + 1]]
        assert xnlo[c].view(np.uint32) == (seg.min() if len(seg) else f32(0)).view(np.uint32), ("xnlo", c)
        if len(seg):
            rng_ = max(rng_, f32(seg.max() - seg.min()))
    assert xn_step.view(np.uint32) == f32(rng_ / f32(255)).view(np.uint32), ("xn_step", float(xn_step), float(rng_))
    x = xnorm.astype(np.float64) - xnlo.astype(np.float64)[cs.group_of]
    code = xcode[:n].astype(np.float64)
    assert (code * float(xn_step) <= x).all(), "xnlo + xcode * xn_step above xnorm"
    assert (xcode[n:] == 0).all(), "xcode of padding rows"
    if xn_step > 0:
        fl = np.minimum(np.floor(x / float(xn_step)), 255)
        assert ((code == fl) | (code == fl - 1)).all(), "xcode needlessly low"
    else:
        assert (code == 0).all()


def check_tables(cs, out, q):
    """P of one query against float64"""
    P = out["P"][q].astype(np.float64)
    q64 = np.abs(cs.Q[q].astype(np.float64))
    for j in range(cs.m_pad):
        if j >= cs.m:
            assert (P[j] == 0).all(), (q, j, "padding table not 0")
            continue
        f, u_ = cs.fr[j], cs.un[j]
        cj = np.abs(cs.cents[cs.k * f:cs.k * u_].reshape(cs.k, u_ - f).astype(np.float64))
        tol = 2.0 * (u_ - f + 1) * U * (cj @ q64[f:u_])
        assert (np.abs(P[j, :cs.k] - cs.P[q, j]) <= tol).all() and (P[j, cs.k:] == 0).all(), (q, j, "P")


def check_tiles(cs, out):
    nn, nn_cnt, gcnt, tiles, meta = out["nn"], out["nn_cnt"], out["gcnt"], out["tiles"], out["meta"]
    want = {}
    for q in range(cs.b):
        cs_q = [int(c) for c in nn[q, :nn_cnt[q]]]
        assert len(set(cs_q)) == len(cs_q) and all(0 <= c < cs.g for c in cs_q), (q, "nn")
        for c in cs_q:
            if cs.sizes[c] > 0:
                want.setdefault(c, []).append(q)
    counts = np.array([len(want.get(c, ())) for c in range(cs.g)])
    assert np.array_equal(gcnt[:cs.g], counts), "gcnt"
    ntiles = int((-(-counts // GF_QT)).sum())
    assert meta[0] == ntiles and meta[1] == counts.sum() and len(tiles) == ntiles, ("meta", meta.tolist(), ntiles, int(counts.sum()))
    got, per_group, prev = {}, {}, -1
    for t in tiles:
        c, nq, r0, r1 = (int(v) for v in t[:4])
        assert prev <= c < cs.g and 1 <= nq <= GF_QT, ("tile", t.tolist())
        prev = c
        assert (r0, r1) == (cs.bounds[c], cs.bounds[c + 1]) and t[4] == out["xnlo"][c].view(np.int32) and (t[5:8] == 0).all(), ("tile", t.tolist())
        qid = t[8:24]
        assert (qid[nq:] == qid[nq - 1]).all(), ("padding slots", t.tolist())
        got.setdefault(c, []).extend(int(v) for v in qid[:nq])
        per_group.setdefault(c, []).append(nq)
    for c in range(cs.g):
        assert sorted(got.get(c, [])) == sorted(want.get(c, [])), ("pairs of group", c)
        nqs = per_group.get(c, [])
        assert len(nqs) == -(-counts[c] // GF_QT) and all(v == GF_QT for v in nqs[:-1]), ("tiles of group", c, nqs)


def check_threshold(cs, out, q):
    """qs of one query; returns whether it filters (1 / step != 0)"""
    bud, inv = float(out["qs"][q, 0]), float(out["qs"][q, 1])
    smp = sample_rows(cs, out["nn"], out["nn_cnt"], q)
    if len(smp) < LIST or q in cs.bad_q:
        assert inv == 0.0, (cs.name, q, "1 / step", inv, "with", len(smp), "sampled rows")
        return False
    assert inv > 0.0, (cs.name, q, "keeps every row with a sample of", len(smp))
    lo = out["P"][q, :cs.m, :cs.k].astype(np.float64).min(axis=1)
    s64 = np.sort(cs.D[q, smp])[LIST - 1]
    e = cs.E[q]
    slop = 4.0 * U * (abs(s64) + e + cs.m * np.abs(lo).sum())
    off = bud + lo.sum() - e - s64
    assert abs(off) <= e + slop, (cs.name, q, "threshold off the sample's 64th D by", off, "margin", e)
    nnq = out["nn"][q, :out["nn_cnt"][q]]
    base = (out["cdist"][q, nnq].astype(np.float64) - out["gnorm"][nnq]) + out["xnlo"][nnq]
    xg = np.sqrt(cs.qq[q]) + np.sqrt(float(out["scalars"][2]))
    rmax = (bud - (base.min() - 8.0 * (cs.d + 4) * 5.9604645e-8 * xg * xg)) * 1.001
    tol = 1e-4 + 8.0 * U * (abs(bud) + np.abs(base).max()) / abs(rmax)      # (a budget far below its two terms: their roundings)
    assert abs(inv * rmax / GF_LEVELS - 1.0) <= tol, (cs.name, q, "1 / step", inv, GF_LEVELS / rmax)
    return True


def check_budget(cs, out, q):
    """budget0 of a filtering query, replayed: tq = the 64th smallest float32 D~ of the sample (approx_row_sum from the
    replayed bases and the dev xnorm and P), budget0 = fl(fl(tq + margin) - sumlo) with gf_quant's sequential float32 sumlo; margin in
    float32: 1e-5 margin and 4 ulps of the budget's terms are allowed.  (The float64 check of check_threshold cannot tell a
    budget without its margin from one with it: E is ~100 times the real error of D~.)"""
    smp = sample_rows(cs, out["nn"], out["nn_cnt"], q)
    vals = cs.approx32(cs.base32[q, cs.group_of[smp]], out["xnorm"], out["P"], q, smp)
    tq = np.sort(vals)[LIST - 1]
    lo = out["P"][q, :cs.m, :cs.k].min(axis=1)
    sumlo = f32(0)
    for j in range(cs.m):
        sumlo = f32(sumlo + lo[j])
    margin = margin32(cs, q, out["scalars"][0])
    want = f32(f32(tq + margin) - sumlo)
    tol = 1e-5 * float(margin) + 4.0 * 2.0 ** -23 * (abs(float(tq)) + float(margin) + abs(float(want)))
    assert abs(float(out["qs"][q, 0]) - float(want)) <= tol, (cs.name, q, "budget0", float(out["qs"][q, 0]), "replayed", float(want), "margin", float(margin))


def margin32(cs, q, xnmax):
    """gf_quant's and gq_rerank's margin, in their float32"""
    with np.errstate(all="ignore"):
        xm = f32(np.sqrt(cs.qq32[q])) + f32(np.sqrt(f32(xnmax)))
        return f32(f32(f32(f32(4.0) * f32(cs.d + 2 * cs.m + 16)) * f32(5.9604645e-8)) * xm) * xm


def check_levels(cs, out, q):
    inv = float(out["qs"][q, 1])
    qb = out["qb"][q].astype(np.int64)
    P = out["P"][q].astype(np.float64)
    m, k = cs.m, cs.k
    assert (qb[:m, k:] == GF_SAT).all() and (qb[m:16] == 0).all(), (cs.name, q, "entries beyond k / padding tables")
    if inv == 0.0:
        assert (qb[:m, :k] == 0).all() and (qb[16] == 0).all(), (cs.name, q, "levels of a query that keeps everything")
        return
    x = np.concatenate([(P[:m, :k] - P[:m, :k].min(axis=1)[:, None]).reshape(-1), np.arange(256) * float(out["scalars"][1])])
    lv = np.concatenate([qb[:m, :k].reshape(-1), qb[16]])
    r = x * inv
    assert (lv <= r * (1.0 + 1e-12)).all(), (cs.name, q, "level too high", lv[lv > r][:4].tolist(), r[lv > r][:4].tolist())
    fl = np.minimum(np.floor(r), GF_SAT)
    exact = np.where(r >= GF_SAT, r >= GF_SAT * (1.0 + 2.0 ** -19), r - np.floor(r) >= r * 2.0 ** -19)
    bad = (lv > fl) | (lv < fl - 1) | (exact & (lv != fl))
    assert not bad.any(), (cs.name, q, "level off the float64 floor", lv[bad][:4].tolist(), r[bad][:4].tolist())


def check_queue(cs, out, q, filters):
    """the queued (row, base) pairs of one query: returns (rows, their D~ replayed in float32) or None after an overflow"""
    qcnt = int(out["qcnt"][q])
    ent = out["queue"][q, :min(qcnt, GF_CAP)]
    rows, base = ent[:, 0].astype(np.int64), ent[:, 1].copy().view(f32)
    searched = cs.searched(out["nn"], out["nn_cnt"], q)
    assert qcnt >= 0 and (np.diff(rows) > 0).all(), (cs.name, q, "a row queued twice (or rows not ascending)")
    assert len(np.setdiff1d(rows, searched)) == 0 and (len(rows) == 0 or (rows[0] >= 0 and rows[-1] < cs.n)), (cs.name, q, "a queued row outside the searched groups")
    grp = cs.group_of[rows]
    with np.errstate(all="ignore"):
        for c in np.unique(grp):
            bb = base[grp == c]
            assert (bb.view(np.uint32) == bb[:1].view(np.uint32)).all(), (cs.name, q, c, "bases of one pair differ")
            assert bb[0].view(np.uint32) == cs.base32[q, c].view(np.uint32), (cs.name, q, c, "base is not gq_approx_scan's", float(bb[0]), float(cs.base32[q, c]))
            if q not in cs.bad_q:
                want = cs.qq[q] - 2.0 * cs.qg[q, c]
                tol = (cs.d + 3) * U * (cs.qq[q] + 2.0 * cs.qg_abs[q, c])
                assert abs(float(bb[0]) - want) <= tol, (cs.name, q, c, "base", float(bb[0]), want)
    if qcnt > GF_CAP:
        return None
    if not filters:
        assert np.array_equal(rows, searched), (cs.name, q, "a query that keeps everything queued", len(rows), "of", len(searched))
    else:
        Dq = cs.D[q, searched]
        t64 = np.sort(Dq)[LIST - 1] if len(searched) >= LIST else np.inf
        must = searched[Dq <= t64 - 2.0 * cs.E[q]]
        missing = np.setdiff1d(must, rows)
        assert len(missing) == 0, (cs.name, q, "dropped rows with D <= T64 - 2E", missing[:4].tolist(), cs.D[q, missing[:4]].tolist(), t64, cs.E[q])
        far = rows[cs.D[q, rows] > upper_bound(cs, out, q)]
        assert len(far) == 0, (cs.name, q, "queued rows beyond the bound", len(far), len(rows))
    return rows, cs.approx32(base, out["xnorm"], out["P"], q, rows)


def check_list(cs, out, q, lv, li, flagged):
    """one path's list of one query against float64; returns the largest |lv - D| / E"""
    searched = cs.searched(out["nn"], out["nn_cnt"], q)
    have = min(LIST, len(searched))
    assert (li[have:] == INT_MAX).all() and np.isposinf(lv[have:]).all(), (cs.name, q, "padding")
    if flagged:
        return 0.0
    rows = li[:have].astype(np.int64)
    assert (rows != INT_MAX).all() and len(np.setdiff1d(rows, searched)) == 0 and len(set(rows.tolist())) == have, (cs.name, q, "listed rows")
    key = ordered_key(lv[:have])
    assert ((np.diff(key) > 0) | ((np.diff(key) == 0) & (np.diff(rows) > 0))).all(), (cs.name, q, "list not ascending by (value, row)")
    if q in cs.bad_q:
        return 0.0
    Dq, e = cs.D[q, searched], cs.E[q]
    L = np.sort(Dq)[LIST - 1] if len(searched) >= LIST else np.inf
    missing = np.setdiff1d(searched[Dq < L - 2.0 * e], rows)
    assert len(missing) == 0, (cs.name, q, "rows with D < L - 2E not listed", missing[:4].tolist())
    assert (cs.D[q, rows] <= L + 2.0 * e).all(), (cs.name, q, "a listed row beyond L + 2E")
    err = np.abs(lv[:have].astype(np.float64) - cs.D[q, rows])
    assert (err <= e).all(), (cs.name, q, "|D~ - D| above the margin", float(err.max()), e)
    return float(err.max() / e) if have else 0.0


def expected_redo(cs, q, lv, li, flagged):
    """gq_rerank's decision from one list: (redo or None where the certificate is on its edge, sorted (dist, row) of the list)"""
    rows = li.astype(np.int64)
    have = rows != INT_MAX
    Dv = np.full(LIST, np.inf, f32)
    Dv[have] = cs.exact32(q, rows[have])
    nan_d = bool(np.isnan(Dv[have]).any())
    fin = have & ~np.isnan(Dv)
    sv = np.where(fin, Dv, f32(np.inf))
    si = np.where(fin, rows, INT_MAX)
    order = np.lexsort((si, ordered_key(sv)))
    sv, si = sv[order], si[order]
    nfin, kk = int(fin.sum()), cs.kk
    tie = any(si[i] != INT_MAX and si[i + 1] != INT_MAX and sv[i] == sv[i + 1] for i in range(min(kk, LIST - 1)))
    redo, edge = bool(flagged) or nan_d or tie, False
    if have.sum() == LIST:
        with np.errstate(all="ignore"):
            margin = margin32(cs, q, cs.xnmax32)
            ek, a_last = sv[min(kk, LIST - 1)], lv[LIST - 1]
            bound = f32(a_last - margin)
            certified = nfin > kk and bool(ek < bound) and not np.isnan(margin) and not np.isnan(a_last)
            edge = bool(np.isfinite(bound) and np.isfinite(ek) and abs(float(ek) - float(bound)) <= 2.0 ** -21 * (abs(float(a_last)) + float(margin)))
        redo = redo or not certified
    return (None if edge and not (bool(flagged) or nan_d or tie) else redo), sv, si


def check_stage(cs, out, oracle):
    """Everything the docstring lists, on the hook's (or the model's) outputs.  Returns per query
    (queued, must keep, upper set) and the figures DESIGN.md 9p records: the largest |lv - D| / E and the certified queries."""
    cs.xnmax32 = out["scalars"][0]
    check_index_state(cs, out)
    check_tiles(cs, out)
    ei, ed, ec = cs.oracle_answer(oracle)
    stats, worst, edges = [], 0.0, 0
    redo = [set(out["redo%d" % p][:int(out["nredo%d" % p][0])].tolist()) for p in range(2)]
    for p in range(2):
        assert len(redo[p]) == out["nredo%d" % p][0] and all(0 <= v < cs.b for v in redo[p]), (cs.name, "redo list", p)
    for q in range(cs.b):
        if q not in cs.bad_q:
            check_tables(cs, out, q)
        filters = check_threshold(cs, out, q)
        check_levels(cs, out, q)
        queued = check_queue(cs, out, q, filters)
        qcnt = int(out["qcnt"][q])
        stats.append((qcnt,) + (figures(cs, out, q)[1:] if filters else (qcnt, qcnt)))
        searched = cs.searched(out["nn"], out["nn_cnt"], q)
        # flags and lists, by group: from the queue's own rows and values
        flag_f = bool(out["anan0"][q].any())
        assert not out["anan0"][q, 1:].any()
        if queued is None:
            assert flag_f, (cs.name, q, "queue overflowed without a flag")
        else:
            rows, vals = queued
            if filters:
                check_budget(cs, out, q)
            nan = bool(np.isnan(vals).any())
            lv_w, li_w = smallest64(vals, rows)
            want = min(LIST, len(rows))
            at_cut = int((ordered_key(np.where(np.isnan(vals), f32(np.inf), vals)) <= ordered_key(lv_w[want - 1])).sum()) if want else 0
            assert flag_f == (nan or at_cut > GF_PLACED), (cs.name, q, "flag", flag_f, "NaN", nan, "at or below the cut", at_cut)
            if not flag_f:
                assert np.array_equal(out["ami0"][q], li_w) and np.array_equal(out["amv0"][q].view(np.uint32), lv_w.view(np.uint32)), \
                    (cs.name, q, "by-group list is not the 64 smallest (D~, row) of its queue")
        # the scan path: every searched row, the bases being the queue's where the pair has one
        flag_s = bool(out["anan1"][q].any())
        if q not in cs.bad_q:
            assert not flag_s, (cs.name, q, "gq_approx_scan flagged a finite query")
        elif queued is not None:           # (a non-finite query keeps everything: the queue holds every pair's base)
            assert flag_s == bool(np.isnan(queued[1]).any()), (cs.name, q, "gq_approx_scan's flag")
        if not flag_s and q not in cs.bad_q:
            lv_w, li_w = smallest64(cs.approx32(cs.base32[q, cs.group_of[searched]], out["xnorm"], out["P"], q, searched), searched)
            assert np.array_equal(out["ami1"][q], li_w) and np.array_equal(out["amv1"][q].view(np.uint32), lv_w.view(np.uint32)), \
                (cs.name, q, "gq_approx_scan's list is not the 64 smallest (D~, row) of the searched rows")
        worst = max(worst, check_list(cs, out, q, out["amv0"][q], out["ami0"][q], flag_f),
                    check_list(cs, out, q, out["amv1"][q], out["ami1"][q], flag_s))
        if not flag_f and not flag_s:
            assert np.array_equal(out["ami0"][q], out["ami1"][q]) and np.array_equal(out["amv0"][q].view(np.uint32), out["amv1"][q].view(np.uint32)), \
                (cs.name, q, "the two paths list different candidates")
        for p, flagged in ((0, flag_f), (1, flag_s)):
            want_redo, sv, si = expected_redo(cs, q, out["amv%d" % p][q], out["ami%d" % p][q], flagged)
            if want_redo is None:
                edges += 1
            else:
                assert (q in redo[p]) == want_redo, (cs.name, q, "path", p, "redone" if q in redo[p] else "certified", "expected", want_redo)
            if q not in redo[p]:
                live = min(cs.kk, int((si != INT_MAX).sum()))
                oi, od, oc = out["oi%d" % p][q], out["od%d" % p][q], out["oc%d" % p][q]
                assert oc == live == ec[q] and np.array_equal(oi[:live], si[:live]) and np.array_equal(oi[:live], ei[q, :live]), (cs.name, q, p, "rows")
                assert np.array_equal(od[:live].view(np.uint32), sv[:live].view(np.uint32)) and \
                    np.array_equal(od[:live].view(np.uint32), ed[q, :live].view(np.uint32)), (cs.name, q, p, "distances")
                assert (oi[live:] == -1).all() and np.isposinf(od[live:]).all()
    assert edges * 10 <= 2 * cs.b, (cs.name, "certificates on their edge", edges)
    certified = [cs.b - len(r) for r in redo]
    return stats, worst, certified, edges


# ---- a numpy model of the stage: what the checks say about a faithful pre-selection and about broken ones ---------------
def stage_model(cs, lim_plus=2, with_margin=True, pad_limit=0):
    """The hook's outputs from a float32 model of the kernels (reductions whose order the kernels leave open -- wave sums --
    are float64 sums rounded once).  lim_plus = 1 / with_margin = False / pad_limit > 0: the three mutations."""
    n, b, g, d, m, k, mp = cs.n, cs.b, cs.g, cs.d, cs.m, cs.k, cs.m_pad
    out = {}
    with np.errstate(all="ignore"):
        gc64, q64 = cs.gcent.astype(np.float64), cs.Q.astype(np.float64)
        cd = ((q64[:, None, :] - gc64[None, :, :]) ** 2).sum(2)
        cdist = cd.astype(f32)
        stride = max(1, min(cs.limit + (int((cs.sizes == 0).sum()) if cs.strategy == 1 else 0), g))
        nn = np.zeros((b, stride), np.int32)
        nn_cnt = np.zeros(b, np.int32)
        for q in range(b):
            order = np.lexsort((np.arange(g), np.where(np.isnan(cdist[q]), np.inf, cdist[q])))
            cnt = min(cs.limit, g)
            if cs.strategy == 1:
                rows_seen = np.cumsum(cs.sizes[order])
                cnt = min(int(np.searchsorted(rows_seen, cs.limit, side="left")) + 1, g)
            nn[q, :cnt], nn_cnt[q] = order[:cnt], cnt
        xnorm = cs.xn.astype(f32)
        gnorm = (gc64 ** 2).sum(1).astype(f32)
        xnlo = np.array([xnorm[cs.bounds[c]:cs.bounds[c + 1]].min() if cs.sizes[c] else 0 for c in range(g)], f32)
        rng_ = max(f32(xnorm[cs.bounds[c]:cs.bounds[c + 1]].max() - xnlo[c]) for c in range(g) if cs.sizes[c])
        xn_step = f32(rng_ / f32(255))
        inv_x = f32(f32(f32(255) / rng_) * GF_SHRINK) if rng_ > 0 and xn_step > 0 else f32(0)
        npad = -(-n // 64) * 64
        xcode = np.zeros(npad, np.uint8)
        xcode[:n] = np.clip(((xnorm - xnlo[cs.group_of]).astype(f32) * inv_x).astype(f32).astype(np.int64), 0, 255)
        P = np.zeros((b, mp, 256), f32)
        P[:, :m, :k] = cs.P.astype(f32)
        xnmax, gnmax = xnorm.max(), gnorm.max()
        base_all = cs.base32                                         # [b][g]
        qs = np.zeros((b, 4), f32)
        qb = np.zeros((b, GF_NT, 256), np.uint8)
        queue = np.zeros((b, GF_CAP, 2), np.uint32)
        qcnt = np.zeros(b, np.int32)
        lists = {p: (np.full((b, LIST), np.inf, f32), np.full((b, LIST), INT_MAX, np.int32), np.zeros((b, 16), np.int32)) for p in range(2)}
        pairs = {}
        for q in range(b):
            nnq = nn[q, :nn_cnt[q]]
            for c in nnq:
                if cs.sizes[c]:
                    pairs.setdefault(int(c), []).append(q)
            smp = sample_rows(cs, nn, nn_cnt, q)
            tq = f32(np.inf)
            bad = not np.isfinite(P[q, :m, :k]).all()
            if len(smp):
                vals = cs.approx32(base_all[q, cs.group_of[smp]], xnorm, P, q, smp)
                bad = bad or bool(np.isnan(vals).any())
                if len(smp) >= LIST:
                    tq = np.sort(np.where(np.isnan(vals), f32(np.inf), vals))[LIST - 1]
            lo = P[q, :m, :k].min(axis=1)
            sumlo = f32(0)
            for j in range(m):
                sumlo = f32(sumlo + lo[j])
            qq = cs.qq32[q]
            mbs = ((cdist[q, nnq] - gnorm[nnq]).astype(f32) + xnlo[nnq]).astype(f32)
            bad = bad or not np.isfinite(mbs).all()
            xg = f32(np.sqrt(qq)) + f32(np.sqrt(gnmax))
            minbase = f32(mbs.min() - f32(f32(f32(8.0) * f32(d + 4)) * f32(5.9604645e-8)) * xg * xg)
            margin = margin32(cs, q, xnmax)
            budget0 = f32(f32(tq + (margin if with_margin else f32(0))) - sumlo)
            rmax = f32(f32(budget0 - minbase) * f32(1.001))
            inv = f32(f32(GF_LEVELS) / max(rmax, f32(1e-30)))
            if bad or not all(np.isfinite(v) for v in (tq, margin, budget0, rmax, inv)):
                inv = f32(0)
            qs[q, 0], qs[q, 1] = budget0, inv
            invs = f32(inv * GF_SHRINK)
            xs = (P[q, :m, :k] - lo[:, None]).astype(f32)
            qb[q, :m, :k] = np.clip(np.nan_to_num((xs * invs).astype(f32), nan=0.0, posinf=255, neginf=0), 0, 255).astype(np.int64)
            qb[q, :m, k:] = GF_SAT
            qb[q, 16] = np.clip(((np.arange(256, dtype=f32) * xn_step).astype(f32) * invs).astype(f32), 0, 255).astype(np.int64)
            # gf_filter: per pair the limit, per row the 17 levels
            rows = cs.searched(nn, nn_cnt, q)
            grp = cs.group_of[rows]
            total = qb[q, 16][xcode[rows]].astype(np.int64)
            for j in range(m):
                total += qb[q, j][cs.idx[j, rows]]
            if inv == 0:
                lim = np.full(g, GF_SAT, np.int64)
            else:
                f = np.floor(((budget0 - (base_all[q] + xnlo).astype(f32)).astype(f32) * inv).astype(f32))
                lim = np.where(f >= GF_SAT - 1, GF_SAT, np.where(f >= -1, np.nan_to_num(f, nan=-9) + lim_plus, 0)).astype(np.int64)
            kept = rows[total < lim[grp]]
            entries = [(int(r), base_all[q, cs.group_of[r]]) for r in kept]
            qcnt[q] = len(entries)
            entries = entries[:GF_CAP]
            queue[q, :len(entries), 0] = [e[0] for e in entries]
            queue[q, :len(entries), 1] = np.array([e[1] for e in entries], f32).view(np.uint32)
            out.setdefault("_kept", {})[q] = kept
        # padding slots repeat a tile's last query: with a limit of their own they queue its rows again
        if pad_limit:
            for c, qsl in pairs.items():
                extra = (-len(qsl)) % GF_QT
                q = qsl[-1]
                if extra:
                    grp_rows = np.intersect1d(out["_kept"][q], np.arange(cs.bounds[c], cs.bounds[c + 1]))
                    room = GF_CAP - qcnt[q]
                    add = np.repeat(grp_rows, extra)[:max(room, 0)]
                    queue[q, qcnt[q]:qcnt[q] + len(add), 0] = add
                    queue[q, qcnt[q]:qcnt[q] + len(add), 1] = np.full(len(add), base_all[q, c], f32).view(np.uint32)
                    qcnt[q] += len(grp_rows) * extra
        for q in range(b):
            cnt = min(int(qcnt[q]), GF_CAP)
            order = np.lexsort((queue[q, :cnt, 1], queue[q, :cnt, 0]))
            queue[q, :cnt] = queue[q, :cnt][order]
            rows_q = queue[q, :cnt, 0].astype(np.int64)
            vals = cs.approx32(queue[q, :cnt, 1].copy().view(f32), xnorm, P, q, rows_q)
            lv, li = smallest64(vals, rows_q)
            want = min(LIST, cnt)
            at_cut = int((ordered_key(np.where(np.isnan(vals), f32(np.inf), vals)) <= ordered_key(lv[want - 1])).sum()) if want else 0
            flag = bool(np.isnan(vals).any()) or qcnt[q] > GF_CAP or at_cut > GF_PLACED
            if at_cut > GF_PLACED:
                lv[:], li[:] = np.inf, INT_MAX
            lists[0][0][q], lists[0][1][q], lists[0][2][q, 0] = lv, li, int(flag)
            rows = cs.searched(nn, nn_cnt, q)
            vals = cs.approx32(base_all[q, cs.group_of[rows]], xnorm, P, q, rows)
            lists[1][0][q], lists[1][1][q] = smallest64(vals, rows)
            lists[1][2][q, 0] = int(np.isnan(vals).any())
        tiles = []
        for c in sorted(pairs):
            for first in range(0, len(pairs[c]), GF_QT):
                qid = pairs[c][first:first + GF_QT]
                tiles.append([c, len(qid), cs.bounds[c], cs.bounds[c + 1], int(xnlo[c].view(np.int32)), 0, 0, 0] + qid + [qid[-1]] * (GF_QT - len(qid)))
        gcnt = np.array([len(pairs.get(c, ())) for c in range(g)], np.int32)
        out.pop("_kept")
        out.update(nn=nn, nn_cnt=nn_cnt, cdist=cdist, xnorm=xnorm, xnlo=xnlo, xcode=xcode, gnorm=gnorm,
                   scalars=np.array([xnmax, xn_step, gnmax], f32), P=P, qs=qs, qb=qb, gcnt=gcnt,
                   tiles=np.array(tiles, np.int64).astype(np.int32).reshape(-1, 24), meta=np.array([len(tiles), gcnt.sum(), 0, 0], np.int32),
                   qcnt=qcnt, queue=queue)
        cs.xnmax32 = xnmax
        for p in range(2):
            lv, li, an = lists[p]
            out["amv%d" % p], out["ami%d" % p], out["anan%d" % p] = lv, li, an
            oi = np.full((b, cs.kk), -1, np.int32)
            od = np.full((b, cs.kk), np.inf, f32)
            oc = np.zeros(b, np.int32)
            redo = []
            for q in range(b):
                want_redo, sv, si = expected_redo(cs, q, lv[q], li[q], an[q].any())
                live = min(cs.kk, int((si != INT_MAX).sum()))
                oi[q, :live], od[q, :live], oc[q] = si[:live], sv[:live], live
                if want_redo is None or want_redo:
                    redo.append(q)
            out["oi%d" % p], out["od%d" % p], out["oc%d" % p] = oi, od, oc
            out["nredo%d" % p] = np.array([len(redo)], np.int32)
            out["redo%d" % p] = np.array(redo + [-1] * (b - len(redo)), np.int32)
    return out
