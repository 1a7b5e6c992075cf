"""Host-side reference for the matrix-core filter in front of KMeans.assign (gulon_amd/csrc/kmeans_mfma.hip): numpy only.

The filter replays the reference's scan over the centroids (KMeans.scala:24-55) on approximate distances and must hand
every row whose scan is decided by less than its error band to the exact kernels.  Nothing here is taken from the
kernels' output: the inputs that sit inside the band (`near_tie_rows`), the scan and its smallest margin in float64
(`scan64`), the band as the file header documents it (`band`) and the kernel form the LDS rule of the header gives each
shape (`EXPECTED_FORM`) are all restated by hand.
"""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)

# kinds of gulon_selftest_assign_filter's form_out
NO_FILTER, RESIDENT, STREAM, BF16_COMPACT, BF16_PIECES = 0, 1, 2, 3, 4

# (s, k) -> (kind, width), by hand from the header comments of kmeans_mfma.hip.  nkb = ceil(k / 32) centroid blocks.
#   bf16 split: s <= 16 and nkb * (na * 1024 + 256) bytes <= 60 KiB, na operand words per lane and block:
#       s <= 8: na = 3 compact words, 3328 B per block, nkb <= 18, k <= 576
#       s <= 10: 4 words, 4352 B, nkb <= 14, k <= 448          s <= 13: 5 words, 5376 B, nkb <= 11, k <= 352
#       s = 14..16: three pieces (six products), 3328 B, k <= 576
#   else resident fp32, T = ceil(s / 2) <= 8 K-steps: nkb * (T + 1) * 256 bytes <= 60 KiB, nkb * (T + 1) <= 240
#   else streaming fp32 with T rounded up to 16 / 32 / 64 (s <= 32 / 64 / 128); s > 128: no filter
EXPECTED_FORM = {
    (1, 3): (BF16_COMPACT, 3), (2, 5): (BF16_COMPACT, 3), (4, 16): (BF16_COMPACT, 3),
    (8, 32): (BF16_COMPACT, 3), (8, 33): (BF16_COMPACT, 3), (8, 64): (BF16_COMPACT, 3), (8, 65): (BF16_COMPACT, 3),
    (8, 576): (BF16_COMPACT, 3),                       # nkb = 18: 59 904 B, the last k that fits
    (9, 448): (BF16_COMPACT, 4),                       # nkb = 14: 60 928 B
    (10, 40): (BF16_COMPACT, 4),
    (11, 352): (BF16_COMPACT, 5),                      # nkb = 11: 59 136 B
    (13, 100): (BF16_COMPACT, 5),
    (14, 576): (BF16_PIECES, 3), (16, 33): (BF16_PIECES, 3),
    (1, 577): (RESIDENT, 1),                           # nkb = 19 > 18: past the bf16 split
    (2, 577): (RESIDENT, 1),
    (2, 3840): (RESIDENT, 1),                          # nkb = 120, 120 * 2 = 240: LDS exactly full
    (3, 640): (RESIDENT, 2),                           # nkb = 20 (even)
    (5, 1100): (RESIDENT, 3),                          # nkb = 35, 140
    (8, 1536): (RESIDENT, 4),                          # nkb = 48, 240: full again
    (9, 449): (RESIDENT, 5),                           # nkb = 15 > 14
    (11, 353): (RESIDENT, 6),                          # nkb = 12 > 11
    (14, 577): (RESIDENT, 7),                          # nkb = 19 (odd)
    (16, 832): (RESIDENT, 8),                          # nkb = 26, 234: the last k that stays resident
    (16, 833): (STREAM, 16),                           # nkb = 27, 243 > 240: the first that streams
    (8, 3000): (STREAM, 16),                           # nkb = 94, 470
    (32, 33): (STREAM, 16),
    (33, 7): (STREAM, 32), (64, 33): (STREAM, 32),
    (65, 40): (STREAM, 64), (128, 300): (STREAM, 64),
    (130, 5): (NO_FILTER, 0),
}


def clustered(seed, n, d, kc=8):
    """Ordinary rows: a mixture of kc anisotropic Gaussians (the data of tests/test_gpu_kmeans.py)."""
    rng = np.random.default_rng(seed)
    cents = rng.uniform(-5, 5, (kc, d))
    scales = rng.uniform(0.1, 1.5, (kc, d))
    which = rng.integers(0, kc, n)
    return (cents[which] + rng.standard_normal((n, d)) * scales[which]).astype(np.float32)


def offsets32(C):
    """KMeans.apply's offsets (KMeans.scala:170-186): |c|^2 as a sequential unfused binary32 sum."""
    C = np.ascontiguousarray(C, np.float32)
    o = np.zeros(C.shape[0], np.float32)
    with np.errstate(all="ignore"):
        for e in range(C.shape[1]):
            o = o + C[:, e] * C[:, e]
    return o


def near_tie_rows(seed, n, d, frm, s, C):
    """n rows of d columns whose slice [frm, frm + s) sits next to the bisector of its two nearest centroids: start
    from ordinary rows, find the two nearest centroids a, b in float64, move the slice along w = C[b] - C[a] onto their
    bisector and push it off again by +- 2^u * S / (2 |w|^2) * w, u uniform in [-30, -20], S = max|c|^2 + 2 |x| max|c|.
    d_b - d_a is then -+ 2^u * S before the slice is rounded to binary32: log-uniform from far below to far above the
    rounding error of any evaluation order, so some rows sit at whatever gap a kernel form gets wrong."""
    rng = np.random.default_rng([seed, 77])
    X = clustered(int(rng.integers(1 << 30)), n, d).astype(np.float64)
    Cd = np.asarray(C, np.float64)
    c2 = (Cd * Cd).sum(axis=1)
    cmax = np.sqrt(c2.max())
    for lo in range(0, n, 4096):
        xs = X[lo:lo + 4096, frm:frm + s]
        dist = c2[None, :] - 2.0 * (xs @ Cd.T)
        if Cd.shape[0] >= 2:
            two = np.argpartition(dist, 1, axis=1)[:, :2]
        else:
            two = np.zeros((xs.shape[0], 2), np.int64)
        r = np.arange(xs.shape[0])
        swap = dist[r, two[:, 0]] > dist[r, two[:, 1]]
        a = np.where(swap, two[:, 1], two[:, 0])
        b = np.where(swap, two[:, 0], two[:, 1])
        w = Cd[b] - Cd[a]
        w2 = (w * w).sum(axis=1)
        ok = w2 > 0
        w2 = np.where(ok, w2, 1.0)
        mid = 0.5 * (Cd[a] + Cd[b])
        t = ((mid - xs) * w).sum(axis=1) / w2                  # onto the bisector
        xb = xs + t[:, None] * w
        S = c2.max() + 2.0 * np.sqrt((xb * xb).sum(axis=1)) * cmax
        u = rng.uniform(-30.0, -20.0, xs.shape[0])
        sign = rng.choice([-1.0, 1.0], xs.shape[0])
        delta = sign * np.exp2(u) * S / (2.0 * w2)
        X[lo:lo + 4096, frm:frm + s] = np.where(ok[:, None], xb + delta[:, None] * w, xs)
    return X.astype(np.float32)


def scan64(X, frm, s, C, rows=None, chunk=None):
    """The reference's scan over c = 0..k-1 of d_c = offsets[c] - 2 x.c, evaluated in float64 (offsets as the reference
    holds them: binary32).  Per row: the argmin (first index) and the smallest |d_c - running minimum before c|, the
    running minimum starting at Float.MaxValue.  A distance that is NaN or +Inf never enters the reference's minimum
    (both of its comparisons are false) and is skipped here.  rows: a subset (default all); evaluated in row chunks."""
    X = np.asarray(X)
    Cd = np.asarray(C, np.float64)
    k = Cd.shape[0]
    off = offsets32(C).astype(np.float64)
    rows = np.arange(X.shape[0]) if rows is None else np.asarray(rows, np.int64)
    if chunk is None:
        chunk = max(64, (1 << 22) // max(k, 1))
    arg = np.zeros(rows.size, np.int64)
    gap = np.zeros(rows.size, np.float64)
    with np.errstate(all="ignore"):
        for lo in range(0, rows.size, chunk):
            xs = X[rows[lo:lo + chunk], frm:frm + s].astype(np.float64)
            dist = off[None, :] - 2.0 * (xs @ Cd.T)
            dist = np.where(np.isnan(dist), np.inf, dist)
            run = np.minimum.accumulate(np.concatenate([np.full((xs.shape[0], 1), FLT_MAX), dist], axis=1), axis=1)
            g = np.abs(dist - run[:, :-1])
            gap[lo:lo + chunk] = np.where(np.isnan(g), np.inf, g).min(axis=1)
            arg[lo:lo + chunk] = dist.argmin(axis=1)
    return arg, gap


def errk(s, kind):
    """The band's factor as the header of kmeans_mfma.hip documents it: 2.1 * (E / S) + the key perturbation, with
    fp32 forms: E / S = (2 s + 4) 2^-24 (the reference's unfused chain against the fma chain, margins included) and the
              centroid's position in 5 mantissa bits: 2.1 * 31 ulp
    bf16 forms: E / S = (s + 1) 2^-24 + 6 (s + 2) 2^-24 + 2^-22.9 (reference chain, six accumulations, dropped pieces)
              and 4 index bits: 2.1 * 15 ulp"""
    if kind in (RESIDENT, STREAM):
        return 2.1 * (2 * s + 4) * 2.0 ** -24 + 2.1 * 31 * 2.0 ** -23
    if kind in (BF16_COMPACT, BF16_PIECES):
        return 2.1 * ((7 * s + 13) * 2.0 ** -24 + 2.0 ** -22.9) + 2.1 * 15 * 2.0 ** -23
    raise ValueError(kind)


def band(X, frm, s, C, kind, rows=None):
    """The documented band of a row, errk * (cmax2 + 2 sqrt(|x|^2 cmax2)) in float64; cmax2 = the largest offset
    (+ 1e-30, the kernels' absolute floor: it decides only where the products underflow).  Inf where an offset is not
    finite or a binary32 evaluation of |x|^2 or of |x|^2 cmax2 overflows, NaN for a slice that holds one: such rows are
    not finite rows, and the filter must flag them."""
    X = np.asarray(X)
    rows = np.arange(X.shape[0]) if rows is None else np.asarray(rows, np.int64)
    off = offsets32(C).astype(np.float64)
    cmax2 = float(off.max()) if np.isfinite(off).all() else np.inf
    with np.errstate(all="ignore"):
        xs = X[rows, frm:frm + s].astype(np.float64)
        nx = (xs * xs).sum(axis=1)
        b = errk(s, kind) * (cmax2 + 2.0 * np.sqrt(nx * cmax2)) + 1e-30
        over = (nx > FLT_MAX) | (nx * cmax2 > FLT_MAX)
        return np.where(np.isnan(nx), np.nan, np.where(over, np.inf, b))


def mixed_data(seed, n, d, frm, s, k, head=0, outliers=0.0):
    """The test data of a case: (X [n, d] float32, centroids [k, s] float32, near [n] bool).  Centroids are drawn from
    ordinary rows; the first `head` rows are ordinary, of the rest a random half are near-tie rows (near[r] True).
    outliers: that fraction of the ordinary rows is scaled by 20, out of the centroids' hull (for shapes whose centroids
    stand closer than the band is wide, where every row between them is a genuine near-tie)."""
    rng = np.random.default_rng([seed, 11])
    pool = clustered(seed, max(n, k), d)
    C = np.ascontiguousarray(pool[rng.choice(pool.shape[0], k, replace=False), frm:frm + s])
    X = pool[:n].copy()
    near = np.zeros(n, bool)
    tail = np.arange(head, n)
    near[rng.permutation(tail)[:tail.size // 2]] = True
    idx = np.flatnonzero(near)
    X[idx] = near_tie_rows(seed, idx.size, d, frm, s, C)
    if outliers:
        far = ~near & (rng.random(n) < outliers)
        X[far] *= np.float32(20.0)
    return X, C, near
