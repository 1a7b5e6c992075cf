"""Learning the map `translate` expects: an orthogonal W that takes the source language's vectors into the target's space
(csrc/alignment.hip).  Not in the reference.

The recipe is the supervised one of MUSE (Conneau et al., "Word translation without parallel data", 2018):

  seed      W_0 = procrustes(sum over the seed dictionary's pairs (s, t) of x_s^T y_t)      -- seed_alignment
  refine    for t = 0 .. rounds: translate the most frequent source words with X W_t by CSLS and the most frequent target
            words back (induce_matches), keep the pairs that chose each other, W_{t+1} = procrustes of THEIR moment --
            always against the original X: maps are not chained                              -- train_alignment
  choose    the W_t with the highest criterion: the mean cosine between the first 10 000 source words and their CSLS
            best target, MUSE's unsupervised validation measure

Everything that touches a vector runs on the device: the map is applied by Rotation.apply_device, the mean similarities
are csls_offsets, the best matches the exact offset scan at k = 1, the mutual test gulon_mutual_rows_dev, the moments
gulon_dataset_pair_moment(_dev) -- rotate.hip's deterministic binary64 moment reading its rows through two lists, a
negative row meaning "no pair".  The host sees d x d moments, counts and the SVDs.

Where this departs from MUSE: everything -- the CSLS mean similarities r included -- is restricted to the first max_rank
rows of each side.  MUSE takes r over the whole vocabulary and filters the induced pairs by rank afterwards.  Centring
(`renorm,center,renorm`) and the unsupervised adversarial start are outside this module.

Both word vector files are taken in FILE order (row = frequency rank), normalised on reading.

pair_moment_reference and mutual_rows_reference restate the two kernels in numpy, chunk order included."""
import ctypes as C

import numpy as np

from . import native as N
from .rotation import Rotation, procrustes

MOMENT_ROWS = 4096            # pairs per chunk of the pair moment (csrc/rotate.hip): fixes the order of its additions
ROWS_PER_PASS = 4096          # rows per batch of induce_matches' best-match queries
CRITERION_ROWS = 10000        # the source rows behind the criterion (MUSE's dico_max_rank of its validation measure)


# ---- references (numpy) ----------------------------------------------------------------------------------------------------

def pair_moment_reference(a, b, rows_a, rows_b):
    """gulon_dataset_pair_moment in numpy: a [na][da], b [nb][db] float32; out[p][q] = sum_i a[rows_a[i]][p] *
    b[rows_b[i]][q] in float64, the list cut by POSITION into chunks of MOMENT_ROWS, each chunk summed i ascending from
    0.0, the chunk sums added in ascending chunk order from 0.0.  A pair with a negative row on either side adds nothing.
    -> (float64 [da][db], the number of pairs used).  ValueError: lists of different length, a row beyond its matrix."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ra, rb = np.asarray(rows_a, np.int64).reshape(-1), np.asarray(rows_b, np.int64).reshape(-1)
    if a.ndim != 2 or b.ndim != 2:
        raise ValueError("requirement failed: a and b are matrices")
    if len(ra) != len(rb):
        raise ValueError(f"requirement failed: {len(ra)} rows of a for {len(rb)} rows of b")
    if (ra >= a.shape[0]).any() or (rb >= b.shape[0]).any():
        raise ValueError("requirement failed: a pair holds a row beyond its matrix")
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    out = np.zeros((a.shape[1], b.shape[1]), np.float64)
    product = np.zeros_like(out)
    used = 0
    with np.errstate(all="ignore"):
        for c0 in range(0, len(ra), MOMENT_ROWS):
            s = np.zeros_like(out)
            for i in range(c0, min(c0 + MOMENT_ROWS, len(ra))):
                if ra[i] < 0 or rb[i] < 0:
                    continue
                used += 1
                np.multiply.outer(a64[ra[i]], b64[rb[i]], out=product)         # exact: binary32 times binary32
                s += product
            out = out + s
    return out, used


def mutual_rows_reference(fwd, bwd):
    """gulon_mutual_rows in numpy: out[s] = fwd[s] if 0 <= fwd[s] < len(bwd) and bwd[fwd[s]] == s, else -1.  -> int32."""
    fwd, bwd = np.asarray(fwd, np.int64).reshape(-1), np.asarray(bwd, np.int64).reshape(-1)
    out = np.full(len(fwd), -1, np.int32)
    for s, t in enumerate(fwd.tolist()):
        if 0 <= t < len(bwd) and bwd[t] == s:
            out[s] = t
    return out


# ---- the two kernels ---------------------------------------------------------------------------------------------------------

def _moment_call(fn, a, b, ptr_a, ptr_b, n):
    out = np.zeros((a.cols, b.cols), np.float64)
    used = C.c_int64(0)
    N.check(fn(a._h, b._h, ptr_a, ptr_b, n, out.reshape(-1), C.byref(used)))
    return out, used.value


def pair_moment(a, b, rows_a, rows_b):
    """gulon_dataset_pair_moment: out[p][q] = sum_i a[rows_a[i]][p] * b[rows_b[i]][q] in binary64 for two DeviceMatrix
    and two lists of rows of equal length; a pair with a negative row on either side is skipped (pair_moment_reference).
    -> (float64 [a.cols][b.cols], the pairs used); the same bits on every call.  ValueError: lists of different length,
    a row beyond its matrix."""
    ra, rb = N.i32(rows_a).reshape(-1), N.i32(rows_b).reshape(-1)
    if len(ra) != len(rb):
        raise ValueError(f"requirement failed: {len(ra)} rows of a for {len(rb)} rows of b")
    n = len(ra)
    return _moment_call(N.lib().gulon_dataset_pair_moment, a, b, ra.ctypes.data if n else None,
                        rb.ctypes.data if n else None, n)


def pair_moment_dev(a, b, d_rows_a, d_rows_b, n):
    """gulon_dataset_pair_moment_dev: pair_moment with the two lists device addresses, trusted as they are; on the null
    stream.  -> (float64 [a.cols][b.cols], the pairs used)."""
    return _moment_call(N.lib().gulon_dataset_pair_moment_dev, a, b, d_rows_a, d_rows_b, int(n))


def mutual_rows(fwd, bwd) -> np.ndarray:
    """gulon_mutual_rows: fwd [ns] each source row's best target row, bwd [nt] each target row's best source row ->
    out [ns] int32, fwd[s] where the two chose each other and -1 elsewhere (mutual_rows_reference)."""
    fwd, bwd = N.i32(fwd).reshape(-1), N.i32(bwd).reshape(-1)
    out = np.zeros(max(len(fwd), 1), np.int32)
    N.check(N.lib().gulon_mutual_rows(fwd.ctypes.data if len(fwd) else None, len(fwd),
                                      bwd.ctypes.data if len(bwd) else None, len(bwd), out.ctypes.data))
    return out[:len(fwd)]


# ---- the seed ------------------------------------------------------------------------------------------------------------------

def _row_of(vectors):
    """word -> row of DeviceWordVectors in any order: its key index, or a dictionary (the first row of a repeated word)."""
    if vectors.key_index is not None:
        return vectors.key_index.lookup
    rows = {}
    for i, w in enumerate(vectors.words):
        rows.setdefault(w, i)
    return rows.get


def _check_sides(source, target):
    if source.matrix is None or target.matrix is None:
        raise ValueError("requirement failed: word vectors without rows cannot be aligned")
    if source.dimension != target.dimension:
        raise ValueError(f"requirement failed: the source has {source.dimension} dimensions, the target "
                         f"{target.dimension}")


def identical_pairs(source, target):
    """MUSE's identical_char seed: (w, w) for every word spelt the same on both sides, in the source's order."""
    there = _row_of(target)
    seen, pairs = set(), []
    for w in source.words:
        if w not in seen and there(w) is not None:
            seen.add(w)
            pairs.append((w, w))
    return pairs


def seed_alignment(source, target, pairs):
    """The orthogonal Procrustes solve on a seed dictionary.  source / target: DeviceWordVectors (any order; align reads
    them in file order), normalised on reading; pairs: [(source word, target word)] (csls.read_dictionary).  A pair with
    a word missing on either side is skipped and counted; the rest go through pair_moment as they come, repeated pairs
    included.  -> (Rotation(float32(procrustes(M))), used, skipped).  ValueError: different dimensions, no usable pair,
    a non-finite moment."""
    _check_sides(source, target)
    row_s, row_t = _row_of(source), _row_of(target)
    ra, rb, skipped = [], [], 0
    for s, t in pairs:
        rs, rt = row_s(s), row_t(t)
        if rs is None or rt is None:
            skipped += 1
        else:
            ra.append(int(rs))
            rb.append(int(rt))
    if not ra:
        raise ValueError(f"requirement failed: none of the {skipped} dictionary pairs has both of its words")
    m, used = pair_moment(source.matrix, target.matrix, ra, rb)
    if not np.isfinite(m).all():
        raise ValueError("the seed pairs have a non-finite moment")
    return Rotation(procrustes(m).astype(np.float32)), used, skipped


# ---- refinement ------------------------------------------------------------------------------------------------------------------

def _best_matches(side, other, offsets, out, dev):
    """out: one int32 per row of `side`'s range, on the device.  out[r] = the row of `other`'s range with the smallest
    distance + offsets[row] to row r of `side` (-1: none is finite): in batches of ROWS_PER_PASS rows, composed where
    they live as one-term expressions and asked of `other` at k = 1, the answers written straight into `out`.  Enqueued
    on the null stream."""
    L = N.lib()
    d = side.dimension
    for r0 in range(side.frm, side.until, ROWS_PER_PASS):
        b = min(ROWS_PER_PASS, side.until - r0)
        dev["off"].upload(np.arange(b + 1, dtype=np.int32))
        dev["rows"].upload(np.arange(r0, r0 + b, dtype=np.int32))
        dev["w"].upload(np.ones(b, np.float32))
        dev["q"].ensure(4 * b * d), dev["key"].ensure(4 * b)
        N.check(L.gulon_dataset_compose_rows_dev(side.matrix._h, dev["off"].ptr, dev["rows"].ptr, dev["w"].ptr, b, 1, 1,
                                                 dev["q"].ptr, None, None))
        N.check(L.gulon_exact_index_query_offset_dev(other._h, dev["q"].ptr, b, 1, offsets.ptr, None,
                                                     C.c_void_p(out.ptr.value + 4 * (r0 - side.frm)), dev["key"].ptr,
                                                     None, None))


def induce_matches(source_matrix, target_matrix, rotation, max_rank, neighbours):
    """One dictionary induction.  source_matrix X, target_matrix Y: DeviceMatrix of unit rows in frequency order;
    rotation: the current map W.  With Rs = min(max_rank, X.rows), Rt = min(max_rank, Y.rows): X W on the device, exact
    cosine indexes S over its first Rs rows and T over Y's first Rt, the CSLS mean similarities of each side to the
    other (csls_offsets, `neighbours` each), every S row's CSLS best T row (fwd) and every T row's best S row, and the
    mutual test.  All on the null stream; no result comes back to the host on the way.
    -> (fwd, match): device arrays (refine._DeviceArray) of Rs int32 each, match[s] = fwd[s] where the two rows chose
    each other, else -1.  The caller frees them."""
    from .csls import csls_offsets
    from .exact import ExactIndex
    from .refine import _DeviceArray
    if max_rank < 1:
        raise ValueError(f"requirement failed: max_rank = {max_rank} < 1")
    rs, rt = min(int(max_rank), source_matrix.rows), min(int(max_rank), target_matrix.rows)
    mapped = rotation.apply_device(source_matrix)
    S = T = r_s = r_t = None
    fwd, match = _DeviceArray(), _DeviceArray()
    dev = {name: _DeviceArray() for name in ("off", "rows", "w", "q", "key", "bwd")}
    try:
        S, T = ExactIndex(mapped, "cosine", 0, rs), ExactIndex(target_matrix, "cosine", 0, rt)
        r_t = csls_offsets(T, S, neighbours)        # per target row: its mean similarity to its nearest source rows
        r_s = csls_offsets(S, T, neighbours)
        fwd.ensure(4 * rs), match.ensure(4 * rs), dev["bwd"].ensure(4 * rt)
        _best_matches(S, T, r_t, fwd, dev)
        _best_matches(T, S, r_s, dev["bwd"], dev)
        N.check(N.lib().gulon_mutual_rows_dev(fwd.ptr, rs, dev["bwd"].ptr, rt, match.ptr, None))
        N.check(N.lib().gulon_device_synchronize())   # the scratch below is freed
        return fwd, match
    except BaseException:
        fwd.free(), match.free()
        raise
    finally:
        for a in dev.values():
            a.free()
        for x in (r_s, r_t):
            if x is not None:
                x.free()
        for x in (S, T):
            if x is not None:
                x.close()
        mapped.close()


def train_alignment(source, target, pairs, rounds=5, max_rank=15000, neighbours=10, write=None):
    """Learn the map of `source` into `target`'s space (DeviceWordVectors in file order, normalised on reading) from the
    seed dictionary `pairs`:
      1. W_0 = seed_alignment(source, target, pairs);
      2. for t = 0 .. rounds: (fwd, match) = induce_matches(X, Y, W_t, max_rank, neighbours) over Rs source rows;
         c_t = the mean cosine of the first V = min(Rs, 10000) source rows with their CSLS best target, as
         trace(W_t^T M) / used over M = the pair moment of the ORIGINAL X, Y on (0 .. V-1, fwd[:V]), in float64;
         unless t is the last: W_{t+1} = float32(procrustes(pair moment of X, Y on (0 .. Rs-1, match)));
         no mutual pair ends the rounds there;
      3. the W_t with the highest c_t, the lowest t on a tie.
    -> (Rotation, {"seed": {"used", "skipped"}, "rounds": [{"mutual", "asked", "criterion"} ...], "chosen": t}).
    write: the task log (None: silent).  ValueError as seed_alignment, and for rounds < 0."""
    from .build import log_task
    from .refine import _DeviceArray
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError("rounds must not be negative")
    rotation, used, skipped = log_task(write, "Solving the seed dictionary", lambda: seed_alignment(source, target, pairs),
                                       lambda r: f"Solved the seed dictionary: {r[1]} pairs, {r[2]} skipped")
    X, Y = source.matrix, target.matrix
    asked = min(int(max_rank), X.rows)
    order = _DeviceArray()
    order.upload(np.arange(max(asked, 1), dtype=np.int32))
    candidates, history = [], {"seed": {"used": used, "skipped": skipped}, "rounds": [], "chosen": 0}
    try:
        for t in range(rounds + 1):
            last = t == rounds

            def step():
                fwd, match = induce_matches(X, Y, rotation, max_rank, neighbours)
                try:
                    v = min(asked, CRITERION_ROWS)
                    m, hit = pair_moment_dev(X, Y, order.ptr, fwd.ptr, v)
                    criterion = float((rotation.matrix.astype(np.float64) * m).sum() / hit) if hit else -np.inf
                    m, mutual = pair_moment_dev(X, Y, order.ptr, match.ptr, asked)
                    entry = {"mutual": mutual, "asked": asked, "criterion": criterion}
                    if last or not mutual:
                        return entry, None
                    if not np.isfinite(m).all():
                        raise ValueError("the mutual pairs have a non-finite moment")
                    return entry, Rotation(procrustes(m).astype(np.float32))
                finally:
                    fwd.free(), match.free()
            entry, nxt = log_task(write, f"Alignment round {t}", step,
                                  lambda r: f"Alignment round {t}: {r[0]['mutual']} mutual pairs of {asked}, criterion "
                                            f"{r[0]['criterion']:.6f}")
            candidates.append(rotation)
            history["rounds"].append(entry)
            if nxt is None:
                break
            rotation = nxt
    finally:
        order.free()
    history["chosen"] = int(np.argmax([r["criterion"] for r in history["rounds"]]))
    return candidates[history["chosen"]], history
