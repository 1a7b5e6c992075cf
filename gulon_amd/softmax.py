"""The inverted softmax (csrc/logsumexp.hip): the retrieval rule `invsm_beta_30` of MUSE's evaluation,
after Smith et al., "Offline bilingual word vectors, orthogonal transformations and the inverted softmax", 2017.

Nearest-neighbour translation asks, per source word x, for the target row y with the largest cos(x, y).  The inverted
softmax normalises the other way round: the probability that target row y translates INTO source word x,

    P(x | y) = exp(beta * cos(x, y)) / sum_x' exp(beta * cos(x', y)),

and ranks the target rows of x by it.  A hub -- a target row near every source word -- has a large denominator and is
demoted, as CSLS demotes it by its mean similarity.  On unit vectors cos = 1 - d / 2, so log P(x | y) =
-(beta / 2) * (d(x, y) + (2 / beta) * L(y)) with

    L(y) = log sum_x' exp(-(beta / 2) * d(x', y)),

and ranking by P descending is ranking by t = d(x, y) + (2 / beta) * L(y) ascending: an offset query (csls.py;
DESIGN.md 9x) with offsets[y] = (2 / beta) * L(y).  L is a reduction over EVERY source row per target row, which no list
query supplies; ExactIndex.batch_query_logsumexp computes it on the device, csls.isf_offsets calls it for every target
row.

  logsumexp_reference   L and the number of terms over a distance matrix, in numpy float64 with the exactly rounded sum
  isf_offsets_from      the float32 offsets behind L
  isf_probabilities     P(x | y) behind the keys t of an offset query with those offsets

beta crosses the C ABI as a binary32 value, so every function here rounds it to float32 first: the products are then
the device's, bit for bit."""
import math

import numpy as np


def _beta(beta) -> float:
    """beta as the entry point takes it: a finite binary32 value > 0, widened."""
    with np.errstate(over="ignore"):
        b = float(np.float32(beta))
    if not (math.isfinite(b) and b > 0):
        raise ValueError(f"requirement failed: beta = {beta}: expected a finite value > 0")
    return b


def logsumexp_reference(dist_rows, beta, exclude=None, rows=None):
    """What gulon_exact_index_query_logsumexp computes, in numpy, with csls.offset_query_reference's conventions.
    dist_rows [b][n] float32: the distance of every query to n rows; rows [n] the row id of every column (None: the
    column number); exclude [b] one row id per query or -1 (None: none).  A column is a term of query q if and only if
    its distance is finite and its row is not exclude[q]; z = float64(d) * (-0.5 * float64(float32(beta))), e = exp(z),
    S = math.fsum of e over the terms -- the exactly rounded sum -- and L = log(S), -inf where S is 0.
    -> (L [b] float64, terms [b] int32)."""
    dist = np.ascontiguousarray(dist_rows, np.float32)
    if dist.ndim != 2:
        raise ValueError("requirement failed: dist_rows is [b][n]")
    b, n = dist.shape
    ids = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, np.int64).reshape(-1)
    if len(ids) != n:
        raise ValueError("requirement failed: one row id per column of dist_rows")
    ex = np.full(b, -1, np.int64) if exclude is None else np.asarray(exclude, np.int64).reshape(-1)
    if len(ex) != b:
        raise ValueError("requirement failed: one excluded row per query")
    scale = -0.5 * _beta(beta)
    L, terms = np.full(b, -np.inf, np.float64), np.zeros(b, np.int32)
    for q in range(b):
        term = np.isfinite(dist[q]) & (ids != ex[q])
        terms[q] = term.sum()
        s = math.fsum(np.exp(dist[q, term].astype(np.float64) * scale).tolist())
        L[q] = math.log(s) if s > 0 else -np.inf
    return L, terms


def isf_offsets_from(L, terms, beta) -> np.ndarray:
    """The offsets of the inverted softmax behind L [n] float64 and terms [n]: float32((2 / beta) * L) where
    terms > 0, +inf -- the row is masked -- where a row has no term.  ValueError where a row has terms and L is not
    finite: every term underflowed, beta is too large for these distances."""
    L = np.asarray(L, np.float64).reshape(-1)
    terms = np.asarray(terms).reshape(-1)
    if len(L) != len(terms):
        raise ValueError("requirement failed: one term count per L")
    live = terms > 0
    bad = np.flatnonzero(live & ~np.isfinite(L))
    if len(bad):
        raise ValueError(f"requirement failed: L[{bad[0]}] = {L[bad[0]]} over {int(terms[bad[0]])} terms: beta too "
                         f"large for these distances")
    out = np.full(len(L), np.inf, np.float32)
    out[live] = ((2.0 / _beta(beta)) * L[live]).astype(np.float32)
    return out


def isf_probabilities(keys, beta) -> np.ndarray:
    """exp(-(beta / 2) * t) in float64 for the keys t of an offset query with isf_offsets: the inverted-softmax
    probability P(x | y) of each listed translation y of the query x.  Over ALL the source words x it sums to 1 per
    target row y; the padding of a list (+inf) gives 0."""
    t = np.asarray(keys, np.float64)
    return np.exp(t * (-0.5 * _beta(beta)))
