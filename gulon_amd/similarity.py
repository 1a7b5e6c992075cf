"""Word-pair similarity: Spearman's rank correlation between the human scores of a benchmark file (WordSim-353,
SimLex-999, MEN, RW ...) and the distances an index puts between the two words of every pair (csrc/pairs.hip; DESIGN.md
9w).

The file: every line is `word1 word2 score`; blank lines and lines starting with `#` are skipped; `: name` opens a
section, as in a questions-words.txt file, so several benchmarks can be concatenated into one.  The model's value of a
pair is MathUtils.distanceSq between the two vectors `lookup` returns for its words, so a pair the annotators scored
HIGH should come out with a LOW distance: the report prints -rho of (distance, score), which is the rho of
(similarity, score) for any similarity that falls as the distance grows.  A pair with a word the target lacks is SKIPPED
and counted as such.

rho is Pearson's correlation of the average ranks.  With less = #{j : v[j] < v[i]} and eq = #{j : v[j] == v[i]} (i
itself included) the average rank of i is less + (eq + 1) / 2 and the mean rank (n + 1) / 2, so c = 2 * less + eq - n is
twice the centred rank, an integer: the device adds up c_x * c_y, c_x^2 and c_y^2 per section in int64 (rank_sums), and
rho = Sxy / sqrt(Sxx * Syy) is finished here (spearman).  Pearson's correlation of the values themselves is not offered.

Two routes give the same report:
  device   WordIndex (sorted and grouped) and ExactWordIndex: the rows, scores and sections are uploaded once, the
           handle's *_pair_distances_dev and gulon_rank_sums_dev run on one stream, the distances never reach the host,
           the int64 sums are read once, at the end;
  generic  any other target with `row_of` and `lookup` (a restriction, a refined or rotated form): both words are looked
           up, pair_distance_reference gives the distances and the host form gulon_rank_sums the sums."""
import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import native as N

Pair = Tuple[str, str, float]
MAX_PAIRS = 1 << 20


def read_pairs(lines, lowercase=False) -> List[Tuple[str, List[Pair]]]:
    """-> [(section name, [(word1, word2, score), ...]), ...] in file order.  Blank lines and lines starting with `#` are
    skipped.  A line starting with `:` opens a section named by the rest of the line; pairs before any header go to a
    section named "".  Any other line must hold exactly three whitespace-separated tokens, the third a finite number
    (word_vectors.parse_float), else ValueError naming its (1-based) line number.  lowercase: the words are lowered, the
    section names are not."""
    from .word_vectors import parse_float
    sections: List[Tuple[str, List[Pair]]] = []
    for number, line in enumerate(lines, 1):
        text = line.strip()
        if not text or text.startswith("#"):
            continue
        if text.startswith(":"):
            sections.append((text[1:].strip(), []))
            continue
        tokens = text.split()
        if len(tokens) != 3:
            raise ValueError(f"line {number}: expected two words and a score, found {len(tokens)} tokens")
        try:
            score = float(parse_float(tokens[2]))
        except ValueError:
            raise ValueError(f"line {number}: invalid score {tokens[2]!r}") from None
        if not math.isfinite(score):
            raise ValueError(f"line {number}: the score must be finite, found {tokens[2]!r}")
        a, b = (tokens[0].lower(), tokens[1].lower()) if lowercase else (tokens[0], tokens[1])
        if not sections:
            sections.append(("", []))
        sections[-1][1].append((a, b, score))
    return sections


# ---- references (numpy), as compose_reference and cosmul_reference are for their kernels --------------------------------

def pair_distance_reference(ya, yb) -> np.ndarray:
    """MathUtils.distanceSq(ya[i], yb[i]) for every i: ya, yb [n][d] (or [d]) float32 -> [n] float32 (or a scalar); one
    running float32 sum over the coordinates in ascending order, t = ya - yb, sum += t * t, every operation rounded on
    its own."""
    a, b = np.ascontiguousarray(ya, np.float32), np.ascontiguousarray(yb, np.float32)
    if a.shape != b.shape or a.ndim not in (1, 2):
        raise ValueError("requirement failed: two vectors, or two lists of vectors, of one shape")
    single = a.ndim == 1
    if single:
        a, b = a[None, :], b[None, :]
    acc = np.zeros(len(a), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(a.shape[1]):
            t = (a[:, e] - b[:, e]).astype(np.float32)
            acc = (acc + (t * t).astype(np.float32)).astype(np.float32)
    return acc[0] if single else acc


def rank_sums_reference(x, y, section, nsections) -> np.ndarray:
    """What gulon_rank_sums computes, in numpy: -> int64 [nsections][5] = {n_s, sum cx * cy, sum cx^2, sum cy^2,
    dropped} per section.  section None: one section.  A pair is live if neither value is NaN and its section lies in
    [0, nsections); c = 2 * less + eq - n_s over the live pairs of its section."""
    x, y = np.ascontiguousarray(x, np.float32).reshape(-1), np.ascontiguousarray(y, np.float32).reshape(-1)
    s = np.zeros(len(x), np.int64) if section is None else np.asarray(section, np.int64).reshape(-1)
    if len(y) != len(x) or len(s) != len(x) or (section is None and nsections != 1):
        raise ValueError("requirement failed: x, y and section of one length; one section without section ids")
    out = np.zeros((nsections, 5), np.int64)
    nan = np.isnan(x) | np.isnan(y)
    for sec in range(nsections):
        mine = s == sec
        out[sec, 4] = int((mine & nan).sum())
        live = np.flatnonzero(mine & ~nan)
        ns = len(live)
        c = []
        for v in (x[live], y[live]):
            less = (v[None, :] < v[:, None]).sum(axis=1, dtype=np.int64)
            eq = (v[None, :] == v[:, None]).sum(axis=1, dtype=np.int64)
            c.append(2 * less + eq - ns)
        out[sec, :4] = (ns, int((c[0] * c[1]).sum()), int((c[0] * c[0]).sum()), int((c[1] * c[1]).sum()))
    return out


def spearman(sxy, sxx, syy) -> float:
    """rho from the integer sums of one section: Sxy / sqrt(Sxx * Syy), the product taken in Python integers; nan when
    either list is constant (or empty)."""
    sxy, sxx, syy = int(sxy), int(sxx), int(syy)
    if sxx * syy == 0:
        return math.nan
    return sxy / math.sqrt(sxx * syy)


def rank_sums(x, y, section=None, nsections=1) -> np.ndarray:
    """gulon_rank_sums, the host form: x, y [n] float32, section [n] int32 or None -> int64 [nsections][5]."""
    x, y = N.f32(x).reshape(-1), N.f32(y).reshape(-1)
    n = len(x)
    if len(y) != n or (section is not None and np.size(section) != n):
        raise ValueError("requirement failed: x, y and section of one length")
    sec = None if section is None else N.i32(section).reshape(-1)
    out = np.zeros((max(nsections, 1), 5), np.int64)
    one = np.zeros(1, np.float32)
    N.check(N.lib().gulon_rank_sums(x if n else one, y if n else one,
                                    None if sec is None else (sec if n else np.zeros(1, np.int32)).ctypes.data, n,
                                    nsections, out.reshape(-1)))
    return out[:nsections]


def pair_distances_raw(fn, handle, rows_a, rows_b) -> np.ndarray:
    """One of the gulon_*_pair_distances host forms over two lists of row ids -> [n] float32."""
    a, b = N.i32(rows_a).reshape(-1), N.i32(rows_b).reshape(-1)
    if len(a) != len(b):
        raise ValueError(f"requirement failed: {len(a)} first rows for {len(b)} second rows")
    out = np.zeros(max(len(a), 1), np.float32)
    one = np.zeros(1, np.int32)
    N.check(fn(handle, a if len(a) else one, b if len(a) else one, len(a), out))
    return out[:len(a)]


def word_distances(target, pairs) -> List[Optional[np.float32]]:
    """`distances` of WordIndex and ExactWordIndex: per (word1, word2) the distance between the two words' vectors as
    the target's index stores them (its pair_distances), None where a word is absent."""
    pairs = list(pairs)
    rows = [(target.row_of(a), target.row_of(b)) for a, b in pairs]
    present = [i for i, (a, b) in enumerate(rows) if a is not None and b is not None]
    out: List[Optional[np.float32]] = [None] * len(pairs)
    if present:
        dist = target.index.pair_distances([rows[i][0] for i in present], [rows[i][1] for i in present])
        for i, v in zip(present, dist):
            out[i] = v
    return out


# ---- the report ------------------------------------------------------------------------------------------------------------

@dataclass
class SectionRho:
    """One section: n live pairs, the pairs skipped for an absent word, those dropped for a NaN distance, and the integer
    sums of the section's ranks -- x the distances, y the human scores."""
    name: str
    n: int = 0
    skipped: int = 0
    dropped: int = 0
    sxy: int = 0
    sxx: int = 0
    syy: int = 0

    @property
    def rho(self) -> float:
        """Spearman's rho between the scores and the SIMILARITY of the pairs: the distances' rho, negated."""
        return 0.0 - spearman(self.sxy, self.sxx, self.syy)

    def line(self) -> str:
        return f"{self.name}: rho {self.rho:.4f} (n = {self.n}, skipped {self.skipped}, dropped {self.dropped})"


@dataclass
class SimilarityReport:
    sections: List[SectionRho]
    total: SectionRho                     # over the pooled pairs of every section

    def lines(self) -> List[str]:
        """One line per section, then the `total:` line."""
        return [s.line() for s in self.sections] + [self.total.line()]


def _resolve(target, sections):
    """-> (skipped per section, rows of word1, rows of word2, scores, section ids) of the pairs both of whose words the
    target has."""
    skipped, a, b, y, sec = [0] * len(sections), [], [], [], []
    for s, (_, pairs) in enumerate(sections):
        for w1, w2, score in pairs:
            r1, r2 = target.row_of(w1), target.row_of(w2)
            if r1 is None or r2 is None:
                skipped[s] += 1
            else:
                a.append(int(r1)), b.append(int(r2)), y.append(score), sec.append(s)
    return skipped, N.i32(a), N.i32(b), N.f32(y), N.i32(sec)


def _device_distances(target):
    """The *_pair_distances_dev call of a target of the device route, as (d_rows_a, d_rows_b, n, d_out) -> None on the
    null stream; None for any other target."""
    from .exact import ExactWordIndex
    from .word_index import WordIndex
    if isinstance(target, ExactWordIndex):
        return target.index.pair_distances_dev
    if type(target) is not WordIndex:                    # a restriction, a refined or rotated form: the generic route
        return None
    return target.index.pair_distances_dev


def _sums_on_device(distances, a, b, y, sec, nsections):
    """The device route: -> int64 [nsections + 1][5], the last row the pooled total."""
    from .refine import _DeviceArray
    n, pooled = len(a), nsections >= 2
    out = np.zeros((nsections + 1, 5), np.int64)
    dev = {name: _DeviceArray() for name in ("a", "b", "y", "sec", "dist", "out")}
    try:
        dev["a"].upload(a), dev["b"].upload(b), dev["y"].upload(y), dev["sec"].upload(sec)
        dev["dist"].ensure(4 * n)
        dev["out"].ensure(out.nbytes)
        distances(dev["a"].ptr, dev["b"].ptr, n, dev["dist"].ptr)
        L = N.lib()
        N.check(L.gulon_rank_sums_dev(dev["dist"].ptr, dev["y"].ptr, dev["sec"].ptr, n, nsections, dev["out"].ptr, None))
        if pooled:
            total = C.c_void_p(dev["out"].ptr.value + nsections * 5 * 8)
            N.check(L.gulon_rank_sums_dev(dev["dist"].ptr, dev["y"].ptr, None, n, 1, total, None))
        read = out if pooled else out[:nsections]
        dev["out"].download(read)                           # the one read
    finally:
        for d in dev.values():
            d.free()
    if not pooled:
        out[nsections] = out[0]
    return out


def _sums_generic(target, sections, y, sec, nsections):
    """The generic route: `lookup` of both words, pair_distance_reference, the host form of the rank sums."""
    ya, yb = [], []
    for _, pairs in sections:
        for w1, w2, _ in pairs:
            if target.row_of(w1) is not None and target.row_of(w2) is not None:
                ya.append(target.lookup(w1)), yb.append(target.lookup(w2))
    x = pair_distance_reference(np.stack(ya), np.stack(yb))
    out = np.zeros((nsections + 1, 5), np.int64)
    out[:nsections] = rank_sums(x, y, sec, nsections)
    out[nsections] = rank_sums(x, y)[0] if nsections >= 2 else out[0]
    return out


def evaluate_pairs(target, sections, route=None) -> SimilarityReport:
    """Spearman's rho of `target` on `sections` (read_pairs), per section and over the pooled pairs.  route: None takes
    the device route where the target has one; "generic" forces the other, which every target with `row_of` and `lookup`
    has.  The report does not depend on the route.  At most 2^20 pairs."""
    if route not in (None, "generic"):
        raise ValueError(f"unknown route {route!r}")
    sections = [(name, list(pairs)) for name, pairs in sections]
    nsections = len(sections)
    skipped, a, b, y, sec = _resolve(target, sections)
    if len(a) > MAX_PAIRS:
        raise ValueError(f"requirement failed: {len(a)} pairs, at most {MAX_PAIRS} can be ranked")
    distances = None if route is not None else _device_distances(target)
    if len(a) == 0:
        sums = np.zeros((nsections + 1, 5), np.int64)
    elif distances is not None:
        sums = _sums_on_device(distances, a, b, y, sec, nsections)
    else:
        sums = _sums_generic(target, sections, y, sec, nsections)

    def score(name, row, skip):
        n, sxy, sxx, syy, dropped = (int(v) for v in row)
        return SectionRho(name, n, skip, dropped, sxy, sxx, syy)
    return SimilarityReport([score(name, sums[s], skipped[s]) for s, (name, _) in enumerate(sections)],
                            score("total", sums[nsections], sum(skipped)))
