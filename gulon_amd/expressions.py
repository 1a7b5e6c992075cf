"""Expression queries: a weighted sum of stored rows as the query, the operands removed from its answer
(csrc/compose.hip; DESIGN.md "Expression queries").

An expression is a non-empty list of terms (key, weight): the key a row of the index -- or, at the WordIndex level, a
word -- and the weight a binary32.  `king - man + woman` is [(king, 1), (man, -1), (woman, 1)]; a single term (w, 1) asks
for the neighbours of w that are not w.

The composed vector, with v_t = Index.lookup(row_t):
  1. normalize_terms: v_t = MathUtils.normalize(v_t);
  2. per coordinate acc = w_0 * v_0[e], then acc = acc + (w_t * v_t[e]) for t = 1, 2, ... in list order, every product
     and every sum rounded to binary32 on its own;
  3. normalize_query: MathUtils.normalize of the sum.
A cosine index sets both flags, an l2 index neither.  `compose_reference` restates this in numpy, bit for bit.

The answer to an expression at k: the index's answer to the composed vector at k + E, E = the number of DISTINCT term
rows, with the term rows removed and the first k kept.  A batch is partitioned by E (`partition_by_operands`) and
each part asked with extra = E, so an answer never depends on what else is in the batch."""
from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple, Union

import numpy as np


@dataclass(frozen=True)
class Term:
    """One operand: `key` is a row id (index level) or a word (WordIndex level)."""
    key: Union[int, str]
    weight: float = 1.0


@dataclass(frozen=True)
class Expression:
    terms: Tuple[Term, ...]

    def __post_init__(self):
        if len(self.terms) == 0:
            raise ValueError("requirement failed: an expression needs at least one term")

    def __iter__(self):
        return iter(self.terms)

    def __len__(self):
        return len(self.terms)


def as_expression(e) -> Expression:
    """An Expression, or any sequence of Terms / (key, weight) pairs."""
    if isinstance(e, Expression):
        return e
    return Expression(tuple(t if isinstance(t, Term) else Term(t[0], float(t[1])) for t in e))


def parse_expression(line: str) -> Expression:
    """`word (op word)*` split on whitespace, op one of the stand-alone tokens + and -: weights +1 and -1.  ValueError
    for an empty line, a leading or trailing operator, two operators in a row or two words in a row.  (A token such as
    `e-mail` or `c++` is a word: only a token that IS + or - is an operator.)"""
    tokens = line.split()
    terms, sign, want_word = [], 1.0, True
    for tok in tokens:
        is_op = tok in ("+", "-")
        if is_op == want_word:
            raise ValueError("invalid expression")
        if is_op:
            sign = 1.0 if tok == "+" else -1.0
        else:
            terms.append(Term(tok, sign))
        want_word = is_op
    if want_word:                                   # nothing at all, or a trailing operator
        raise ValueError("invalid expression")
    return Expression(tuple(terms))


def resolve_expressions(row_of, expressions):
    """Expressions over words (Expression objects, sequences of Term / (word, weight), or text for parse_expression)
    -> the same over row ids by `row_of` (word -> row or None); None where a word is absent."""
    out = []
    for e in expressions:
        e = parse_expression(e) if isinstance(e, str) else as_expression(e)
        rows = [row_of(t.key) for t in e]
        out.append(None if any(r is None for r in rows) else
                   Expression(tuple(Term(r, t.weight) for r, t in zip(rows, e))))
    return out


def compose_reference(vectors, weights, normalize_terms=False, normalize_query=False) -> np.ndarray:
    """The composed vector of one expression: vectors [T][d] = Index.lookup of its term rows, weights [T]."""
    from .index import normalize
    v = np.ascontiguousarray(vectors, np.float32)
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    if v.ndim != 2 or len(v) != len(w) or len(w) == 0:
        raise ValueError("requirement failed: one weight per vector, at least one of them")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        acc = None
        for t in range(len(w)):
            x = normalize(v[t]) if normalize_terms else v[t]
            p = (w[t] * x).astype(np.float32)                       # one rounding per product
            acc = p if acc is None else (acc + p).astype(np.float32)   # and one per sum
        return normalize(acc) if normalize_query else acc


COSMUL_EPS = np.float32(0.001)


def cosmul_reference(distances, weights) -> np.ndarray:
    """The 3CosMul scores of n rows against one expression (csrc/cosmul.hip): distances [E][n], the
    distance of every row to each term's vector as the index's ordinary query returns it; weights [E], a weight > 0 a
    positive term, any other a negative one.  s_t = max(1 - 0.25 * d_t, 0) with a NaN taken as 0; P and N the products of
    the positive and of the negative terms' s_t in list order, the first factor starting each, N = 1 without a negative
    term; score = P / (N + COSMUL_EPS).  Every operation is rounded to float32 on its own.  -> [n] float32."""
    d = np.ascontiguousarray(distances, np.float32)
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    if d.ndim != 2 or len(d) != len(w) or len(w) == 0 or not (w > 0).any():
        raise ValueError("requirement failed: one weight per row of distances, at least one of them positive")
    quarter, one, zero = np.float32(0.25), np.float32(1), np.float32(0)
    prod = {True: None, False: None}
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(len(w)):
            s = (one - (quarter * d[t]).astype(np.float32)).astype(np.float32)
            s = np.where(s > zero, s, zero).astype(np.float32)      # fmaxf(s, 0): a NaN goes to 0
            sign = bool(w[t] > 0)
            prod[sign] = s if prod[sign] is None else (prod[sign] * s).astype(np.float32)
        neg = np.ones(d.shape[1], np.float32) if prod[False] is None else prod[False]
        return (prod[True] / (neg + COSMUL_EPS).astype(np.float32)).astype(np.float32)


def distinct_operands(expression) -> int:
    return len({t.key for t in as_expression(expression)})


def partition_by_operands(expressions) -> Dict[int, List[int]]:
    """E -> the positions of the expressions with E distinct term keys, ascending E; a repeated operand counts once."""
    parts: Dict[int, List[int]] = {}
    for i, e in enumerate(expressions):
        parts.setdefault(distinct_operands(e), []).append(i)
    return dict(sorted(parts.items()))


def to_csr(expressions):
    """-> (term_offsets [b + 1], term_rows [T], term_weights [T]) for expressions over row ids."""
    exprs = [as_expression(e) for e in expressions]
    offsets = np.zeros(len(exprs) + 1, np.int32)
    offsets[1:] = np.cumsum([len(e) for e in exprs])
    rows = np.asarray([t.key for e in exprs for t in e], np.int32).reshape(-1)
    weights = np.asarray([t.weight for e in exprs for t in e], np.float32).reshape(-1)
    return offsets, rows, weights


def query_partitioned(expressions: Sequence, call, columns):
    """Runs call(part, extra) -> arrays (each with len(part) rows) once per partition of `expressions` by their number
    of distinct operands, extra = that number, and puts the rows back in input order.  columns: per returned array its
    (trailing shape, dtype, fill)."""
    exprs = [as_expression(e) for e in expressions]
    out = [np.full((len(exprs),) + tuple(shape), fill, dtype) for shape, dtype, fill in columns]
    for extra, where in partition_by_operands(exprs).items():
        got = call([exprs[i] for i in where], extra)
        for dst, src in zip(out, got):
            dst[where] = src
    return out
