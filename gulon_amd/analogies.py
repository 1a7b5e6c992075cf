"""Analogy accuracy: a:b :: c:d questions in the `questions-words.txt` format, asked of an index on the device
(csrc/analogy.hip).

The file: `: name` opens a section, every other line is `a b c d`.  A question is the expression
[(b, +1), (a, -1), (c, +1)] -- in that order, which fixes the bits of the composed vector (expressions.py) -- and counts
as correct at k when d is among the first k neighbours of it that are none of a, b, c.  A question with a word the
target lacks is SKIPPED and counted as such; a d that is itself one of the operands is asked and can never hit.

Two routes give the same report:
  device   WordIndex (sorted and grouped) and ExactWordIndex: per batch of up to BATCH questions the handle's
           *_query_terms_dev and gulon_analogy_counts_dev on one stream; the answer lists never reach the host, the two
           counter arrays are read once, at the end;
  generic  any other target with `row_of` and `batch_query_expressions` (a RefinedIndex, ...): its result lists are
           scored by the host form gulon_analogy_counts.

method "mul" asks the same questions by the multiplicative objective 3CosMul (csrc/cosmul.hip): the rows
are ranked by cos'(d, b) * cos'(d, c) / (cos'(d, a) + eps) instead of by their distance to b - a + c.  Its device route
(a flat WordIndex, an ExactWordIndex) is *_query_cosmul_dev in the place of *_query_terms_dev; its generic route asks
the target's `batch_query_cosmul`."""
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

from . import native as N
from .expressions import Expression, Term, to_csr
from .word_index import BATCH

Question = Tuple[str, str, str, str]
MAX_KS = 16


def read_questions(lines, lowercase=False) -> List[Tuple[str, List[Question]]]:
    """-> [(section name, [(a, b, c, d), ...]), ...] in file order.  A line starting with `:` opens a section named by
    the rest of the line; questions before any header go to a section named "".  Any other line must hold exactly four
    whitespace-separated tokens, else ValueError naming its (1-based) line number.  lowercase: the words are lowered,
    the section names are not."""
    sections: List[Tuple[str, List[Question]]] = []
    for number, line in enumerate(lines, 1):
        if line.lstrip().startswith(":"):
            sections.append((line.lstrip()[1:].strip(), []))
            continue
        tokens = line.split()
        if len(tokens) != 4:
            raise ValueError(f"line {number}: expected 4 words, found {len(tokens)}")
        if lowercase:
            tokens = [t.lower() for t in tokens]
        if not sections:
            sections.append(("", []))
        sections[-1][1].append(tuple(tokens))
    return sections


def question_expression(a, b, c) -> Expression:
    """b - a + c, in the order that fixes the bits."""
    return Expression((Term(b, 1.0), Term(a, -1.0), Term(c, 1.0)))


@dataclass
class SectionScore:
    """One section: questions asked, questions skipped for an absent word, and per k the questions whose d was among
    the first k answers."""
    name: str
    asked: int = 0
    skipped: int = 0
    hits: Dict[int, int] = field(default_factory=dict)

    def accuracy(self, k) -> float:
        return self.hits[k] / self.asked if self.asked else 0.0

    def line(self) -> str:
        scores = " ".join(f"@{k} {self.accuracy(k):.4f}" for k in sorted(self.hits))
        return f"{self.name}: {scores} (n = {self.asked}, skipped {self.skipped})"


@dataclass
class AnalogyReport:
    ks: Tuple[int, ...]
    sections: List[SectionScore]

    @property
    def total(self) -> SectionScore:
        out = SectionScore("total", hits={k: 0 for k in self.ks})
        for s in self.sections:
            out.asked += s.asked
            out.skipped += s.skipped
            for k in self.ks:
                out.hits[k] += s.hits[k]
        return out

    @property
    def asked(self):
        return self.total.asked

    @property
    def skipped(self):
        return self.total.skipped

    @property
    def hits(self):
        return self.total.hits

    def lines(self) -> List[str]:
        """One line per section, then the `total:` line."""
        return [s.line() for s in self.sections] + [self.total.line()]


def _check_ks(ks) -> Tuple[int, ...]:
    ks = tuple(int(k) for k in ks)
    if not ks or len(ks) > MAX_KS or ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"requirement failed: ks must be 1 to {MAX_KS} ascending values from 1 up, got {ks}")
    return ks


def _resolve(target, sections):
    """-> (skipped per section, the askable questions as (section, (row a, row b, row c), row d))."""
    skipped, asked = [0] * len(sections), []
    for s, (_, questions) in enumerate(sections):
        for q in questions:
            rows = [target.row_of(w) for w in q]
            if any(r is None for r in rows):
                skipped[s] += 1
            else:
                asked.append((s, (int(rows[0]), int(rows[1]), int(rows[2])), int(rows[3])))
    return skipped, asked


def _device_query(target):
    """The *_query_terms_dev call of a target of the device route, as
    (d_off, d_rows, d_w, b, k, extra, d_oi, d_od, d_oc, d_of) -> None on the null stream; None for any other target."""
    from .exact import ExactWordIndex
    from .word_index import WordIndex
    L = N.lib()
    if isinstance(target, ExactWordIndex):
        cosine, h = int(target.metric == "cosine"), target.index._h
        return lambda off, rows, w, b, k, extra, oi, od, oc, of: N.check(L.gulon_exact_index_query_terms_dev(
            h, off, rows, w, b, k, extra, cosine, cosine, oi, od, oc, of, None))
    if type(target) is not WordIndex:                   # a restriction, a refined or rotated form: the generic route
        return None
    cosine = int(target.metric == "cosine")
    if target._grouped:
        h = target.index._h
        strategy, limit = target.index._strategy()
        return lambda off, rows, w, b, k, extra, oi, od, oc, of: N.check(L.gulon_grouped_index_query_terms_dev(
            h, off, rows, w, b, k, extra, cosine, cosine, strategy, limit, oi, od, oc, None))
    pq = target.index.vector_index
    return lambda off, rows, w, b, k, extra, oi, od, oc, of: N.check(L.gulon_index_query_terms_dev(
        pq._h, off, rows, w, b, k, extra, cosine, cosine, 0, pq.length, oi, od, oc, of, None))


def _device_cosmul(target):
    """_device_query for method "mul": the *_query_cosmul_dev call of a flat WordIndex or an ExactWordIndex, with the
    arguments of _device_query's (extra and d_of are not used: the answer has no depth to choose and no tie flags)."""
    from .exact import ExactWordIndex
    from .word_index import WordIndex
    L = N.lib()
    if isinstance(target, ExactWordIndex):
        h = target.index._h
        return lambda off, rows, w, b, k, extra, oi, od, oc, of: N.check(L.gulon_exact_index_query_cosmul_dev(
            h, off, rows, w, b, k, 1, oi, od, oc, None, None))
    if type(target) is not WordIndex or target._grouped:
        return None
    pq = target.index.vector_index
    return lambda off, rows, w, b, k, extra, oi, od, oc, of: N.check(L.gulon_index_query_cosmul_dev(
        pq._h, off, rows, w, b, k, 1, 0, pq.length, oi, od, oc, None))


def _count_on_device(query, asked, ks, nsections, by_operands=True):
    """The device route: -> (hits [nsections][len(ks)], asked [nsections]).  by_operands: the questions are asked in
    parts by their number of distinct operands, which is the `extra` of each part."""
    from .refine import _DeviceArray
    kmax, nks = ks[-1], len(ks)
    hits, count = np.zeros((nsections, nks), np.int32), np.zeros(nsections, np.int32)
    names = ("off", "rows", "w", "expected", "section", "ks", "hits", "asked", "oi", "od", "oc", "of")
    dev = {name: _DeviceArray() for name in names}
    try:
        dev["ks"].upload(np.asarray(ks, np.int32))
        dev["hits"].upload(hits)
        dev["asked"].upload(count)
        parts: Dict[int, list] = {}
        for item in asked:                                  # by the number of distinct operands: extra = that number
            parts.setdefault(len(set(item[1])) if by_operands else 0, []).append(item)
        for extra in sorted(parts):
            part = parts[extra]
            for s in range(0, len(part), BATCH):
                batch = part[s:s + BATCH]
                b = len(batch)
                off, rows, w = to_csr([question_expression(*operands) for _, operands, _ in batch])
                dev["off"].upload(off), dev["rows"].upload(rows), dev["w"].upload(w)
                dev["expected"].upload(np.asarray([d for _, _, d in batch], np.int32))
                dev["section"].upload(np.asarray([sec for sec, _, _ in batch], np.int32))
                for name, itemsize in (("oi", 4 * kmax), ("od", 4 * kmax), ("oc", 4), ("of", 4)):
                    dev[name].ensure(b * itemsize)
                query(dev["off"].ptr, dev["rows"].ptr, dev["w"].ptr, b, kmax, extra, dev["oi"].ptr, dev["od"].ptr,
                      dev["oc"].ptr, dev["of"].ptr)
                N.check(N.lib().gulon_analogy_counts_dev(dev["oi"].ptr, dev["oc"].ptr, b, kmax, dev["expected"].ptr,
                                                         dev["section"].ptr, dev["ks"].ptr, nks, nsections,
                                                         dev["hits"].ptr, dev["asked"].ptr, None, None))
        dev["hits"].download(hits)                          # the one read, after the last batch
        dev["asked"].download(count)
    finally:
        for a in dev.values():
            a.free()
    return hits, count


def count_lists(lists, counts, expected, section, ks, nsections, hits=None, asked=None, ranks=False):
    """gulon_analogy_counts, the host form: lists [b][kin] int32 with counts[q] live entries -> (hits
    [nsections][len(ks)], asked [nsections]), added to the arrays given; ranks=True: also the rank of every question."""
    lists = N.i32(lists)
    b, kin = lists.shape
    ks = N.i32(ks).reshape(-1)
    hits = np.zeros((nsections, len(ks)), np.int32) if hits is None else hits
    asked = np.zeros(nsections, np.int32) if asked is None else asked
    rank = np.full(max(b, 1), -1, np.int32) if ranks else None
    one = np.zeros(1, np.int32)
    N.check(N.lib().gulon_analogy_counts(lists.reshape(-1) if lists.size else one, N.i32(counts) if b else one, b, kin,
                                         N.i32(expected) if b else one, N.i32(section) if b else one,
                                         ks if ks.size else one, len(ks), nsections,
                                         hits.reshape(-1) if hits.size else one, asked if asked.size else one,
                                         None if rank is None else rank.ctypes.data))
    return (hits, asked, rank[:b]) if ranks else (hits, asked)


def _count_generic(target, sections, ks, nsections, method="add"):
    """The generic route: the target's own batch_query_expressions (method "mul": batch_query_cosmul) over words, its
    lists scored by the host form."""
    kmax = ks[-1]
    hits, count = np.zeros((nsections, len(ks)), np.int32), np.zeros(nsections, np.int32)
    items = [(s, q) for s, (_, questions) in enumerate(sections) for q in questions
             if all(target.row_of(w) is not None for w in q)]
    for s0 in range(0, len(items), BATCH):
        batch = items[s0:s0 + BATCH]
        ask = target.batch_query_cosmul if method == "mul" else target.batch_query_expressions
        results = ask(kmax, [question_expression(a, b, c) for _, (a, b, c, _) in batch])
        lists, counts = np.full((len(batch), kmax), -1, np.int32), np.zeros(len(batch), np.int32)
        for i, r in enumerate(results):
            counts[i] = len(r.rows)
            lists[i, :counts[i]] = r.rows
        count_lists(lists, counts, [target.row_of(q[3]) for _, q in batch], [s for s, _ in batch], ks, nsections,
                    hits, count)
    return hits, count


def evaluate_analogies(target, sections, ks=(1, 5, 10), route=None, method="add") -> AnalogyReport:
    """The accuracy of `target` on `sections` (read_questions) at every k of `ks` (ascending, at most 16).  route: None
    takes the device route where the target has one; "generic" forces the other, which every target with `row_of` and
    `batch_query_expressions` has.  The report does not depend on the route.  method: "add", the neighbours of
    b - a + c (3CosAdd), or "mul", the multiplicative objective 3CosMul: a cosine target (ValueError otherwise) with
    `batch_query_cosmul` (NotImplementedError otherwise)."""
    ks = _check_ks(ks)
    if route not in (None, "generic"):
        raise ValueError(f"unknown route {route!r}")
    if method not in ("add", "mul"):
        raise ValueError(f"unknown method {method!r}")
    if method == "mul":
        if not hasattr(target, "batch_query_cosmul"):
            raise NotImplementedError(f"{type(target).__name__} has no cosmul queries: --method mul is not supported")
        if getattr(target, "metric", "cosine") != "cosine":
            raise ValueError("requirement failed: cosmul queries need a cosine index")
    sections = [(name, list(questions)) for name, questions in sections]
    nsections = len(sections)
    skipped, asked = _resolve(target, sections)
    query = None if route is not None else _device_cosmul(target) if method == "mul" else _device_query(target)
    if not asked:
        hits, count = np.zeros((nsections, len(ks)), np.int32), np.zeros(nsections, np.int32)
    elif query is not None:
        hits, count = _count_on_device(query, asked, ks, nsections, by_operands=method == "add")
    else:
        hits, count = _count_generic(target, sections, ks, nsections, method)
    return AnalogyReport(ks, [SectionScore(name, int(count[s]), skipped[s], {k: int(hits[s, j]) for j, k in enumerate(ks)})
                              for s, (name, _) in enumerate(sections)])
