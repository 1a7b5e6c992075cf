"""Expressions (gulon_amd/expressions.py): the grammar of `query-words -x`, the numpy restatement of the composition
arithmetic against cases worked out by hand, and the partition of a batch by its number of distinct operands: no GPU."""
from fractions import Fraction

import numpy as np
import pytest

from gulon_amd.expressions import (Expression, Term, compose_reference, distinct_operands, parse_expression,
                                   partition_by_operands, query_partitioned, to_csr)

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the grammar -----------------------------------------------------------------------------------------------------

def test_parse_words_and_operators():
    e = parse_expression("king - man + woman")
    assert e == Expression((Term("king", 1.0), Term("man", -1.0), Term("woman", 1.0)))
    assert parse_expression("paris") == Expression((Term("paris", 1.0),))
    assert parse_expression("  a\t+  a ") == Expression((Term("a", 1.0), Term("a", 1.0)))
    assert parse_expression("a - b - c").terms[2] == Term("c", -1.0)


def test_a_word_may_hold_operator_characters():
    """Only a token that IS + or - is an operator."""
    e = parse_expression("e-mail + c++ - -5 + +x")
    assert [t.key for t in e] == ["e-mail", "c++", "-5", "+x"]
    assert [t.weight for t in e] == [1.0, 1.0, -1.0, 1.0]
    assert parse_expression("a-b") == Expression((Term("a-b", 1.0),))


@pytest.mark.parametrize("line", ["", "   ", "+ a", "- a", "a +", "a -", "a + + b", "a - + b", "a b", "a + b c", "+",
                                  "a + b -", "+ +"])
def test_invalid_expressions(line):
    with pytest.raises(ValueError, match="invalid expression"):
        parse_expression(line)


def test_an_expression_needs_a_term():
    with pytest.raises(ValueError):
        Expression(())


# ---- the arithmetic --------------------------------------------------------------------------------------------------

def test_products_and_sums_round_on_their_own():
    """a = b = 1 + 2^-12: a * b = 1 + 2^-11 + 2^-24 exactly, a tie between two binary32 neighbours that rounds to the
    even one, 1 + 2^-11.  Minus (1 + 2^-11): the unfused chain gives 0, one fused multiply-add would give 2^-24."""
    a = F(1 + 2.0 ** -12)
    c = F(1 + 2.0 ** -11)
    exact = Fraction(float(a)) * Fraction(float(a)) - Fraction(float(c))
    assert exact == Fraction(1, 2 ** 24)                               # what an fma would return
    got = compose_reference([[a], [c]], [a, -1.0])
    assert got.dtype == np.float32 and got.tolist() == [0.0]
    # the same with the roles swapped: acc = 1 * c, then acc + (-a * a): the product is still rounded first
    assert compose_reference([[c], [a]], [1.0, -a]).tolist() == [0.0]


def test_last_bit_cases_in_list_order():
    """Three terms, weights 0.3 and -1.7 among them: the expected value is built one rounding at a time with exact
    rational arithmetic in between, and differs from the fused and from the reassociated evaluation."""
    def rn(x):                                                      # round a rational to binary32 (via binary64: the
        return F(float(x))                                          # operands below keep x exact in binary64)

    w = [F(0.3), F(-1.7), F(1.0)]
    v = [F(5772 / 4096), F(6733 / 4096), F(2251 / 4096)]
    p = [rn(Fraction(float(wi)) * Fraction(float(vi))) for wi, vi in zip(w, v)]
    want = rn(Fraction(float(rn(Fraction(float(p[0])) + Fraction(float(p[1]))))) + Fraction(float(p[2])))
    got = compose_reference([[x] for x in v], w)
    assert _bits(got)[0] == _bits(want)
    fused = F(float(Fraction(float(w[0])) * Fraction(float(v[0])) + Fraction(float(w[1])) * Fraction(float(v[1]))
                    + Fraction(float(w[2])) * Fraction(float(v[2]))))      # one rounding at the end
    backwards = compose_reference([[x] for x in v[::-1]], w[::-1])
    assert _bits(fused) != _bits(want) and _bits(backwards)[0] != _bits(want)
    print("in order", float(want), "single rounding", float(fused), "reversed", float(backwards[0]))


def test_a_product_of_binary32_is_exact_in_binary64():
    """(what rn() above relies on: 24 + 24 significand bits fit in 53)"""
    a, b = F(0.3), F(1 + 2.0 ** -12)
    assert Fraction(float(a) * float(b)) == Fraction(float(a)) * Fraction(float(b))


def test_normalisation_of_terms_and_of_the_sum():
    from gulon_amd.index import normalize
    rng = np.random.default_rng(5)
    V = rng.standard_normal((3, 7)).astype(np.float32)
    w = np.asarray([1, -1, 0.3], np.float32)
    terms = np.stack([normalize(r) for r in V])
    acc = (w[0] * terms[0]).astype(np.float32)
    acc = (acc + (w[1] * terms[1]).astype(np.float32)).astype(np.float32)
    acc = (acc + (w[2] * terms[2]).astype(np.float32)).astype(np.float32)
    assert np.array_equal(_bits(compose_reference(V, w, True, False)), _bits(acc))
    assert np.array_equal(_bits(compose_reference(V, w, True, True)), _bits(normalize(acc)))
    assert np.array_equal(_bits(compose_reference(V[:1], [1.0], False, True)), _bits(normalize(V[0])))
    assert np.array_equal(_bits(compose_reference(V[:1], [1.0])), _bits(V[0]))


def test_x_minus_x_is_zero_under_l2_and_nan_under_cosine():
    x = np.asarray([[0.5, -2.0, 3.25]], np.float32)
    both = np.concatenate([x, x])
    assert compose_reference(both, [1, -1]).tolist() == [0.0, 0.0, 0.0]
    assert np.isnan(compose_reference(both, [1, -1], True, True)).all()


def test_compose_reference_rejects_mismatched_input():
    for vectors, weights in (([[1.0]], [1.0, 2.0]), (np.zeros((0, 3)), []), ([1.0, 2.0], [1.0])):
        with pytest.raises(ValueError):
            compose_reference(vectors, weights)


# ---- the partition ---------------------------------------------------------------------------------------------------

def test_duplicate_operands_count_once():
    exprs = [[(5, 1.0)], [(5, 1.0), (5, -1.0)], [(1, 1.0), (2, -1.0), (1, 1.0)], [(1, 1.0), (2, 1.0), (3, 1.0)],
             [(9, 0.3)], [(4, 1.0), (7, 1.0)]]
    assert [distinct_operands(e) for e in exprs] == [1, 1, 2, 3, 1, 2]
    assert partition_by_operands(exprs) == {1: [0, 1, 4], 2: [2, 5], 3: [3]}
    assert list(partition_by_operands(exprs)) == [1, 2, 3]
    assert partition_by_operands([parse_expression("a + b - a")]) == {2: [0]}
    assert partition_by_operands([]) == {}


def test_csr_form():
    off, rows, w = to_csr([[(5, 1.0)], [Term(1, 1.0), Term(2, -1.7)], Expression((Term(3, 0.3),))])
    assert off.tolist() == [0, 1, 3, 4] and rows.tolist() == [5, 1, 2, 3]
    assert (off.dtype, rows.dtype, w.dtype) == (np.int32, np.int32, np.float32)
    assert np.array_equal(_bits(w), _bits([1.0, 1.0, -1.7, 0.3]))
    off, rows, w = to_csr([])
    assert off.tolist() == [0] and rows.size == 0 and w.size == 0


def test_partitioned_call_restores_the_input_order():
    exprs = [[(1, 1.0), (2, 1.0)], [(3, 1.0)], [(4, 1.0), (4, 1.0)], [(5, 1.0), (6, 1.0), (7, 1.0)]]
    calls = []

    def call(part, extra):
        calls.append((extra, [[t.key for t in e] for e in part]))
        first = np.asarray([e.terms[0].key for e in part], np.int32)
        return np.stack([first, first + extra], axis=1), first * 10

    rows, tens = query_partitioned(exprs, call, (((2,), np.int32, -1), ((), np.int32, 0)))
    assert calls == [(1, [[3], [4, 4]]), (2, [[1, 2]]), (3, [[5, 6, 7]])]
    assert rows.tolist() == [[1, 3], [3, 4], [4, 5], [5, 8]] and tens.tolist() == [10, 30, 40, 50]
