"""The device ingest's one-token conversion (gulon_amd/csrc/ingest_parse.h), compiled for the host
(tests/native/ingest_parse_host.c), against an exact rounding written here: the token as a Fraction, scaled to the
binary32 quantum of its binade (the subnormal quantum below 2^-126), rounded half to even on integers; a result of
2^128 is infinity.  Neither word_vectors.parse_float nor the code under test takes part in the expected side.

Every answer the function gives must be that rounding; what it may not decide it must flag.  The flagged share is
bounded where the issue bounds it (none of the %.6f tokens, at most 1 in 10 000 of the shortest round-trip decimals),
so that "flag everything" does not pass."""
from ingest_tokens import (check, check_edges, convert, crafted_midpoints_of_forty_digits, exact_bits,  # noqa: F401
                           fixed_six_decimals, long_significands, midpoints_of_eight_and_nine_digits,
                           outside_the_grammar, shortest_round_trip)


def test_exact_bits_knows_the_corner_cases():
    """The expected side, on values whose rounding is known by hand."""
    assert exact_bits("1") == 0x3F800000 and exact_bits("-2.5") == 0xC0200000
    assert exact_bits("16777217") == 0x4B800000 and exact_bits("16777219") == 0x4B800002      # ties to even
    assert exact_bits("3.4028234663852886e38") == 0x7F7FFFFF
    # the midpoint of the largest finite value and 2^128 is 340282356779733661637539395458142568448: it goes to
    # infinity (ties to even), its 17-digit truncation ...3366e38 lies below it, ...3367e38 above
    assert exact_bits("340282356779733661637539395458142568448") == 0x7F800000
    assert exact_bits("340282356779733661637539395458142568447") == 0x7F7FFFFF
    assert exact_bits("3.4028235677973366e38") == 0x7F7FFFFF and exact_bits("3.4028235677973367e38") == 0x7F800000
    assert exact_bits("1.401298464324817e-45") == 1
    assert exact_bits("7.006492321624085e-46") == 0 and exact_bits("7.006492321624086e-46") == 1   # half of it: tie
    assert exact_bits("-0") == 0x80000000 and exact_bits("1e-999") == 0 and exact_bits("-1e999") == 0xFF800000
    assert exact_bits("1.1754943508222875e-38") == 0x00800000


def test_fixed_six_decimals(convert):
    """%.6f of values in (-10, 10): at most 7 significant digits.  None may be flagged."""
    assert check(convert, "%.6f", fixed_six_decimals(11, 120000), 0) == 0


def test_shortest_round_trip_decimals(convert):
    """Shortest round-trip decimals of random finite binary32 bit patterns, subnormals included, in scientific and
    positional form: each must come back as the very pattern it was printed from; at most 1 in 10 000 flagged."""
    pats, sci, pos = shortest_round_trip(12, 120000)
    assert len(pats) >= 100000
    for name, toks in (("shortest scientific", sci), ("shortest positional", pos)):
        check(convert, name, toks, 1e-4)
        got = convert(toks)
        back = [(t, g, int(p)) for t, g, p in zip(toks, got, pats) if g is not None and g != int(p)]
        assert not back, back[:5]


def test_decimal_midpoints_of_eight_and_nine_digits(convert):
    """Integers of 8 and 9 digits that ARE midpoints of neighbouring binary32 values, and their neighbours one unit
    of the last decimal digit away: ties must go to even, the neighbours to their own side."""
    check(convert, "8/9-digit midpoints", midpoints_of_eight_and_nine_digits(13, 102000), 1e-4)


def test_crafted_midpoints_of_forty_digits(convert):
    """The tokens of tests/test_word_vectors.py::test_parse_float_is_correctly_rounded (generator restated): exact
    midpoints +- 10^-40 written with 40+ digits -- more than 19 significant digits may be flagged, never guessed."""
    check(convert, "crafted 40-digit midpoints", crafted_midpoints_of_forty_digits(5, 3000), None)


def test_long_significands_over_the_whole_range(convert):
    """10 to 19 significant digits with exponents from below the subnormals to above the overflow, and exact
    midpoints of binary32 values (subnormal ones too) cut to 19 digits: the wide-integer paths."""
    check(convert, "long significands", long_significands(14, 100000), 1e-4)


def test_edges(convert):
    """What a 64-bit significand decides, it must decide, except between the largest finite value and 2^128, where
    the function defers to the host reader: flagged, not converted (ingest_tokens.edges)."""
    check_edges(convert)


def test_outside_the_grammar_is_flagged(convert):
    tokens = outside_the_grammar()
    got = convert(tokens)
    assert [t for t, g in zip(tokens, got) if g is not None] == []
