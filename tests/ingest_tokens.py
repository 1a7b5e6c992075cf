"""Shared by tests/test_ingest_parse.py (the host build of gulon_amd/csrc/ingest_parse.h) and
tests/test_gpu_ingest_edges.py (the device build inside ingest_convert): the exact rounding that both are held to, the
check that compares a converter with it, the token families, and the fixture that builds the host converter.  No tests
in here.

A converter takes a list of tokens and returns, per token, the binary32's bits as an int, or None: flagged.

The expected side is an exact rounding written here: the token as a Fraction, scaled to the binary32 quantum of its
binade (the subnormal quantum below 2^-126), rounded half to even on integers; a result of 2^128 is infinity.  Neither
word_vectors.parse_float nor the code under test takes part in it."""
import math
import os
import random
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exact_bits(token):
    """Bits of the binary32 nearest to the decimal `token` (ties to even), from exact rationals."""
    v = Fraction(token)
    neg = token.lstrip().startswith("-")
    sign = 0x80000000 if neg else 0
    v = abs(v)
    if v == 0:
        return sign
    e = v.numerator.bit_length() - v.denominator.bit_length()       # 2^(e-1) < v < 2^(e+1)
    if Fraction(2) ** e > v:
        e -= 1
    assert Fraction(2) ** e <= v < Fraction(2) ** (e + 1)
    qe = max(e, -126) - 23                                          # exponent of the quantum in v's binade
    scaled = v / Fraction(2) ** qe
    m, rem = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rem
    if twice > scaled.denominator or (twice == scaled.denominator and (m & 1)):
        m += 1
    if m == 0:
        return sign
    if qe + m.bit_length() > 128:                                   # m * 2^qe >= 2^128
        return sign | 0x7F800000
    val = math.ldexp(float(m), qe)                                  # exact: m < 2^25, the result is a binary32
    return sign | struct.unpack("<I", struct.pack("<f", val))[0]


@pytest.fixture(scope="module")
def convert(tmp_path_factory):
    """The host converter: tests/native/ingest_parse_host.c, built by gcc."""
    exe = str(tmp_path_factory.mktemp("ingest_parse") / "ingest_parse_host")
    src = os.path.join(ROOT, "tests", "native", "ingest_parse_host.c")
    # -ffp-contract=off: the library's flag; the short path is one multiplication or one division
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-o", exe, src], check=True)

    def run(tokens):
        assert not any("\n" in t for t in tokens)
        out = subprocess.run([exe], input="".join(t + "\n" for t in tokens).encode("utf-8"), capture_output=True,
                             timeout=600, check=True).stdout.decode("ascii").split("\n")
        assert out[-1] == "" and len(out) == len(tokens) + 1
        return [None if o == "FLAG" else int(o, 16) for o in out[:-1]]
    return run


def check(convert, name, tokens, max_flagged_share):
    """Every answer `convert` gives is the exact rounding; the flagged share is at most max_flagged_share (None: no
    cap).  Returns the number of flagged tokens."""
    got = convert(tokens)
    flagged = sum(g is None for g in got)
    print(f"{name}: {len(tokens)} tokens, {flagged} flagged")
    wrong = [(t, f"{g:08x}", f"{exact_bits(t):08x}") for t, g in zip(tokens, got)
             if g is not None and g != exact_bits(t)]
    assert not wrong, (name, len(wrong), wrong[:5])
    if max_flagged_share is not None:
        assert flagged <= max_flagged_share * len(tokens), (name, flagged, len(tokens))
    return flagged


def fixed_six_decimals(seed, count):
    """%.6f of `count` values in (-10, 10): at most 7 significant digits."""
    rng = np.random.default_rng(seed)
    return ["%.6f" % x for x in rng.uniform(-10, 10, count)]


def shortest_round_trip(seed, count):
    """(patterns, scientific, positional): the shortest round-trip decimals, in both forms, of `count` binary32 bit
    patterns less those that are not finite -- 11 in 12 of them random, 1 in 24 positive subnormals, 1 in 24 negative
    ones."""
    rng = np.random.default_rng(seed)
    sub = count // 24
    pats = rng.integers(0, 1 << 32, count - 2 * sub, dtype=np.uint64).astype(np.uint32)
    pats = np.concatenate([pats, rng.integers(0, 1 << 23, sub, dtype=np.uint64).astype(np.uint32),         # subnormals
                           (rng.integers(0, 1 << 23, sub, dtype=np.uint64) | (1 << 31)).astype(np.uint32)])
    pats = pats[(pats >> 23) & 0xFF != 0xFF]
    vals = pats.view(np.float32)
    sci = [np.format_float_scientific(x, unique=True) for x in vals]
    pos = [np.format_float_positional(x, unique=True) for x in vals]
    return pats, sci, pos


def midpoints_of_eight_and_nine_digits(seed, count):
    """Integers of 8 and 9 digits that ARE midpoints of neighbouring binary32 values, and their neighbours one unit
    of the last decimal digit away, in four spellings; at least `count` tokens."""
    rnd = random.Random(seed)
    tokens = ["16777217", "16777216", "16777218", "16777219"]
    while len(tokens) < count:
        e = rnd.randrange(24, 30)
        ulp = 1 << (e - 23)
        mid = rnd.randrange(1 << 23, 1 << 24) * ulp + ulp // 2
        if 10 ** 7 <= mid < 10 ** 9:
            form = rnd.choice(["%d", "%d.0", "%d.", "%de0"])
            tokens += [form % mid, form % (mid - 1), form % (mid + 1)]
    return tokens


def crafted_midpoints_of_forty_digits(seed, count):
    """The tokens of tests/test_word_vectors.py::test_parse_float_is_correctly_rounded (generator restated): `count`
    exact midpoints +- 10^-40 written with 40+ digits, each followed by a 17-digit repr, after 14 fixed tokens."""
    rnd = random.Random(seed)
    toks = ["0.1", "1e-3", "-2.5", "3", "1.000000059604644775390625", "1.00000005960464477539062500001",
            "1.00000005960464477539062499999", "16777217", "16777219", "-16777217.0", "0.30000001192092896",
            "1.1754943508222875e-38", "7.0064923216240854e-46", "3.4028235e38"]
    for _ in range(count):
        mant = rnd.randrange(1 << 23, 1 << 24)
        e = rnd.randrange(-30, 30)
        mid = Fraction(2 * mant + 1, 2) * Fraction(2) ** e
        delta = Fraction(rnd.choice([-1, 0, 1]), 10 ** 40)
        v = mid + delta
        toks.append(f"{v.numerator * 10 ** 45 // v.denominator}e-45")
        toks.append(repr(rnd.uniform(-10, 10)))
    return toks


def long_significands(seed, count):
    """The wide-integer paths.  For 3 in 5 of `count`: a significand of 10 to 19 digits in two spellings, with
    exponents from below the subnormals to above the overflow.  For the other 2 in 5: the exact midpoint of a binary32
    value and its successor (subnormal ones too) cut to 19 digits, rounded down and up."""
    rnd = random.Random(seed)
    tokens = []
    for _ in range(count * 3 // 5):
        nd = rnd.randrange(10, 20)
        w = rnd.randrange(10 ** (nd - 1), 10 ** nd)
        tokens.append(f"{rnd.choice(['', '-', '+'])}{w}e{rnd.randrange(-70, 25)}")
        tokens.append(f"{w // 10 ** (nd - 1)}.{w % 10 ** (nd - 1):0{nd - 1}d}E{rnd.randrange(-50, 42)}")
    for _ in range(count - count * 3 // 5):
        p = rnd.randrange(0, 0x7F7FFFFF)
        lo, hi = (Fraction(struct.unpack("<f", struct.pack("<I", x))[0]) for x in (p, p + 1))
        mid = (lo + hi) / 2
        e10 = math.floor(math.log10(mid)) - 18
        w = mid / Fraction(10) ** e10
        for digits in {math.floor(w), math.ceil(w)}:                  # 19 digits just below / at / above the midpoint
            tokens.append(f"{digits}e{e10}")
    return tokens


def edges():
    """(tokens, must_decide, must_flag): the overflow edge, the subnormal edge, zeros, exponents out of range, the
    corners of the grammar.  Of the tokens, what a 64-bit significand decides must be decided (must_decide) ...
    except between the largest finite value and 2^128, where the function defers to the host reader (whose detour
    through the binary64 returns infinity for decimals just BELOW the midpoint as well; ingest_parse.h,
    GULON_PARSE_UNDECIDED): flagged, not converted (must_flag)."""
    tokens = ["3.4028234663852886e38", "3.4028235e38", "3.4028235677973365e38", "3.4028235677973366e38",
              "3.4028235677973367e38", "3.4028236e38", "-3.4028235677973366e38", "340282356779733661637539395458142568448",
              "1.401298464324817e-45", "1.4e-45", "1e-45", "7.006492321624085e-46", "7.006492321624086e-46",
              "7.0064923216240853e-46", "7.0064923216240854e-46", "7.1e-46", "7e-46", "-7.1e-46",
              "1.1754943508222875e-38", "1.1754942106924411e-38", "1.17549435e-38", "1.17549428e-38",
              "-0", "-0.0", "0", "+0", "0e99", "-0e-99", "0.000e5", "1e-999", "-1e-999", "1e999", "-1e999", "1e39",
              "1e38", "9.9999999999e38", "1e-46", "1e-65", "1e-66", "9999999999999999999e-65", "9999999999999999999e-66",
              "9999999999999999999e38", "9999999999999999999e19", "9999999999999999999e20", "5.", ".5", "-.5e1", "5.e-1",
              "00000000000000000000000001", "0.00000000000000000000000000000000000000000000140", "1" + "0" * 38,
              "1" + "0" * 39, "1e+5", "1E-5", "100000000000000000000", "123456789012345678900000",
              "0.000000000000000000000000000000000000000000001"]
    must_decide = ["3.4028235e38", "7.006492321624085e-46", "7.006492321624086e-46", "7.0064923216240853e-46", "1e39",
                   "-0", "0e99", "1e-999", "1e999", "1.401298464324817e-45", "3.4028234663852886e38", "1" + "0" * 39]
    must_flag = ["3.4028235677973365e38", "3.4028235677973366e38", "3.4028235677973367e38", "-3.4028235677973366e38"]
    return tokens, must_decide, must_flag


def check_edges(convert):
    """The edges through `convert`: nothing decided wrongly, must_decide decided, must_flag flagged.  Returns the
    answers."""
    tokens, must_decide, must_flag = edges()
    got = convert(tokens)
    for t, g in zip(tokens, got):
        assert g is None or g == exact_bits(t), (t, g, exact_bits(t))
    decided = dict(zip(tokens, got))
    for t in must_decide:
        assert decided[t] is not None, t
    for t in must_flag:
        assert decided[t] is None, t
    print("edges:", sum(g is None for g in got), "of", len(tokens), "flagged")
    return got


def outside_the_grammar():
    """Tokens the grammar of ingest_parse.h does not cover: every one must be flagged."""
    return ["NaN", "nan", "Infinity", "-Infinity", "inf", "0x1p3", "0x1.8p1", "1.5f", "1.5d", "1e", "1e+", "e5", ".",
            "+", "-", "", "1.0\r", " 1", "1 ", "\t1", "1_000", "1..2", "1.2.3", "--1", "+-1", "1e5.0", "1e 5",
            "١٢", "１", "1,5", "1" * 40, "0." + "3" * 40, "12345678901234567891",
            "1.00000000000000000001", "3" * 65, "0." + "0" * 70 + "1"]
