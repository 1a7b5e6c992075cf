/* One decimal token of a word2vec text file -> the correctly rounded binary32 (nearest, ties to even), or "flagged".
 *
 * This is the per-token arithmetic of the device ingest (ingest.hip), kept free of HIP types so that the system
 * compiler builds it for the host as well (tests/native/ingest_parse_host.c).  The contract is
 * word_vectors.parse_float, i.e. java.lang.Float.parseFloat on the tokens WordVectors.readWord2Vec meets
 * (WordVectors.scala:141-252): the function DECIDES a token exactly or FLAGS it; it never guesses.  A flagged
 * token is converted by the host's parse_float.
 *
 * Grammar:  [+-] digits* [ . digits* ] [ (e|E) [+-] digits+ ]   with at least one digit before the exponent.
 * Everything else is flagged: NaN, Infinity, hex floats, suffixes, whitespace (the \r of a CRLF line), non-ASCII
 * digits, underscores, a token longer than GULON_PARSE_MAX_TOKEN bytes, and a token with a non-zero digit after its
 * first GULON_PARSE_MAX_DIGITS significant ones (the significand is carried in 64 bits).
 *
 * Arithmetic, with the value = w * 10^q, 0 < w < 10^19:
 *   - w < 2^24 and |q| <= 10: float(w) and 10^|q| are exact, so ONE IEEE multiplication or division is the
 *     correctly rounded result (the %.6f tokens of a word2vec file all end here);
 *   - q > 38 is infinity, q < -65 is zero (w * 10^-66 < 10^-47 < 2^-150, half of the smallest subnormal);
 *   - otherwise exact integers of 160 bits: q >= 0: w * 5^q (< 2^153) * 2^q;  q < 0: the binary long division
 *     w / 5^-q (5^65 < 2^151), 32 quotient bits and the "remainder is non-zero" bit.  Both give the leading 32 bits
 *     of the value and a sticky bit, which round_bits turns into the binary32 -- subnormals and the overflow to
 *     infinity included.  Nothing is approximated; the path flags only the sliver under 2^128 described at
 *     GULON_PARSE_UNDECIDED, where it defers to the host reader.
 * The binary64 is never touched: rounding through it rounds twice. */
#ifndef GULON_INGEST_PARSE_H
#define GULON_INGEST_PARSE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define GULON_PARSE_HD __host__ __device__
#else
#define GULON_PARSE_HD
#endif

#define GULON_PARSE_MAX_TOKEN 64  /* bytes; the positional form of the smallest subnormal takes 48 */
#define GULON_PARSE_MAX_DIGITS 19 /* 10^19 < 2^64 */

/* a[0..4]: 160-bit unsigned integer, least significant limb first.  Loops are of fixed length and indices are
 * compile-time constants after unrolling, so the limbs stay in registers. */
static inline GULON_PARSE_HD void gulon_parse_mul_small(uint32_t a[5], uint32_t m) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    c += (uint64_t)a[i] * m;
    a[i] = (uint32_t)c;
    c >>= 32;
  }
}

/* a *= 5^k, 0 <= k <= 65 (the caller keeps the product below 2^160) */
static inline GULON_PARSE_HD void gulon_parse_mul_pow5(uint32_t a[5], int k) {
  while (k >= 13) {
    gulon_parse_mul_small(a, 1220703125u); /* 5^13 */
    k -= 13;
  }
  uint32_t p = 1;
  while (k-- > 0) p *= 5u;
  gulon_parse_mul_small(a, p);
}

/* number of bits of a (0 for a == 0) */
static inline GULON_PARSE_HD int gulon_parse_bitlen(const uint32_t a[5]) {
  int len = 0;
#pragma unroll
  for (int i = 0; i < 5; i++)
    if (a[i]) len = 32 * i + 32 - __builtin_clz(a[i]);
  return len;
}

/* a <<= s, 0 <= s < 160; no set bit may leave the 160 */
static inline GULON_PARSE_HD void gulon_parse_shl(uint32_t a[5], int s) {
  const int ws = s >> 5, bs = s & 31;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (ws > k) { a[4] = a[3]; a[3] = a[2]; a[2] = a[1]; a[1] = a[0]; a[0] = 0; }
  if (bs) {
#pragma unroll
    for (int i = 4; i >= 1; i--) a[i] = (a[i] << bs) | (a[i - 1] >> (32 - bs));
    a[0] <<= bs;
  }
}

/* Not a magnitude: the one region left to the host.  From a quarter of an ulp above the largest finite value up to
 * 2^128 the answer hangs on the midpoint 2^128 - 2^103, and there the host reader is the contract, not this function:
 * parse_float goes through the binary64, which IS that midpoint for every decimal within 2^74 of it, and returns
 * infinity also for those just below it (Float.parseFloat gives the largest finite value).  Flagging the region makes
 * both readers agree on every input; no word2vec file has such a token. */
#define GULON_PARSE_UNDECIDED 0xFFFFFFFFu

/* value = (hi + fraction) * 2^e2 with 2^31 <= hi < 2^32 and sticky = (fraction != 0)  ->  bits of the nearest
 * binary32 magnitude, ties to even; subnormals, zero and infinity included. */
static inline GULON_PARSE_HD uint32_t gulon_parse_round_bits(uint32_t hi, int sticky, int e2) {
  const int e = e2 + 31; /* 2^e <= value < 2^(e+1) */
  if (e > 127) return 0x7F800000u;
  if (e == 127 && hi >= 0xFFFFFF40u) return GULON_PARSE_UNDECIDED;
  int shift = 8;         /* bits of hi below the kept significand */
  int be = e + 127;
  if (be < 1) { shift += 1 - be; be = 1; }
  if (shift > 32) return 0u; /* value < 2^-150: below half of the smallest subnormal */
  const uint64_t h = hi;
  const uint64_t m = h >> shift, rem = h & (((uint64_t)1 << shift) - 1), half = (uint64_t)1 << (shift - 1);
  const int up = rem > half || (rem == half && (sticky || (m & 1)));
  /* m carries the implicit bit when normal (m >= 2^23): (be - 1) << 23 plus m puts it into the exponent field, and
   * a carry out of the significand moves on to the next binade (or to infinity) by itself */
  const uint32_t bits = ((uint32_t)(be - 1) << 23) + (uint32_t)m + (uint32_t)up;
  return bits > 0x7F800000u ? 0x7F800000u : bits;
}

/* magnitude bits of w * 10^q, w != 0, exactly rounded */
static inline GULON_PARSE_HD uint32_t gulon_parse_scale(uint64_t w, int q) {
  if (q > 38) return 0x7F800000u;
  if (q < -65) return 0u;
  if (w < (1u << 24) && q >= -10 && q <= 10) {
    float p = 1.0f;
    for (int i = q < 0 ? -q : q; i > 0; i--) p *= 10.0f; /* exact up to 10^10 = 2^10 * 9765625 */
    const float x = (float)(uint32_t)w;
    float r;
    if (q >= 0) r = x * p;
    else {
#if defined(__HIP_DEVICE_COMPILE__)
      r = __fdiv_rn(x, p);
#else
      r = x / p;
#endif
    }
    union { float f; uint32_t u; } v;
    v.f = r;
    return v.u;
  }
  if (q >= 0) {
    uint32_t a[5] = {(uint32_t)w, (uint32_t)(w >> 32), 0u, 0u, 0u};
    gulon_parse_mul_pow5(a, q);
    const int len = gulon_parse_bitlen(a);
    gulon_parse_shl(a, 160 - len);
    return gulon_parse_round_bits(a[4], (a[0] | a[1] | a[2] | a[3]) != 0, q + len - 32);
  }
  const int k = -q;
  uint32_t dv[5] = {1u, 0u, 0u, 0u, 0u};
  gulon_parse_mul_pow5(dv, k);
  const int sd = 159 - gulon_parse_bitlen(dv);
  gulon_parse_shl(dv, sd); /* 2^158 <= dv < 2^159 */
  uint32_t r[5] = {(uint32_t)w, (uint32_t)(w >> 32), 0u, 0u, 0u};
  const int sw = 158 - gulon_parse_bitlen(r);
  gulon_parse_shl(r, sw);  /* 2^157 <= r < 2^158 <= dv */
  /* w / 5^k = r / dv * 2^(sd - sw), r / dv in (1/4, 1): 33 or 34 steps of the restoring division fill 32 bits */
  uint32_t quo = 0;
  int n = 0;
  while (!(quo & 0x80000000u)) {
    uint32_t t[5];
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 4; i >= 1; i--) r[i] = (r[i] << 1) | (r[i - 1] >> 31);
    r[0] <<= 1;
#pragma unroll
    for (int i = 0; i < 5; i++) {
      const uint64_t x = (uint64_t)r[i] - dv[i] - borrow;
      t[i] = (uint32_t)x;
      borrow = (x >> 32) & 1u;
    }
    const uint32_t ge = borrow ? 0u : 1u;
#pragma unroll
    for (int i = 0; i < 5; i++) r[i] = ge ? t[i] : r[i];
    quo = (quo << 1) | ge;
    n++;
  }
  return gulon_parse_round_bits(quo, (r[0] | r[1] | r[2] | r[3] | r[4]) != 0, sd - sw - k - n);
}

/* Returns 1 and the binary32's bits in *out, or 0: flagged (*out untouched). */
static inline GULON_PARSE_HD int gulon_parse_f32(const unsigned char *s, int len, uint32_t *out) {
  if (len <= 0 || len > GULON_PARSE_MAX_TOKEN) return 0;
  int i = 0, neg = 0;
  if (s[0] == '+' || s[0] == '-') { neg = s[0] == '-'; i = 1; }
  uint64_t w = 0;
  int nd = 0, q = 0, seen = 0, toomany = 0;
  for (int frac = 0; frac < 2; frac++) {
    if (frac) {
      if (i < len && s[i] == '.') i++;
      else break;
    }
    while (i < len) {
      const unsigned c = (unsigned)s[i] - '0';
      if (c > 9u) break;
      i++;
      seen = 1;
      if (nd == 0 && c == 0) { q -= frac; continue; }    /* a leading zero carries no digit, only (after the point) scale */
      if (nd < GULON_PARSE_MAX_DIGITS) { w = w * 10u + c; nd++; q -= frac; }
      else { toomany |= c != 0; q += 1 - frac; }         /* a zero past the 19th digit only scales */
    }
  }
  if (!seen) return 0;
  if (i < len && (s[i] == 'e' || s[i] == 'E')) {
    i++;
    int eneg = 0, ex = 0, ne = 0;
    if (i < len && (s[i] == '+' || s[i] == '-')) { eneg = s[i] == '-'; i++; }
    while (i < len) {
      const unsigned c = (unsigned)s[i] - '0';
      if (c > 9u) break;
      i++;
      ne++;
      if (ex < 100000) ex = ex * 10 + (int)c;
    }
    if (!ne) return 0;
    q += eneg ? -ex : ex;
  }
  if (i != len || toomany) return 0;
  const uint32_t sign = neg ? 0x80000000u : 0u;
  const uint32_t mag = w == 0 ? 0u : gulon_parse_scale(w, q);
  if (mag == GULON_PARSE_UNDECIDED) return 0;
  *out = sign | mag;
  return 1;
}

#endif
