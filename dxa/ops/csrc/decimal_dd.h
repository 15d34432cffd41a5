// Decimal → double, correctly rounded (round to nearest, ties to even) for every input, as Java's
// Double.parseDouble is.  One routine, shared by the JSON parser, CAST(string AS DOUBLE) and the host check of the
// tests (it is __host__ __device__ and uses IEEE double operations and integers only, so all three agree).
//
// The digits arrive as two 19-digit halves and a flag: value = (head × 10^nt + tail + δ) × 10^(e10 − nt), where
// head holds the first 19 significant digits, tail the next nt (≤ 19) and 0 ≤ δ < 1 stands for the digits after
// the 38th (`sticky`: one of them is not zero).
//
//   1. Fast paths: zero, exact small exponents (both operands exact doubles, one IEEE operation), overflow and
//      underflow by the exponent alone.
//   2. A double-double estimate (hi, lo) of the value, relative error below 2^-101 (derivation at the code), in a
//      domain scaled by a power of two (pow10_dd.h) so that nothing in it is subnormal.
//   3. One rounding of hi + lo to the target grid: 53 bits, or the 2^-1074 grid below 2^-1022.  The estimate decides
//      unless hi + lo lies within its error bound of a rounding boundary (a midpoint of two neighbouring doubles).
//   4. Otherwise dxa_dd::resolve compares digits × 10^E with the boundary (2L + 1) × 2^b in exact integer
//      arithmetic (32-bit limbs; under 900 bits), reading the digits after the 38th from the text where they matter.
//      It is a cold noinline function: about one random long-mantissa text in 2^47 reaches it, besides true ties.
#pragma once
#include <stdint.h>

#include "pow10_dd.h"

#if defined(__HIPCC__)
#define DXA_DD_HD __host__ __device__
#else
#define DXA_DD_HD
#endif

namespace dxa_dd {

DXA_DD_HD inline double from_bits(uint64_t b) {
  double d;
  __builtin_memcpy(&d, &b, 8);
  return d;
}
DXA_DD_HD inline uint64_t to_bits(double d) {
  uint64_t b;
  __builtin_memcpy(&b, &d, 8);
  return b;
}
DXA_DD_HD inline double pow2(int e) { return from_bits((uint64_t)(e + 1023) << 52); }      // −1022 ≤ e ≤ 1023

// Unsigned integers of up to 1024 bits, little-endian 32-bit limbs; w[n..] is zero.  The bounds at `resolve` keep
// every value below 900 bits; a carry past the last limb is dropped rather than written out of bounds.
constexpr int kLimbs = 32;
struct Big {
  uint32_t w[kLimbs];
  int n;
};

DXA_DD_HD inline void big_set(Big& b, unsigned __int128 v) {
  for (int i = 0; i < kLimbs; ++i) b.w[i] = 0;
  b.n = 0;
  while (v) {
    b.w[b.n++] = (uint32_t)v;
    v >>= 32;
  }
}

DXA_DD_HD inline void big_mul_small(Big& b, uint32_t m) {
  uint64_t c = 0;
  for (int i = 0; i < b.n; ++i) {
    c += (uint64_t)b.w[i] * m;
    b.w[i] = (uint32_t)c;
    c >>= 32;
  }
  if (c && b.n < kLimbs) b.w[b.n++] = (uint32_t)c;
}

DXA_DD_HD inline void big_mul_pow5(Big& b, int a) {
  for (; a >= 13; a -= 13) big_mul_small(b, 1220703125u);                // 5^13 < 2^31
  uint32_t m = 1;
  for (; a > 0; --a) m *= 5;
  if (m > 1) big_mul_small(b, m);
}

DXA_DD_HD inline void big_shl(Big& b, int s) {
  if (b.n == 0 || s <= 0) return;
  const int ws = s >> 5, bs = s & 31;
  for (int i = kLimbs - 1; i >= 0; --i) {
    const int j = i - ws;
    uint32_t v = 0;
    if (j >= 0) {
      v = b.w[j] << bs;
      if (bs && j >= 1) v |= b.w[j - 1] >> (32 - bs);
    }
    b.w[i] = v;
  }
  b.n = b.n + ws + 1 > kLimbs ? kLimbs : b.n + ws + 1;
  while (b.n > 0 && b.w[b.n - 1] == 0) --b.n;
}

DXA_DD_HD inline int big_cmp(const Big& x, const Big& y) {
  if (x.n != y.n) return x.n < y.n ? -1 : 1;
  for (int i = x.n - 1; i >= 0; --i)
    if (x.w[i] != y.w[i]) return x.w[i] < y.w[i] ? -1 : 1;
  return 0;
}

DXA_DD_HD inline void big_sub(Big& x, const Big& y) {                    // x −= y, x ≥ y
  uint64_t borrow = 0;
  for (int i = 0; i < x.n; ++i) {
    const uint64_t d = (uint64_t)x.w[i] - y.w[i] - borrow;
    x.w[i] = (uint32_t)d;
    borrow = (d >> 32) & 1;
  }
  while (x.n > 0 && x.w[x.n - 1] == 0) --x.n;
}

// The double nearest to V = (head × 10^nt + tail + δ) × 10^(e10 − nt), known to be one of the neighbours
// lower = L × 2^ge and upper = (L + 1) × 2^ge: V is compared with their midpoint (2L + 1) × 2^(ge − 1) exactly.
//
// With D = head × 10^nt + tail (< 2^127), E = e10 − nt, N = 2L + 1 (< 2^55) and b = ge − 1, both sides are brought
// to integers: X = D × 5^max(E,0) × 2^max(E−b,0) against Q = N × 5^max(−E,0) × 2^max(b−E,0), and one unit of D is
// P = 5^max(E,0) × 2^max(E−b,0).  Sizes: −367 ≤ E ≤ 308, so a power of five has at most 853 bits; the caller
// only asks when V is within 2^-100 of the midpoint, so X and Q have the same length, which is that of the side
// that carries the power of five times a factor below 2^127: under 900 bits (and never more than 10 × P or
// 10 × Q in the digit loop).
//
// Without dropped digits (δ = 0) the comparison of X and Q decides, an equality being a tie: the even neighbour.
// With dropped digits X ≥ Q means above and X + P ≤ Q means below; in between, the boundary's own decimal
// expansion agrees with all 38 digits, and the digits after them are read from the text: R = Q − X is what the
// dropped digits must reach, R ← 10 R − d P per digit d, above as soon as R < 0, below as soon as R ≥ P (the
// remaining digits are worth less than one P), and below or tied when the digits run out.
//
// `text` is the number's text from its first digit (no sign); it is read up to the first character that is neither
// a digit nor '.', at most text_len characters.
DXA_DD_HD __attribute__((noinline)) inline double resolve(uint64_t head, uint64_t tail, int nt, int e10,
                                                          bool sticky, uint64_t L, int ge, const uint8_t* text,
                                                          int text_len) {
  const double lower = __builtin_ldexp((double)L, ge), upper = __builtin_ldexp((double)(L + 1), ge);
  unsigned __int128 D = head;
  for (int i = 0; i < nt; ++i) D *= 10;
  D += tail;
  const int E = e10 - nt, b = ge - 1;
  Big x, q;
  big_set(x, D);
  big_set(q, (unsigned __int128)(2 * L + 1));
  if (E >= 0) big_mul_pow5(x, E);
  else big_mul_pow5(q, -E);
  const int sh = E - b;
  if (sh >= 0) big_shl(x, sh);
  else big_shl(q, -sh);
  const int c = big_cmp(x, q);
  if (c > 0 || (c == 0 && sticky)) return upper;
  if (c == 0) return (L & 1) ? upper : lower;
  if (!sticky) return lower;
  big_sub(q, x);                                          // R, kept in q
  big_set(x, 1);                                          // P, built in x
  if (E >= 0) big_mul_pow5(x, E);
  if (sh >= 0) big_shl(x, sh);
  if (big_cmp(q, x) >= 0) return lower;
  int sig = 0;                                            // significant digits passed
  for (int i = 0; i < text_len; ++i) {
    const uint32_t ch = text[i];
    if (ch == '.') continue;
    const uint32_t d = ch - '0';
    if (d >= 10u) break;
    if (sig < 38) {
      if (sig || d) ++sig;
      continue;
    }
    big_mul_small(q, 10);
    for (uint32_t k = 0; k < d; ++k) {
      if (big_cmp(q, x) < 0) return upper;
      big_sub(q, x);
    }
    if (big_cmp(q, x) >= 0) return lower;
  }
  return q.n ? lower : ((L & 1) ? upper : lower);
}

}  // namespace dxa_dd

// The whole conversion.  head: the first 19 significant digits (0 only for a zero); tail, nt: the next nt ≤ 19;
// sticky: a non-zero digit followed them; e10: the decimal exponent of head's last digit; text, text_len: the
// number's text from its first digit, for `resolve`.  `exact` (tests), when given, is set to 1 where the exact
// path decided.
DXA_DD_HD __attribute__((always_inline)) inline double dxa_decimal_to_double(uint64_t head, int e10, uint64_t tail,
                                                                             int nt, bool sticky,
                                                                             const uint8_t* text, int text_len,
                                                                             int* exact = nullptr) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
  const double(*tab)[2] = c_pow10dd;
#else
  const double(*tab)[2] = h_pow10dd;
#endif
  if (head == 0) return 0.0;
  if (tail == 0 && !sticky && head < (1ull << 53)) {      // exact operands, one rounding
    if (e10 >= 0 && e10 <= 22) return (double)head * tab[e10 - DXA_POW10_DD_MIN][0];
    if (e10 < 0 && e10 >= -22) return (double)head / tab[-e10 - DXA_POW10_DD_MIN][0];
  }
  if (e10 > DXA_POW10_DD_MAX) return __builtin_inf();     // ≥ 1e309
  if (e10 < DXA_POW10_DD_MIN) return 0.0;                 // < 1e19 × 1e-349, below half the least subnormal
  // The estimate.  M = mh + ml + f is the mantissa (mh: head, without its low 11 bits when it has more than 53,
  // exact; ml < 2^11: those bits; f < 1: the tail as a fraction), P = ph + pl + ρ the table's 10^e10 × 2^K with
  // |pl| ≤ 2^-53 ph and |ρ| ≤ 2^-106 ph.  V × 2^K = M × P is summed as s + low with
  //     h + e1 = mh × ph, t2 + e2 = ml × ph (both exact: FMA residuals), s + r = h + t2 (exact two-sum),
  //     low = ((r + e1) + t1) + ((e2 + t3) + t4), t1 = mh × pl, t3 = f × ph, t4 = ml × pl.
  // Errors relative to V, with |r|, |e1|, |t1| ≤ 2^-53 V, |t2| ≤ 2^-42 V, |e2| ≤ 2^-95 V, and |t3| ≤ 2^-59 V,
  // |t4| ≤ 2^-95 V (a tail means head ≥ 1e18 > 2^59):
  //     ρ: 2^-106; rounding of t1: 2^-106; t3 with the rounding of tail and of the division: 3 × 2^-53 × 2^-59
  //     < 2^-110; t4: 2^-148; the sum r + e1 (≤ 2^-52 V): 2^-105; + t1 (≤ 2^-51 V): 2^-104; (e2 + t3) + t4: 2^-111;
  //     the last sum (≤ 2^-51 V): 2^-104; dropped: f × pl ≤ 2^-112, the digits after the 38th ≤ 1e-37 < 2^-122.
  // Together below 3.1 × 2^-104 < 2^-102; the factors (1 + 2^-52) left out above do not reach the next power of
  // two, and the bound used is 2^-101.  Contraction is off so that host and device round every product alike.
  const int K = e10 < -DXA_POW10_DD_SCALED_BEYOND ? DXA_POW10_DD_SCALE
                                                   : (e10 > DXA_POW10_DD_SCALED_BEYOND ? -DXA_POW10_DD_SCALE : 0);
  const double ph = tab[e10 - DXA_POW10_DD_MIN][0], pl = tab[e10 - DXA_POW10_DD_MIN][1];
  const bool wide = head >= (1ull << 53);
  const double mh = (double)(wide ? (head & ~0x7FFull) : head);
  const double h = mh * ph;
  const double e1 = __builtin_fma(mh, ph, -h);
  const double t1 = mh * pl;
  double s = h, low = e1 + t1;
  if (wide) {
    const double ml = (double)(head & 0x7FFull);
    const double t2 = ml * ph;
    const double e2 = __builtin_fma(ml, ph, -t2);
    s = h + t2;
    const double r = t2 - (s - h);                        // |h| ≥ |t2|
    const double f = nt ? (double)tail / tab[nt - DXA_POW10_DD_MIN][0] : 0.0;
    low = ((r + e1) + t1) + ((e2 + f * ph) + ml * pl);
  }
  const double hi = s + low;
  const double lo = low - (hi - s);                       // |s| ≥ |low|: exact, |lo| ≤ ulp(hi) / 2
  // One rounding.  hi is normal (the scaling sees to that), ue is the exponent of its ulp and qe that of the least
  // subnormal, both in the scaled domain.
  const uint64_t hb = dxa_dd::to_bits(hi);
  const int ex = (int)(hb >> 52) - 1023, ue = ex - 52, qe = -1074 + K;
  const double band = hi * 0x1p-101;
  uint64_t L;
  int ge;
  if (ue >= qe) {
    // 53 bits: hi is the answer unless hi + lo comes within `band` of hi ± half the gap to hi's neighbour on lo's
    // side; below a power of two that gap is half an ulp (not at 2^-1022, where subnormals keep the ulp)
    if (ex - K >= 1025) return __builtin_inf();
    const uint64_t mant = (hb & ((1ull << 52) - 1)) | (1ull << 52);
    const bool fine = mant == (1ull << 52) && lo < 0 && ue > qe;
    if (__builtin_fabs(lo) + band < dxa_dd::pow2(ue - (fine ? 2 : 1))) return __builtin_ldexp(hi, -K);
    if (lo > 0) { L = mant; ge = ue - K; }
    else if (fine) { L = 2 * mant - 1; ge = ue - 1 - K; }
    else { L = mant - 1; ge = ue - K; }
  } else {
    // below 2^-1022: round x = (hi + lo) / 2^qe to an integer, once.  n = rint(hi's part) stands unless that
    // part is exactly halfway (any other distance from a half is at least an ulp of it, and |lo| half of that);
    // then lo decides, if it is outside the band
    const double x = hi * dxa_dd::pow2(-qe), n = __builtin_rint(x);
    double res = n;
    if (__builtin_fabs(x - n) == 0.5) {
      const double fl = x - 0.5;
      if (__builtin_fabs(lo) > band) res = lo > 0 ? fl + 1.0 : fl;
      else { L = (uint64_t)fl; ge = -1074; res = -1.0; }
    }
    if (res >= 0.0) return __builtin_ldexp(res, qe - K);
  }
  if (exact) *exact = 1;
  return dxa_dd::resolve(head, tail, nt, e10, sticky, L, ge, text, text_len);
}
