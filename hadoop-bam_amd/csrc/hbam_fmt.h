// hbam_fmt.h -- the number formatters of the SAM text writer (hbam_samtext.hip),
// as __host__ __device__ functions so that a host program can check them
// against libc (tools/fmt_check.cpp).
//
//   ndigits_u32 / len_i32   the length of a decimal
//   fmt_u32 / fmt_i32       the decimal, most significant digit first
//   fmt_g                   a 32-bit float as C's printf("%g") in the "C" locale
//
// Every formatter writes through put(index, char) and returns the length, so a
// caller that only measures passes a put that does nothing.
//
// fmt_g is exact.  A finite float is m * 2^e with m < 2^24 and -149 <= e <= 104.
// With X the decimal exponent, the six significant digits are
// round-half-even(m * 2^e * 10^(5 - X)).  That product is a ratio of two
// integers below 2^192 (powers of 5 and 2 go to the numerator or the
// denominator by their sign), the quotient comes out of a 24-step restoring
// division and the remainder decides the rounding against half the
// denominator: ties and denormals round as glibc's exact printf does.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HBAM_FMT_HD __host__ __device__ inline
#else
#define HBAM_FMT_HD inline
#endif

namespace hbam {
namespace fmt {

HBAM_FMT_HD uint32_t pow10_u32(uint32_t k) {  // k <= 9
  uint32_t p = 1;
  for (uint32_t i = 0; i < k; ++i) p *= 10u;
  return p;
}

HBAM_FMT_HD uint32_t ndigits_u32(uint32_t v) {
  return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6
         : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}

HBAM_FMT_HD uint32_t abs_i32(int32_t v) { return v < 0 ? 0u - (uint32_t)v : (uint32_t)v; }  // INT_MIN -> 2^31
HBAM_FMT_HD uint32_t len_i32(int32_t v) { return ndigits_u32(abs_i32(v)) + (v < 0 ? 1u : 0u); }

template <class Put>
HBAM_FMT_HD uint32_t fmt_u32(uint32_t v, Put put) {
  const uint32_t nd = ndigits_u32(v);
  for (uint32_t k = nd; k-- > 0;) {
    put(k, (char)('0' + v % 10u));
    v /= 10u;
  }
  return nd;
}

template <class Put>
HBAM_FMT_HD uint32_t fmt_i32(int32_t v, Put put) {
  if (v >= 0) return fmt_u32((uint32_t)v, put);
  put(0u, '-');
  return 1u + fmt_u32(abs_i32(v), [&](uint32_t i, char c) { put(i + 1u, c); });
}

struct NoPut {
  HBAM_FMT_HD void operator()(uint32_t, char) const {}
};

// ---- 192-bit unsigned integers, little-endian words ---------------------------
constexpr int kBigWords = 6;
struct Big {
  uint32_t w[kBigWords];
};

HBAM_FMT_HD void big_set(Big& a, uint32_t v) {
#pragma unroll
  for (int i = 0; i < kBigWords; ++i) a.w[i] = 0;
  a.w[0] = v;
}

HBAM_FMT_HD void big_mul(Big& a, uint32_t m) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < kBigWords; ++i) {
    const uint64_t t = (uint64_t)a.w[i] * m + c;
    a.w[i] = (uint32_t)t;
    c = t >> 32;
  }
}

HBAM_FMT_HD void big_mul_pow5(Big& a, uint32_t k) {
  while (k >= 13u) {
    big_mul(a, 1220703125u);  // 5^13
    k -= 13u;
  }
  uint32_t p = 1;
  for (uint32_t i = 0; i < k; ++i) p *= 5u;
  big_mul(a, p);
}

HBAM_FMT_HD void big_shl(Big& a, uint32_t s) {
  while (s >= 32u) {
#pragma unroll
    for (int i = kBigWords - 1; i > 0; --i) a.w[i] = a.w[i - 1];
    a.w[0] = 0;
    s -= 32u;
  }
  if (s) {
#pragma unroll
    for (int i = kBigWords - 1; i > 0; --i) a.w[i] = (a.w[i] << s) | (a.w[i - 1] >> (32u - s));
    a.w[0] <<= s;
  }
}

HBAM_FMT_HD void big_shr1(Big& a) {
#pragma unroll
  for (int i = 0; i < kBigWords - 1; ++i) a.w[i] = (a.w[i] >> 1) | (a.w[i + 1] << 31);
  a.w[kBigWords - 1] >>= 1;
}

HBAM_FMT_HD int big_cmp(const Big& a, const Big& b) {
  int r = 0;
#pragma unroll
  for (int i = 0; i < kBigWords; ++i)  // the highest differing word decides
    if (a.w[i] != b.w[i]) r = a.w[i] > b.w[i] ? 1 : -1;
  return r;
}

HBAM_FMT_HD void big_sub(Big& a, const Big& b) {  // a >= b
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < kBigWords; ++i) {
    const uint64_t t = (uint64_t)a.w[i] - b.w[i] - borrow;
    a.w[i] = (uint32_t)t;
    borrow = (t >> 32) & 1u;
  }
}

// printf("%g") of the float with these bits.  At most 13 characters
// ("-1.17549e-38", "-0.000123457").
constexpr uint32_t kMaxG = 13;

template <class Put>
HBAM_FMT_HD uint32_t fmt_g(uint32_t bits, Put put) {
  uint32_t n = 0;
  const uint32_t be = (bits >> 23) & 0xffu, frac = bits & 0x7fffffu;
  if (be == 0xffu && frac) {  // libc prints the sign of a NaN; SAM text does not
    put(0u, 'n');
    put(1u, 'a');
    put(2u, 'n');
    return 3;
  }
  if (bits >> 31) put(n++, '-');
  if (be == 0xffu) {
    put(n++, 'i');
    put(n++, 'n');
    put(n++, 'f');
    return n;
  }
  if (be == 0 && frac == 0) {
    put(n++, '0');
    return n;
  }
  const uint32_t m = be ? (frac | 0x800000u) : frac;
  const int e = be ? (int)be - 150 : -149;
  const int bl = 31 - __builtin_clz(m) + e;  // floor(log2 v)
  // floor(bl * 0.30102921): floor(log10 v) or one less; the quotient's range settles it
  int X = (int)(((int64_t)bl * 78913) >> 18);
  uint32_t q = 0;
  for (int tries = 0; tries < 4; ++tries) {
    const int k = 5 - X;  // v * 10^k = v * 5^k * 2^k
    Big num, den;
    big_set(num, m);
    big_set(den, 1u);
    if (k >= 0) big_mul_pow5(num, (uint32_t)k); else big_mul_pow5(den, (uint32_t)-k);
    const int s2 = e + k;
    if (s2 >= 0) big_shl(num, (uint32_t)s2); else big_shl(den, (uint32_t)-s2);
    // q = num / den < 10^7 < 2^24, the remainder stays in num
    Big d = den;
    big_shl(d, 23u);
    q = 0;
    for (int b = 23; b >= 0; --b) {
      if (big_cmp(num, d) >= 0) {
        big_sub(num, d);
        q |= 1u << b;
      }
      big_shr1(d);
    }
    if (q >= 1000000u) {
      ++X;
      continue;
    }
    if (q < 100000u) {
      --X;
      continue;
    }
    big_shl(num, 1u);  // 2 * remainder against the denominator: half to even
    const int c = big_cmp(num, den);
    if (c > 0 || (c == 0 && (q & 1u))) ++q;
    if (q == 1000000u) {
      q = 100000u;
      ++X;
    }
    break;
  }
  uint32_t nd = 6;  // %g drops trailing zeros
  while (nd > 1u && q % 10u == 0) {
    q /= 10u;
    --nd;
  }
  auto digit = [&](uint32_t i) { return (char)('0' + (q / pow10_u32(nd - 1u - i)) % 10u); };
  if (X < -4 || X >= 6) {
    put(n++, digit(0));
    if (nd > 1u) {
      put(n++, '.');
      for (uint32_t i = 1; i < nd; ++i) put(n++, digit(i));
    }
    put(n++, 'e');
    put(n++, X < 0 ? '-' : '+');
    const uint32_t ax = (uint32_t)(X < 0 ? -X : X);  // <= 45
    put(n++, (char)('0' + ax / 10u));
    put(n++, (char)('0' + ax % 10u));
  } else if (X >= 0) {
    const uint32_t ni = (uint32_t)X + 1u;
    for (uint32_t i = 0; i < ni; ++i) put(n++, i < nd ? digit(i) : '0');
    if (nd > ni) {
      put(n++, '.');
      for (uint32_t i = ni; i < nd; ++i) put(n++, digit(i));
    }
  } else {
    put(n++, '0');
    put(n++, '.');
    for (int z = -1; z > X; --z) put(n++, '0');
    for (uint32_t i = 0; i < nd; ++i) put(n++, digit(i));
  }
  return n;
}

HBAM_FMT_HD uint32_t len_g(uint32_t bits) { return fmt_g(bits, NoPut()); }

// ---- the other direction: a decimal text as the nearest 32-bit float ------------
HBAM_FMT_HD uint32_t big_bits(const Big& a) {  // the bit length (0 for zero)
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < kBigWords; ++i)
    if (a.w[i]) r = 32u * (uint32_t)i + 32u - (uint32_t)__builtin_clz(a.w[i]);
  return r;
}

constexpr uint32_t kParseDigits = 19;  // significant digits that enter the value

// The float32 nearest to the decimal get(0) .. get(len - 1), ties to even, with
// no rounding through a double: false when the text is not
//   -?digits[.digits][(e|E)[+-]digits]  |  -?.digits[(e|E)[+-]digits]  |  nan  |  inf  |  -inf
// (nan is 0x7FC00000; hex floats, "infinity", a '+' sign and upper-case
// specials are refused).  Overflow gives +-inf, underflow denormals or +-0.
// The first kParseDigits significant digits make the integer D; nonzero digits
// behind them only say "a little more than D" (a sticky bit).  That is exact
// for every text of at most 19 significant digits -- all that %g, %.9g,
// Float.toString and Double.toString print -- and may be one unit off for a
// longer text whose first 19 digits end exactly on a float or on the midpoint
// of two.  The value D * 10^E is a ratio of two integers below 2^192 (the
// powers of 5 go to the numerator or the denominator by E's sign, the powers
// of 2 into the exponent); a 26-step restoring division gives the 25 or 26
// leading bits, and those, the remainder and the sticky bit round the 24 (or,
// for a denormal, fewer) that are kept.
template <class Get>
HBAM_FMT_HD bool parse_f32(Get get, uint32_t len, uint32_t* bits) {
  uint32_t i = 0, sign = 0;
  if (len == 3 && get(0u) == 'n' && get(1u) == 'a' && get(2u) == 'n') {
    *bits = 0x7fc00000u;
    return true;
  }
  if (i < len && get(i) == '-') {
    sign = 0x80000000u;
    ++i;
  }
  if (len - i == 3 && get(i) == 'i' && get(i + 1u) == 'n' && get(i + 2u) == 'f') {
    *bits = sign | 0x7f800000u;
    return true;
  }
  uint64_t D = 0;
  uint32_t nd = 0;   // significant digits in D
  int64_t e10 = 0;
  bool sticky = false;
  uint32_t nint = 0, nfrac = 0;
  for (; i < len; ++i, ++nint) {
    const uint32_t d = (uint32_t)(uint8_t)get(i) - '0';
    if (d > 9u) break;
    if (nd < kParseDigits) {
      if (D != 0 || d != 0) {
        D = D * 10u + d;
        ++nd;
      }
    } else {
      sticky |= d != 0;
      ++e10;
    }
  }
  if (i < len && get(i) == '.') {
    for (++i; i < len; ++i, ++nfrac) {
      const uint32_t d = (uint32_t)(uint8_t)get(i) - '0';
      if (d > 9u) break;
      if (nd < kParseDigits) {
        if (D != 0 || d != 0) {
          D = D * 10u + d;
          ++nd;
        }
        --e10;
      } else {
        sticky |= d != 0;
      }
    }
    if (nfrac == 0) return false;  // "1." and "."
  } else if (nint == 0) {
    return false;
  }
  if (i < len) {
    if (get(i) != 'e' && get(i) != 'E') return false;
    ++i;
    bool eneg = false;
    if (i < len && (get(i) == '+' || get(i) == '-')) {
      eneg = get(i) == '-';
      ++i;
    }
    if (i >= len) return false;
    int64_t x = 0;
    for (; i < len; ++i) {
      const uint32_t d = (uint32_t)(uint8_t)get(i) - '0';
      if (d > 9u) return false;
      if (x < 1000000) x = x * 10 + d;  // (saturates far outside the float range)
    }
    e10 += eneg ? -x : x;
  }
  if (D == 0) {
    *bits = sign;
    return true;
  }
  // 10^(nd - 1 + e10) <= D * 10^e10 < 10^(nd + e10)
  const int64_t top = (int64_t)nd + e10;
  if (top > 39) {  // >= 10^39 > FLT_MAX
    *bits = sign | 0x7f800000u;
    return true;
  }
  if (top < -45) {  // < 10^-45 < 2^-150, half the smallest denormal
    *bits = sign;
    return true;
  }
  Big num, den;
  big_set(num, (uint32_t)D);
  num.w[1] = (uint32_t)(D >> 32);
  big_set(den, 1u);
  if (e10 >= 0) big_mul_pow5(num, (uint32_t)e10); else big_mul_pow5(den, (uint32_t)-e10);  // |e10| <= 64
  // num / den * 2^sh in (2^24, 2^26)
  const int sh = 25 - ((int)big_bits(num) - (int)big_bits(den));
  if (sh >= 0) big_shl(num, (uint32_t)sh); else big_shl(den, (uint32_t)-sh);
  Big d = den;
  big_shl(d, 25u);
  uint32_t q = 0;
  for (int b = 25; b >= 0; --b) {
    if (big_cmp(num, d) >= 0) {
      big_sub(num, d);
      q |= 1u << b;
    }
    big_shr1(d);
  }
  const bool rest = sticky || big_bits(num) != 0;
  const int qb = 32 - (int)__builtin_clz(q);         // 25 or 26
  const int e = qb - 1 + (int)e10 - sh;              // the value lies in [2^e, 2^(e + 1))
  const int keep = e >= -126 ? 24 : 24 - (-126 - e);  // mantissa bits kept (a denormal keeps fewer)
  if (keep < 0) {  // below 2^-150
    *bits = sign;
    return true;
  }
  const uint32_t drop = (uint32_t)(qb - keep);  // 1 .. 26
  uint32_t m = q >> drop;
  const uint32_t low = q & ((1u << drop) - 1u), half = 1u << (drop - 1u);
  if (low > half || (low == half && (rest || (m & 1u)))) ++m;
  // a normal m carries its implicit bit into the exponent field; so does a rounding up to 2^24 or 2^23
  uint32_t r = e >= -126 ? m + ((uint32_t)(e + 126) << 23) : m;
  if (r >= 0x7f800000u) r = 0x7f800000u;
  *bits = sign | r;
  return true;
}

}  // namespace fmt
}  // namespace hbam
