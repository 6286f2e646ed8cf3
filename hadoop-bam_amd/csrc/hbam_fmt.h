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

}  // namespace fmt
}  // namespace hbam
