// fmt_check -- host check of csrc/hbam_fmt.h (the number formatters of the SAM
// text writer) against libc's snprintf.  Test tool, not product.
//
//   fmt_check [random_count]     default 2,000,000 float bit patterns
//
// Floats: fmt_g against snprintf("%g") (libc's "-nan" read as "nan") over every
// power of two from 2^-149 to 2^127 with its two neighbours, the values around
// the fixed / exponent switch points, exact ties at the sixth digit, zeros,
// infinities, NaNs, the largest denormal and random bit patterns from a fixed
// seed.  Integers: fmt_i32 / fmt_u32 / the length functions against "%d" /
// "%u" around every power of ten and at the ends of the ranges.
// Prints the counts; exit status 1 on any mismatch.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../csrc/hbam_fmt.h"

namespace {

uint64_t g_checked = 0, g_bad = 0;

uint32_t bits_of(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

float float_of(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}

struct Buf {
  char c[32];
  uint32_t hi = 0;
  Buf() { memset(c, 0, sizeof c); }
};

void report(const char* what, const std::string& arg, const std::string& got, const std::string& want) {
  if (++g_bad <= 20) fprintf(stderr, "MISMATCH %s(%s): got '%s' want '%s'\n", what, arg.c_str(), got.c_str(), want.c_str());
}

void check_float_bits(uint32_t b) {
  Buf o;
  const uint32_t n = hbam::fmt::fmt_g(b, [&](uint32_t i, char ch) {
    if (i < sizeof o.c - 1) o.c[i] = ch;
    if (i + 1 > o.hi) o.hi = i + 1;
  });
  char want[64];
  snprintf(want, sizeof want, "%g", (double)float_of(b));
  const char* w = strcmp(want, "-nan") == 0 ? "nan" : want;
  ++g_checked;
  char arg[32];
  snprintf(arg, sizeof arg, "0x%08x", b);
  if (n != strlen(w) || n != o.hi || n > hbam::fmt::kMaxG || strcmp(o.c, w) != 0 || hbam::fmt::len_g(b) != n)
    report("fmt_g", arg, std::string(o.c) + "/" + std::to_string(n), w);
}

void check_float(float f) {
  check_float_bits(bits_of(f));
  check_float_bits(bits_of(-f));
}

void around(float f) {  // f, its neighbours and theirs
  float lo = f, hi = f;
  check_float(f);
  for (int k = 0; k < 3; ++k) {
    lo = nextafterf(lo, -INFINITY);
    hi = nextafterf(hi, INFINITY);
    check_float(lo);
    check_float(hi);
  }
}

void check_i32(int32_t v) {
  Buf o;
  const uint32_t n = hbam::fmt::fmt_i32(v, [&](uint32_t i, char ch) {
    if (i < sizeof o.c - 1) o.c[i] = ch;
  });
  char want[32];
  snprintf(want, sizeof want, "%d", v);
  ++g_checked;
  if (n != strlen(want) || strcmp(o.c, want) != 0 || hbam::fmt::len_i32(v) != n)
    report("fmt_i32", want, o.c, want);
}

void check_u32(uint32_t v) {
  Buf o;
  const uint32_t n = hbam::fmt::fmt_u32(v, [&](uint32_t i, char ch) {
    if (i < sizeof o.c - 1) o.c[i] = ch;
  });
  char want[32];
  snprintf(want, sizeof want, "%u", v);
  ++g_checked;
  if (n != strlen(want) || strcmp(o.c, want) != 0 || hbam::fmt::ndigits_u32(v) != n)
    report("fmt_u32", want, o.c, want);
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t random_count = argc > 1 ? strtoull(argv[1], nullptr, 10) : 2000000ull;

  // every power of two and its neighbours (2^-149 .. 2^127)
  for (int e = -149; e <= 127; ++e) around(ldexpf(1.0f, e));
  // the fixed / exponent switch points and the rounding that crosses them
  for (float f : {1e-4f, 9.999995e-5f, 9.99999e-5f, 0.000100000005f, 999999.5f, 999999.4375f, 999999.0f, 1e6f,
                  1000000.5f, 1e5f, 99999.95f, 99999.949f, 1e-5f, 1e-3f, 1.0f, 10.0f, 0.1f, 0.5f, 123456.0f,
                  1234567.0f, 0.000123456f, 3.14159274f, 1e10f, 1e-10f, 1e38f, 3.40282347e38f, 1.17549435e-38f})
    around(f);
  // exact ties at the sixth digit (all exactly representable): half to even
  for (float f : {100000.5f, 100001.5f, 100002.5f, 999998.5f, 1000005.0f, 1000015.0f, 1000025.0f, 10000050.0f,
                  10000150.0f, 12345.65f, 1234.565f, 1.0000005f, 2.0000015f, 8388607.5f, 16777215.0f, 4194303.5f,
                  1.5f, 2.5f, 0.0009765625f, 0.00048828125f, 1024.0009765625f, 65536.5f, 131072.5f, 262144.5f,
                  524288.5f, 1048577.0f, 2097155.0f})
    around(f);
  // 0.5-ulp cases: the midpoints of consecutive six-digit decimals that floats of
  // every binade hit or just miss
  for (uint32_t m = 0x800000u; m < 0x1000000u; m += 0x12345u)
    for (int e = -149; e <= 104; e += 7) check_float(ldexpf((float)m, e));
  // zeros, infinities, NaNs, denormals
  for (uint32_t b : {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u,
                     0xff800001u, 0x7fffffffu, 0xffffffffu, 0x007fffffu, 0x807fffffu, 0x00000001u, 0x80000001u,
                     0x00000002u, 0x00000003u, 0x00400000u, 0x00800000u, 0x7f7fffffu, 0xff7fffffu})
    check_float_bits(b);
  for (uint32_t b = 1; b < 0x800000u; b += 0x3fff) check_float_bits(b);  // across the denormals
  // random bit patterns, fixed seed (xorshift64*)
  uint64_t x = 0x9E3779B97F4A7C15ull;
  for (uint64_t i = 0; i < random_count; ++i) {
    x ^= x >> 12;
    x ^= x << 25;
    x ^= x >> 27;
    check_float_bits((uint32_t)((x * 0x2545F4914F6CDD1Dull) >> 32));
  }

  // integers: 0, +-1, 9/10, 99/100, ... up to 10^9, the ends of the ranges
  check_i32(0);
  check_u32(0);
  uint64_t p = 1;
  for (int k = 0; k <= 9; ++k, p *= 10) {
    for (int64_t d = -2; d <= 2; ++d) {
      const int64_t v = (int64_t)p + d;
      if (v >= 0 && v <= (int64_t)UINT_MAX) check_u32((uint32_t)v);
      if (v <= INT_MAX) {
        check_i32((int32_t)v);
        check_i32((int32_t)-v);
      }
    }
  }
  for (int32_t v : {INT_MIN, INT_MIN + 1, INT_MAX, INT_MAX - 1, -1, 1, 255, 256, 65535, 65536, -32768, 32767, -128, 127})
    check_i32(v);
  for (uint32_t v : {UINT_MAX, UINT_MAX - 1, (uint32_t)INT_MAX, (uint32_t)INT_MAX + 1u, 4294967295u, 4000000000u,
                     268435455u})
    check_u32(v);
  for (uint64_t i = 0; i < 200000; ++i) {
    x ^= x >> 12;
    x ^= x << 25;
    x ^= x >> 27;
    const uint32_t v = (uint32_t)((x * 0x2545F4914F6CDD1Dull) >> 32) >> (i % 32);
    check_u32(v);
    check_i32((int32_t)v);
    check_i32((int32_t)(0u - v));
  }

  printf("fmt_check: %llu values checked, %llu mismatches\n", (unsigned long long)g_checked, (unsigned long long)g_bad);
  return g_bad ? 1 : 0;
}
