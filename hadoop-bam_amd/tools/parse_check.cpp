// parse_check -- host check of csrc/hbam_fmt.h's parse_f32 (the float reader of
// the SAM text parser) against glibc's strtof, which rounds correctly.  Test
// tool, not product.
//
//   parse_check [random_count]     default 2,000,000 float bit patterns
//
// Texts: "%.9g" (which round-trips every float) and "%g" of every power of two
// from 2^-149 to 2^127 with its neighbours, of the specials and of random bit
// patterns from a fixed seed; decimals of 17, 18 and 19 significant digits at
// and beside the midpoints of adjacent floats (the exact ties among them: the
// odd integers between 2^24 and 2^63), with the last digit moved up and down;
// overflow and underflow around FLT_MAX and the smallest denormal; the
// spellings of the grammar (a leading '.', exponents with and without a sign,
// leading zeros).  Every text has at most 19 significant digits or lies off
// the ties (parse_f32's stated limit: the 39-digit midpoint above FLT_MAX,
// an exact tie, is outside it).  A "%.9g" text must also give back the bits it was printed
// from.  Texts outside the grammar must be refused.
// Prints the counts; exit status 1 on any mismatch.
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

bool parse(const std::string& s, uint32_t* bits) {
  return hbam::fmt::parse_f32([&](uint32_t i) { return s[i]; }, (uint32_t)s.size(), bits);
}

void report(const std::string& text, const char* got, uint32_t a, uint32_t b) {
  if (++g_bad <= 20) fprintf(stderr, "MISMATCH '%s': %s 0x%08x, want 0x%08x\n", text.c_str(), got, a, b);
}

// parse_f32(text) against strtof(text)
void check_text(const std::string& text) {
  ++g_checked;
  uint32_t got = 0;
  if (!parse(text, &got)) {
    report(text, "refused", 0, 0);
    return;
  }
  char* end = nullptr;
  const uint32_t want = bits_of(strtof(text.c_str(), &end));
  if (*end != 0 || got != want) report(text, "got", got, want);
}

void check_refused(const std::string& text) {
  ++g_checked;
  uint32_t got = 0;
  if (parse(text, &got)) report(text, "accepted as", got, 0);
}

void check_bits(uint32_t b) {
  const float f = float_of(b);
  if (f != f) return;  // (NaN payloads have no text)
  char t[64];
  snprintf(t, sizeof t, "%.9g", (double)f);
  check_text(t);
  uint32_t got = 0;
  ++g_checked;
  if (!parse(t, &got) || got != b) report(t, "round trip", got, b);
  snprintf(t, sizeof t, "%g", (double)f);
  check_text(t);
}

void around(float f) {
  float lo = f, hi = f;
  check_bits(bits_of(f));
  check_bits(bits_of(-f));
  for (int k = 0; k < 3; ++k) {
    lo = nextafterf(lo, -INFINITY);
    hi = nextafterf(hi, INFINITY);
    check_bits(bits_of(lo));
    check_bits(bits_of(hi));
  }
}

// the decimal of `digits` significant digits nearest to x, and that decimal
// with its last mantissa digit one up and one down
void near(double x, int digits) {
  char t[80];
  snprintf(t, sizeof t, "%.*e", digits - 1, x);
  check_text(t);
  std::string s(t);
  const size_t e = s.find('e');
  for (int dir = -1; dir <= 1; dir += 2) {
    std::string u = s;
    size_t k = e - 1;
    while (true) {  // add dir to the mantissa's last digit, carrying
      if (u[k] == '.') {
        --k;
        continue;
      }
      const int d = u[k] - '0' + dir;
      if (d >= 0 && d <= 9) {
        u[k] = (char)('0' + d);
        break;
      }
      u[k] = dir > 0 ? '0' : '9';
      if (k == 0 || u[k - 1] == '-') {
        u.clear();  // (a carry out of the first digit: skip)
        break;
      }
      --k;
    }
    if (!u.empty()) check_text(u);
  }
}

void midpoints(float f) {  // of f and its upper neighbour, f finite and positive
  const float g = nextafterf(f, INFINITY);
  if (std::isinf(g)) return;
  const double mid = ((double)f + (double)g) * 0.5;  // exact: 25 significant bits
  for (int digits : {17, 18, 19}) {
    near(mid, digits);
    near(-mid, digits);
  }
  if (mid >= 16777216.0 && mid < 9.2e18) {  // an integer: its 19 digits are the exact tie
    char t[64];
    snprintf(t, sizeof t, "%.0f", mid);
    check_text(t);
    check_text(std::string(t) + ".0");
    check_text(std::string(t) + ".000000000000000000000000001");  // a sticky digit breaks the tie upward
    check_text(std::string("-") + t);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t random_count = argc > 1 ? strtoull(argv[1], nullptr, 10) : 2000000ull;

  for (int e = -149; e <= 127; ++e) {
    around(ldexpf(1.0f, e));
    midpoints(ldexpf(1.0f, e));
    midpoints(nextafterf(ldexpf(1.0f, e), 0.0f));
    midpoints(ldexpf(1.5f, e));
  }
  midpoints(0.0f);  // 2^-150: ties to zero
  // the specials and the spellings
  for (const char* t : {"nan", "inf", "-inf", "0", "-0", "0.0", "-0.0", "0e0", "00", "-000.000e-5", ".5", "-.5",
                        ".0", "5e3", "5E3", "5e+3", "5e-3", "5E-03", "0005.2500", "1e0000000000000000000001",
                        "1e-0000000000000000000001", "1e99999999999999999999", "1e-99999999999999999999",
                        "-1e99999999999999999999", "0e99999999999999999999", "0.000000000000000000000000000000000001",
                        "100000000000000000000000000000000000000", "1000000000000000000000000000000000000000",
                        "1.0000000596046448", "1.00000005960464478", "1.00000005960464477", "1.0000000596046447",
                        "3.4028236e38", "3.40282356e38", "3.4028235677973366e38", "3.4028235677973367e38",
                        "3.4028234e38", "340282346638528859811704183484516925440", "340282356779733661637539395458142568447",
                        "7.0064923216240853e-46", "7.0064923216240854e-46",
                        "7.006492321624085e-46", "7.006492321624086e-46", "1.4012984643248171e-45",
                        "2.1019476964872256e-45", "2.1019476964872257e-45", "1.1754943508222875e-38",
                        "1.1754942106924411e-38", "1.17549428e-38", "1.17549435e-38", "16777217", "16777219",
                        "16777217.0000000000000001", "9007199791611905", "123456789012345678901234567890",
                        "0.1", "0.2", "0.3", "3.14159274", "1e-45", "1e-46", "4e-46", "7e-46", "8e-46"})
    check_text(t);
  for (const char* t : {"", "-", "+1", "+inf", "1.", ".", "-.", "e5", ".e5", "1e", "1e+", "1e-", "1.e5", "0x1p3",
                        "0x10", "infinity", "-infinity", "NaN", "NAN", "INF", "Inf", "-nan", "1.5.2", "1 ", " 1", "1f",
                        "1e5.0", "--1", "1-", "na", "in", "i", "n", "nan0", "1,2"})
    check_refused(t);
  // random bit patterns, fixed seed (xorshift64*)
  uint64_t x = 0x9E3779B97F4A7C15ull;
  for (uint64_t i = 0; i < random_count; ++i) {
    x ^= x >> 12;
    x ^= x << 25;
    x ^= x >> 27;
    const uint32_t b = (uint32_t)((x * 0x2545F4914F6CDD1Dull) >> 32);
    check_bits(b);
    if ((i & 63) == 0 && (b & 0x7f800000u) != 0x7f800000u) midpoints(float_of(b & 0x7fffffffu));
  }
  printf("parse_check: %llu texts checked, %llu mismatches\n", (unsigned long long)g_checked,
         (unsigned long long)g_bad);
  return g_bad ? 1 : 0;
}
