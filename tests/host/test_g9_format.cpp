// tests/host/test_g9_format.cpp -- afec_amd/csrc/text/afx_g9.h against snprintf("%.9g"), byte for byte, as a stand-alone
// program (g++, and a second time with -fsanitize=address,undefined; tests/test_text_format_cpu.py builds and runs both):
//   * random bit patterns over all finite doubles, and more values inside [1e-18, 1e27)
//   * every power of ten 1e-323 .. 1e308 with its two neighbours
//   * constructed exact ties: q + 0.5, 10q + 5, (10q + 5) * 100, (10q + 5) / 2^s for nine-digit q, x.25 / x.75
//   * the smallest subnormal, DBL_MIN, DBL_MAX, +-0, NaN, +-infinity, and the exponent estimate for every binary exponent
//   test_g9_format [random patterns] [values in range]     (defaults 20000000 10000000)
#include <cfloat>
#include <clocale>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../afec_amd/csrc/text/afx_g9.h"

namespace {

// the random parts run on a few threads, each with a generator and counts of its own (snprintf costs about a microsecond
// on a value far from 1, which is most bit patterns)
thread_local long long g_checked = 0, g_failed = 0;
std::atomic<long long> g_all_checked{0}, g_all_failed{0};

thread_local uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t next_random() {   // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 0x2545F4914F6CDD1Dull;
}

double from_bits(uint64_t b) {
  double v;
  std::memcpy(&v, &b, 8);
  return v;
}

void check(double v) {
  char want[40], got[afx::kG9MaxChars + 1];
  if (std::isnan(v)) std::strcpy(want, "NaN");
  else if (std::isinf(v)) std::strcpy(want, v < 0 ? "-INF" : "INF");
  else std::snprintf(want, sizeof want, "%.9g", v);
  uint32_t limbs[afx::kG9Limbs];
  const afx::G9 g = afx::g9_digits(v, afx::G9Limbs{limbs, 1});
  const int n = afx::g9_write(g, got);
  ++g_checked;
  if (n != afx::g9_length(g) || n > afx::kG9MaxChars || (size_t)n != std::strlen(want) || std::memcmp(got, want, (size_t)n) != 0) {
    got[n < 0 ? 0 : n > afx::kG9MaxChars ? afx::kG9MaxChars : n] = 0;
    if (++g_failed <= 5) std::fprintf(stderr, "%.17g: got \"%s\" (length %d, g9_length %d), snprintf \"%s\"\n", v, got, n, afx::g9_length(g), want);
  }
}

void both_signs(double v) {
  check(v);
  check(-v);
}

uint32_t nine_digits() { return 100000000u + (uint32_t)(next_random() % 900000000ull); }

}  // namespace

int main(int argc, char** argv) {
  std::setlocale(LC_ALL, "C");
  const long long n_patterns = argc > 1 ? std::atoll(argv[1]) : 20000000, n_range = argc > 2 ? std::atoll(argv[2]) : 10000000;

  // the exponent estimate: floor(b * log10 2) for every binary exponent a double has
  for (int b = -1100; b <= 1100; ++b) {
    const int want = (int)std::floor((long double)b * 0.30102999566398119521373889472449L);
    if (afx::g9_floor_log10_pow2(b) != want) {
      std::fprintf(stderr, "g9_floor_log10_pow2(%d) = %d, not %d\n", b, afx::g9_floor_log10_pow2(b), want);
      return 1;
    }
  }

  const double specials[] = {0.0, 4.9406564584124654e-324, DBL_MIN, DBL_MAX, from_bits(0x000FFFFFFFFFFFFFull), from_bits(0x0010000000000001ull),
                             100000000.5, 100000001.5, 12345678.25, 12345678.75, 1000000005.0, 1000000015.0, 999999999.5, 99999999.95,
                             9.9999999995e-05, 1e-05, 123456789.0, 1234567890.0, 0.1, 0.5, 1.0, 1e-18, 1e27, 1e26, 1e-19, 9.999999995e26,
                             9.99999999e-19, 0.0001, 0.00001, 999999999.0, 1e9, 1e8};
  for (double v : specials) both_signs(v);
  check(std::nan(""));
  check(-std::nan(""));
  check(from_bits(0x7FF0000000000001ull));   // a signalling NaN's bits
  check(from_bits(0xFFFFFFFFFFFFFFFFull));
  both_signs(INFINITY);

  for (int x = -323; x <= 308; ++x) {
    char text[16];
    std::snprintf(text, sizeof text, "1e%d", x);
    const double p = std::strtod(text, nullptr);
    both_signs(p);
    both_signs(std::nextafter(p, 0.0));
    both_signs(std::nextafter(p, INFINITY));
  }

  for (int i = 0; i < 40000; ++i) {
    const uint32_t q = nine_digits();
    both_signs((double)q + 0.5);                            // nine digits and a half: exact
    both_signs((double)(10ull * q + 5));                    // ten digits, the last one 5
    both_signs((double)(10ull * q + 5) * 100.0);            // the same with zeros behind: below 2^53, exact
    both_signs((double)(10ull * q + 5) * 1e12);             // up to 1e22: still exact (below 2^53 times 5^12 * 2^12)
    for (int s = 1; s <= 60; s += 1 + (int)(next_random() % 7)) both_signs(std::ldexp((double)(10ull * q + 5), -s));
    const uint32_t x = (uint32_t)(next_random() % 100000000ull);   // up to eight digits before .25 / .75
    both_signs((double)x + 0.25);
    both_signs((double)x + 0.75);
    both_signs(((double)x + 0.25) / 1024.0);
    both_signs(std::ldexp((double)(2ull * q + 1), -1 - (int)(next_random() % 40)));
  }

  const int n_threads = 8;
  std::vector<std::thread> threads;
  for (int t = 0; t < n_threads; ++t)
    threads.emplace_back([=] {
      g_state = 0xD1B54A32D192ED03ull * (uint64_t)(t + 1);
      for (long long i = t; i < n_patterns; i += n_threads) {
        const uint64_t b = next_random();
        check(from_bits(((b >> 52) & 0x7FF) == 0x7FF ? b & ~(1ull << 62) : b));   // every finite double: an exponent of ones loses a bit
      }
      // inside [1e-18, 1e27): the binary exponents -60 .. 89 evenly, the ends cut off
      for (long long i = t; i < n_range;) {
        const uint64_t r = next_random();
        const double v = std::ldexp(1.0 + (double)(r >> 12) * 0x1p-52, -60 + (int)(r % 150));
        if (v < 1e-18 || v >= 1e27) continue;
        check((r & 0x800) ? -v : v);
        i += n_threads;
      }
      // the subnormals, which random patterns hardly reach
      for (int i = t; i < 1000000; i += n_threads) check(from_bits(next_random() >> 12 >> (next_random() % 52)));
      g_all_checked += g_checked;
      g_all_failed += g_failed;
    });
  for (std::thread& t : threads) t.join();
  g_checked += g_all_checked;
  g_failed += g_all_failed;

  std::printf("test_g9_format: %lld values, %lld differ from snprintf(\"%%.9g\")\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}
