// Host harness for the record's key split (test infrastructure): split_key_hd (csrc/dev_wave.hpp, the
// arithmetic of the device's split_key) against / and % on the CPU, for tests/test_split_key.py.
// Built with UBSan and AddressSanitizer (host code only).  Prints the number of keys checked; a
// mismatch is printed and ends the run with status 1.
#include <cstdint>
#include <cstdio>

#include "dev_wave.hpp"

static long g_checked = 0;

static bool check(int64_t key, int32_t C) {
  if (key < 0) return true;
  int64_t m = -1;
  int32_t c = -1;
  llampc::split_key_hd(key, C, m, c);
  ++g_checked;
  if (m == key / C && c == (int32_t)(key % C)) return true;
  std::printf("MISMATCH key %lld C %d: got (%lld, %d), want (%lld, %lld)\n", (long long)key, C, (long long)m, c,
              (long long)(key / C), (long long)(key % C));
  return false;
}

int main() {
  const int32_t Cs[] = {1, 2, 3, 63, 64, 65, 1000};
  bool ok = true;
  for (const int32_t C : Cs) {
    ok &= check(0, C) & check(C - 1, C) & check(C, C);
    // m C - 1, m C, m C + 1: every m up to 2^12, then a stride coprime to the small Cs up to 10^7
    for (int64_t m = 1; m <= 10000000; m += (m < 4096 ? 1 : 997)) ok &= check(m * C - 1, C) & check(m * C, C) & check(m * C + 1, C);
    ok &= check((int64_t)10000000 * C - 1, C) & check((int64_t)10000000 * C, C) & check((int64_t)10000000 * C + 1, C);
    // around 2^53 (the fp64 quotient's first rounding) and its multiples of C
    const int64_t p53 = (int64_t)1 << 53;
    for (int64_t d = -2048; d <= 2048; ++d) ok &= check(p53 + d, C);
    const int64_t m53 = p53 / C;
    for (int64_t d = -3; d <= 3; ++d) ok &= check((m53 + d) * C - 1, C) & check((m53 + d) * C, C) & check((m53 + d) * C + 1, C);
  }
  std::printf("checked %ld\n", g_checked);
  return ok ? 0 : 1;
}
