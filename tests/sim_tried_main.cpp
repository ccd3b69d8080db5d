// tests/sim_tried_main.cpp — the tried set of a constrained walk (csrc/sim_tried.hpp: plain C++, nothing of the device in it) against a naive list-based
// reference, built stand-alone with AddressSanitizer and UBSan by tests/test_sim_tried.py.  For total in {1, 63, 64, 65, 128, 255, 256}: every position is
// marked, one after the other, and before each marking the count, "all tried", membership of every position and the pick-th untried position for EVERY
// pick (and for one pick too many: -1) are compared with the list.  Orders of marking: all total! of them for total <= 6, and 40 seeded random orders
// plus ascending and descending for each of the sizes above.  The over-width test: tried_fits accepts 0 .. 256 and nothing else.
// Prints "ok <orders checked>" and exits 0, or the first disagreement and exits 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "sim_tried.hpp"

static int fail(const char* what, int total, int a, int b, int c) {
  std::printf("FAILED %s: total %d: %d %d %d\n", what, total, a, b, c);
  return 1;
}

// one order of marking, checked state by state; returns 0 when everything agrees
static int run_order(int total, const std::vector<int>& order) {
  TriedSet t;
  tried_clear(t);
  std::vector<bool> ref((size_t)total, false);                     // the reference: a flag per position, searched naively
  for (int step = 0; step <= total; step++) {
    std::vector<int> untried;
    for (int p = 0; p < total; p++)
      if (!ref[(size_t)p]) untried.push_back(p);
    if (tried_count(t) != total - (int)untried.size()) return fail("count", total, step, tried_count(t), (int)untried.size());
    if (tried_all(t, total) != untried.empty()) return fail("all", total, step, (int)tried_all(t, total), (int)untried.size());
    for (int p = 0; p < total; p++)
      if (tried_has(t, p) != ref[(size_t)p]) return fail("has", total, step, p, (int)ref[(size_t)p]);
    for (int pick = 0; pick < (int)untried.size(); pick++)
      if (tried_pick(t, total, pick) != untried[(size_t)pick]) return fail("pick", total, step, pick, tried_pick(t, total, pick));
    if (tried_pick(t, total, (int)untried.size()) != -1) return fail("pick past the end", total, step, (int)untried.size(), tried_pick(t, total, (int)untried.size()));
    if (tried_pick(t, total, -1) != -1) return fail("negative pick", total, step, -1, tried_pick(t, total, -1));
    if (step == total) break;
    tried_mark(t, order[(size_t)step]);
    ref[(size_t)order[(size_t)step]] = true;
  }
  // positions at and beyond `total` were never set: the words past the last position are untouched
  for (int p = total; p < (int)SIM_TRIED_BITS; p++)
    if (tried_has(t, p)) return fail("beyond total", total, p, 1, 0);
  tried_clear(t);
  if (tried_count(t) != 0 || tried_pick(t, total, 0) != 0) return fail("clear", total, tried_count(t), tried_pick(t, total, 0), 0);
  return 0;
}

int main() {
  long orders = 0;
  // every order on the small sizes
  for (int total = 1; total <= 6; total++) {
    std::vector<int> order((size_t)total);
    std::iota(order.begin(), order.end(), 0);
    do {
      if (run_order(total, order)) return 1;
      orders++;
    } while (std::next_permutation(order.begin(), order.end()));
  }
  // ascending, descending and seeded random orders on the sizes around the word boundaries
  const int sizes[] = {1, 63, 64, 65, 128, 255, 256};
  uint64_t x = 0x9E3779B97F4A7C15ULL;
  for (int total : sizes) {
    std::vector<int> order((size_t)total);
    std::iota(order.begin(), order.end(), 0);
    if (run_order(total, order)) return 1;
    std::reverse(order.begin(), order.end());
    if (run_order(total, order)) return 1;
    orders += 2;
    for (int rep = 0; rep < 40; rep++) {
      for (int i = total - 1; i > 0; i--) {                        // Fisher-Yates over xorshift64
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        std::swap(order[(size_t)i], order[(size_t)(x % (uint64_t)(i + 1))]);
      }
      if (run_order(total, order)) return 1;
      orders++;
    }
  }
  // total == 0: nothing to pick, vacuously all tried
  {
    TriedSet t;
    tried_clear(t);
    if (!tried_all(t, 0) || tried_pick(t, 0, 0) != -1) return fail("empty", 0, 0, 0, 0);
  }
  // the over-width error
  for (int total = -2; total <= 600; total++)
    if (tried_fits(total) != (total >= 0 && total <= 256)) return fail("fits", total, (int)tried_fits(total), 0, 0);
  if (SIM_TRIED_BITS != 256 || SIM_TRIED_WORDS != 4 || sizeof(TriedSet) != 32) return fail("width", SIM_TRIED_BITS, SIM_TRIED_WORDS, (int)sizeof(TriedSet), 0);
  std::printf("ok %ld\n", orders);
  return 0;
}
