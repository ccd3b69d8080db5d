// sim_tried.hpp — the TRIED SET of a constrained random walk (vsr_sim_constrain.hpp): which of the enabled instances of the state a walker
// stands on have been drawn and refused already.  A bitmask over POSITIONS 0 .. total-1, position p being the p-th enabled instance in ordinal order.
// Plain C++ with no device call and nothing of the model in it: the kernel includes it with SIM_TRIED_FN set to its own function qualifiers, and
// tests/test_sim_tried.py builds it alone, with sanitizers, against a list-based reference (tests/sim_tried_main.cpp).
//
// The four words are four named members and every function spells them out: the set stays in registers.  (As an array walked by unrolled loops the
// compiler left three of the words in scratch memory: 32 bytes per lane.)
#pragma once
#include <cstdint>

#ifndef SIM_TRIED_FN
#define SIM_TRIED_FN inline
#endif

enum { SIM_TRIED_WORDS = 4, SIM_TRIED_BITS = 64 * SIM_TRIED_WORDS };   // 256 positions; no bound on the enabled instances is derived — the largest count met is 14 and a state beyond the width ends the run

struct TriedSet {
  uint64_t w0, w1, w2, w3;            // position p is bit p & 63 of word p >> 6
};

SIM_TRIED_FN int tried_popc64(uint64_t x) {
  x = x - ((x >> 1) & 0x5555555555555555ULL);
  x = (x & 0x3333333333333333ULL) + ((x >> 2) & 0x3333333333333333ULL);
  x = (x + (x >> 4)) & 0x0F0F0F0F0F0F0F0FULL;
  return (int)((x * 0x0101010101010101ULL) >> 56);
}

SIM_TRIED_FN void tried_clear(TriedSet& t) { t.w0 = t.w1 = t.w2 = t.w3 = 0; }

// a state with more enabled instances than the set has positions cannot be walked (the caller ends the run: VSRMC_SIM_ERR_TRIED_WIDTH)
SIM_TRIED_FN bool tried_fits(int total) { return total >= 0 && total <= (int)SIM_TRIED_BITS; }

SIM_TRIED_FN int tried_count(const TriedSet& t) { return tried_popc64(t.w0) + tried_popc64(t.w1) + tried_popc64(t.w2) + tried_popc64(t.w3); }

// every one of the `total` positions has been tried (total == 0: vacuously)
SIM_TRIED_FN bool tried_all(const TriedSet& t, int total) { return tried_count(t) >= total; }

SIM_TRIED_FN void tried_mark(TriedSet& t, int pos) {
  const uint64_t bit = (uint64_t)1 << (pos & 63);
  const int k = pos >> 6;
  t.w0 |= k == 0 ? bit : 0;
  t.w1 |= k == 1 ? bit : 0;
  t.w2 |= k == 2 ? bit : 0;
  t.w3 |= k == 3 ? bit : 0;
}

SIM_TRIED_FN bool tried_has(const TriedSet& t, int pos) {
  const int k = pos >> 6;
  const uint64_t w = k == 0 ? t.w0 : k == 1 ? t.w1 : k == 2 ? t.w2 : k == 3 ? t.w3 : 0;
  return (w >> (pos & 63)) & 1;
}

// one word of tried_pick: `left` positions of this word exist; pick counts the untried ones still to skip (negative: found already)
SIM_TRIED_FN void tried_pick_word(uint64_t tried_word, int left, int base, int& pick, int& pos) {
  uint64_t open = left <= 0 ? (uint64_t)0 : left >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << left) - 1);
  open &= ~tried_word;
  const int c = tried_popc64(open);
  if (pos < 0 && pick >= 0) {
    if (pick < c) {
      for (int skip = pick; skip > 0; skip--) open &= open - 1;    // drop the `pick` lowest untried positions
      pos = base + tried_popc64((open & (~open + 1)) - 1);         // the index of the lowest one left
    }
    pick -= c;                                                     // (negative once the position is found)
  }
}

// the position of the pick-th (0-based) UNTRIED one among positions 0 .. total-1, or -1 when fewer than pick + 1 are untried
SIM_TRIED_FN int tried_pick(const TriedSet& t, int total, int pick) {
  int pos = -1;
  tried_pick_word(t.w0, total, 0, pick, pos);
  tried_pick_word(t.w1, total - 64, 64, pick, pos);
  tried_pick_word(t.w2, total - 128, 128, pick, pos);
  tried_pick_word(t.w3, total - 192, 192, pick, pos);
  return pos;
}
