// slice_policy_main.cpp — SlicePolicy (csrc/host_slice_policy.hpp) driven the way step_slices drives it, with a scripted number of instances per parent in
// the place of k_step_list.  Built and run by tests/test_slice_policy.py (g++ -fsanitize=address,undefined); exit status 0 and "ok" = every check held.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_slice_policy.hpp"

static int g_failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      g_failures++;                                       \
    }                                                     \
  } while (0)

static const uint64_t CAP = 64;

struct Outcome {
  bool failed = false;
  uint64_t failed_at = 0, accepted = 0, listings = 0, relisted = 0;
};

// the loop of step_slices: next, "launch", judge, consume
static Outcome drive(const std::vector<uint64_t>& ipp, SlicePolicy sp, const std::string& tag) {
  const uint64_t n = ipp.size();
  std::vector<int> cover(n, 0);
  Outcome o;
  uint64_t guard = 0;
  while (sp.next()) {
    CHECK(++guard <= 64 * (n + 1), "%s: the loop does not end", tag.c_str());
    if (guard > 64 * (n + 1)) break;
    CHECK(sp.lo < sp.end && sp.end <= n && sp.end - sp.lo <= sp.bound, "%s: slice [%llu, %llu)", tag.c_str(), (unsigned long long)sp.lo, (unsigned long long)sp.end);
    uint64_t inst = 0;
    for (uint64_t i = sp.lo; i < sp.end; i++) inst += ipp[i];
    const uint64_t lo = sp.lo, end = sp.end;
    const SliceVerdict v = sp.judge(inst);
    if (v == SliceVerdict::Fail) {
      CHECK(end - lo == 1 && inst > CAP, "%s: failure on %llu parents with %llu instances", tag.c_str(), (unsigned long long)(end - lo), (unsigned long long)inst);
      o.failed = true;
      o.failed_at = lo;
      break;
    }
    if (v == SliceVerdict::Relist) {
      CHECK(inst > CAP && sp.pos == lo, "%s: a slice that fits was listed again", tag.c_str());
      continue;
    }
    CHECK(inst <= CAP, "%s: accepted [%llu, %llu) with %llu instances", tag.c_str(), (unsigned long long)lo, (unsigned long long)end, (unsigned long long)inst);
    CHECK(sp.pos == end, "%s: pos after an accepted slice", tag.c_str());
    for (uint64_t i = lo; i < end; i++) cover[i]++;
    o.accepted++;
  }
  o.listings = sp.listings;
  o.relisted = sp.relisted;
  for (uint64_t i = 0; i < n; i++) {
    const int want = o.failed && i >= o.failed_at ? 0 : 1;
    CHECK(cover[i] == want, "%s: parent %llu lies in %d accepted slices", tag.c_str(), (unsigned long long)i, cover[i]);
  }
  CHECK(o.listings == o.accepted + o.relisted + (o.failed ? 1 : 0), "%s: listings", tag.c_str());
  return o;
}

int main() {
  int cases = 0;
  for (uint64_t n : {1, 63, 64, 65, 1000}) {
    std::vector<std::pair<std::string, std::vector<uint64_t>>> patterns;
    patterns.push_back({"zeros", std::vector<uint64_t>(n, 0)});
    patterns.push_back({"ones", std::vector<uint64_t>(n, 1)});
    std::vector<uint64_t> spike(n, 1);
    spike[n / 2] = 65;
    patterns.push_back({"spike", spike});
    std::vector<uint64_t> dense(n, 1);
    for (uint64_t i = n / 3; i < n / 3 + (n + 2) / 3; i++) dense[i] = 16;   // slices of more than four such parents overflow
    patterns.push_back({"dense", dense});
    for (const auto& p : patterns)
      for (uint64_t first : {(uint64_t)1, (uint64_t)3, slice_initial(CAP, 1, "VSRMC_NO_SUCH_KNOB"), (uint64_t)4096})
        for (int mode = 0; mode < 3; mode++) {   // doubling; adaptive under a bound of 64 parents; adaptive under a bound of 5
          const uint64_t bound = mode == 0 ? ~(uint64_t)0 : mode == 1 ? 64 : 5;
          const std::string tag = p.first + " n=" + std::to_string(n) + " first=" + std::to_string(first) + " mode=" + std::to_string(mode);
          const Outcome o = drive(p.second, SlicePolicy(0, n, CAP, first, mode != 0, bound), tag);
          const bool is_spike = p.first == "spike";
          CHECK(o.failed == is_spike, "%s: failed = %d", tag.c_str(), (int)o.failed);
          if (is_spike) CHECK(o.failed_at == n / 2, "%s: failed at %llu", tag.c_str(), (unsigned long long)o.failed_at);
          if (p.first == "zeros" || (p.first == "ones" && first <= CAP)) CHECK(o.relisted == 0, "%s: %llu void listings", tag.c_str(), (unsigned long long)o.relisted);
          if (p.first == "dense" && n >= 63 && first >= 64 && mode == 0) CHECK(o.relisted > 0, "%s: the dense run never overflowed the list", tag.c_str());
          cases++;
        }
  }
  // a range that does not start at 0 (a witness: one parent)
  {
    SlicePolicy sp(41, 42, CAP, 1);
    CHECK(sp.next() && sp.lo == 41 && sp.end == 42, "one parent");
    CHECK(sp.judge(7) == SliceVerdict::Accept && !sp.next(), "one parent accepted");
  }
  // the first slice
  CHECK(slice_initial(64, 8, "VSRMC_NO_SUCH_KNOB") == 8 && slice_initial(64, 0, "VSRMC_NO_SUCH_KNOB") == 64 && slice_initial(64, 1000, "VSRMC_NO_SUCH_KNOB") == 1, "list_cap / ords");
  bool knob = true;
  CHECK(slice_initial(64, 8, "VSRMC_NO_SUCH_KNOB", &knob) == 8 && !knob, "no knob");
  setenv("VSRMC_TEST_SLICE_KNOB", "7", 1);
  CHECK(slice_initial(64, 8, "VSRMC_TEST_SLICE_KNOB", &knob) == 7 && knob, "the knob overrides");
  setenv("VSRMC_TEST_SLICE_KNOB", "0", 1);
  CHECK(slice_initial(64, 8, "VSRMC_TEST_SLICE_KNOB") == 1, "a knob of 0 is one parent");
  CHECK(SlicePolicy(0, 10, CAP, 0).slice == 1 && SlicePolicy(0, 10, CAP, 100, true, 5).slice == 5, "the first slice is at least 1 and at most the bound");
  // halving, then growing back by doubling up to the first size and no further
  {
    SlicePolicy sp(0, 1000, CAP, 40);
    CHECK(sp.next() && sp.end == 40 && sp.judge(65) == SliceVerdict::Relist && sp.slice == 20, "halved");
    CHECK(sp.next() && sp.lo == 0 && sp.end == 20 && sp.judge(65) == SliceVerdict::Relist && sp.slice == 10, "halved again");
    CHECK(sp.next() && sp.end == 10 && sp.judge(64) == SliceVerdict::Accept && sp.slice == 20, "a list that is exactly full is accepted; doubled");
    CHECK(sp.next() && sp.lo == 10 && sp.end == 30 && sp.judge(0) == SliceVerdict::Accept && sp.slice == 40, "doubled to the first size");
    CHECK(sp.next() && sp.end == 70 && sp.judge(1) == SliceVerdict::Accept && sp.slice == 40, "capped at the first size");
    CHECK(sp.listings == 5 && sp.relisted == 2, "counters");
  }
  // the adaptive rule: list_cap / (1.5 * the largest instances per parent so far + 1), at most the bound, at least 1; it never grows back
  {
    SlicePolicy sp(0, 1000, CAP, 64, true, 48);
    CHECK(sp.slice == 48 && sp.next() && sp.end == 48, "bounded first slice");
    CHECK(sp.judge(48) == SliceVerdict::Accept && sp.slice == 25, "1 per parent -> 64 / 2.5");
    CHECK(sp.next() && sp.lo == 48 && sp.end == 73 && sp.judge(0) == SliceVerdict::Accept && sp.slice == 25, "the largest so far stays");
    CHECK(sp.next() && sp.judge(50) == SliceVerdict::Accept && sp.slice == 16, "2 per parent -> 64 / 4");
    CHECK(sp.next() && sp.end - sp.lo == 16 && sp.judge(65) == SliceVerdict::Relist && sp.slice == 8, "an overflow halves all the same");
    CHECK(sp.next() && sp.end - sp.lo == 8 && sp.judge(64) == SliceVerdict::Accept && sp.slice == 4, "8 per parent -> 64 / 13");
    SlicePolicy tiny(0, 10, CAP, 1, true, 48);
    CHECK(tiny.next() && tiny.judge(64) == SliceVerdict::Accept && tiny.slice == 1, "never less than one parent");
    SlicePolicy idle(0, 1000, CAP, 1, true, 48);
    CHECK(idle.next() && idle.judge(0) == SliceVerdict::Accept && idle.slice == 48, "no instance at all -> the bound");
  }
  if (g_failures) {
    std::printf("%d checks failed\n", g_failures);
    return 1;
  }
  std::printf("ok %d cases\n", cases);
  return 0;
}
