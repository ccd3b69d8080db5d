// host_slice_policy.hpp — which parents the next k_step_list launch lists, and what the number of instances it offered means.  Plain host
// C++, no HIP call and nothing of the model in it: step_slices (host_step_slices.hpp) asks it between launches, and tests/test_slice_policy.py drives it
// with a scripted number of instances per parent in the place of the kernel.
//
// A listing that offered more instances than the list holds is void: nothing of it is consumed, the same parents are listed again half at a time, and one
// parent that overflows alone is the failure.  After an accepted slice the next one is either the current size doubled, up to the first one (a slice that
// was halved grows back once the dense region is behind), or — adaptive — sized from the largest instances per parent any slice has shown so far, times 1.5.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

// parents of the first slice: the list cannot overflow when each has at most `ords` instances; env_knob (a TEST KNOB of include/vsrmc.h), when set, overrides
inline uint64_t slice_initial(uint64_t list_cap, int ords, const char* env_knob, bool* from_knob = nullptr) {
  uint64_t slice = std::max<uint64_t>(1, list_cap / (uint64_t)std::max(1, ords));
  const char* e = std::getenv(env_knob);
  if (e) slice = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
  if (from_knob) *from_knob = e != nullptr;
  return slice;
}

enum class SliceVerdict { Accept, Relist, Fail };

struct SlicePolicy {
  uint64_t pos, hi;                    // parents [pos, hi) have not been accepted yet
  uint64_t lo = 0, end = 0;            // the slice that next() handed out last
  uint64_t list_cap, bound;            // entries of the instance list; the most parents a slice may ever have
  uint64_t slice0, slice;
  bool adaptive;
  double ipp_max = 0;                  // adaptive: the largest instances per parent of any accepted slice
  uint64_t listings = 0, relisted = 0; // launches judged, the void ones among them

  SlicePolicy(uint64_t lo_, uint64_t hi_, uint64_t list_cap_, uint64_t first_slice, bool adaptive_ = false, uint64_t bound_ = ~(uint64_t)0)
      : pos(lo_), hi(hi_), list_cap(list_cap_), bound(bound_), slice0(std::max<uint64_t>(1, std::min(first_slice, bound_))), slice(slice0), adaptive(adaptive_) {}

  bool next() {                        // false: every parent is accepted
    if (pos >= hi) return false;
    lo = pos;
    end = std::min(hi, pos + slice);
    return true;
  }

  SliceVerdict judge(uint64_t n_instances) {   // what the listing of [lo, end) offered
    listings++;
    if (n_instances > list_cap) {
      if (end - lo == 1) return SliceVerdict::Fail;
      slice = std::max<uint64_t>(1, (end - lo) / 2);
      relisted++;
      return SliceVerdict::Relist;
    }
    if (adaptive) {
      ipp_max = std::max(ipp_max, (double)n_instances / (double)(end - lo));
      slice = std::max<uint64_t>(1, std::min(bound, (uint64_t)((double)list_cap / (ipp_max * 1.5 + 1.0))));
    } else {
      slice = std::min(slice0, slice * 2);
    }
    pos = end;
    return SliceVerdict::Accept;
  }
};
