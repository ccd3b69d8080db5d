// vsr_constrain.hpp — k_constrain: a state constraint (TLC's CONSTRAINT: one exported predicate of a program vsr_where_parse.hpp compiled) applied to the
// newest stored level right after it was written.  The shape and the preconditions of k_where (vsr_where.hpp): one lane per index of the level, grid-stride
// over whole waves, refs[i] == 0 = a hole, where_run with the operand stack [slot][lane] in LDS, lanes without a record run with valid = false, message
// loops run to the wave's largest bag.  Nothing is applied, the seen-set is not touched, k_expand is not involved.
//
// Bit k of the program's result is the constraint.  A record where it is clear is OUT OF MODEL: the lane zeroes refs[i] and fps[i] — what k_partition does
// to the states another rank owns; every consumer of a level skips such an index.  The state keeps its slot in the seen-set: membership
// is a function of the state, it can never come back as an in-model state, and with its ref gone it is never a parent.
//
// Everything else is accumulated in registers of the lane over the whole grid-stride loop, reduced across the wave once at the end of the launch and
// flushed with one atomic per counter and wave (no hot global counter):
//   kept     count, record words, largest bag, xor and sum of the fingerprints (the figures of k_level_checksum and of the oracle fixtures)
//   pruned   count, smallest fingerprint; for every exported predicate p of the program the count and the smallest fingerprint among the PRUNED states
//            with bit p set (where_run returns all bits at once: a user's invariant is not lost on the states the search does not keep)
// and the fingerprints of the pruned states are appended wave-wise (wave_alloc: one atomic per wave and trip that prunes) to a list of which the first
// list_cap that arrive are kept (ConstrainCtl::n_list = the true number).  No scratch, no scalar memory writes.
#pragma once
#include "vsr_where.hpp"

namespace vsr {

#if defined(__HIPCC__)

struct ConstrainCtl {
  u64 kept, kept_words, kept_max_bag, kept_xor, kept_sum;
  u64 pruned, pruned_min_fp;          // ~0 = none
  u64 p_count[WHERE_MAX_EXPORTS];     // pruned states with bit p set
  u64 p_min_fp[WHERE_MAX_EXPORTS];    // the smallest fingerprint among them, ~0 = none
  u64 n_list;                         // pruned states offered to the list
};

template <int MODEL>
__global__ void __launch_bounds__(256)
k_constrain(Model M, const u32* __restrict__ prog, int n_exports, int k_bit, const u64* __restrict__ words, u64* refs, u64* fps, u64 n, ConstrainCtl* ctl,
            u64* list, u64 list_cap) {
  __shared__ int stack[WHERE_MAX_DEPTH * 256];
  WhereLdsStack S{stack + threadIdx.x};
  u32 kept = 0, pruned = 0, bag = 0;                                // per lane, reduced at the end
  u64 kwords = 0, kxor = 0, ksum = 0, pmin = ~(u64)0;
  u32 pcnt[WHERE_MAX_EXPORTS];                                     // indexed by unrolled constants only
  u64 pminf[WHERE_MAX_EXPORTS];
#pragma unroll
  for (int p = 0; p < WHERE_MAX_EXPORTS; p++) { pcnt[p] = 0; pminf[p] = ~(u64)0; }
  const u64 step = (u64)gridDim.x * blockDim.x;
  const u64 n_round = (n + 63) & ~(u64)63;                         // whole waves stay together
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += step) {
    const u64 ref = i < n ? refs[i] : 0;
    const bool valid = ref != 0;
    const u64* rec = words + (ref >> 8);
    const int nmsg = valid ? hdr_nmsg(rec[0]) : 0;
    // (wave_max_uniform written out: through the helper this kernel compiles to one v_xor fewer, and the change that introduced the helper left every
    // kernel's code as it was)
    int wmax = nmsg;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wmax = max(wmax, __shfl_xor(wmax, d));
    wmax = (int)VSR_WHERE_UNI(wmax);
    const u32 bits = where_run<WhereLdsStack, const u64*, WhereNoPair, MODEL>(prog, M.fixed, rec, valid, nmsg, wmax, S);
    if (!valid) continue;                                          // (a lane without a record ran the program over zeros; nothing below crosses lanes but wave_alloc)
    const u64 fp = fps[i];
    if ((bits >> k_bit) & 1) {
      kept++;
      kwords += ref & 0xFF;
      bag = max(bag, (u32)nmsg);
      kxor ^= fp;
      ksum += fp;
      continue;
    }
    refs[i] = 0;                                                   // out of model: withdrawn from the level
    fps[i] = 0;
    pruned++;
    pmin = fp < pmin ? fp : pmin;
#pragma unroll
    for (int p = 0; p < WHERE_MAX_EXPORTS; p++)
      if (p < n_exports && ((bits >> p) & 1)) { pcnt[p]++; pminf[p] = fp < pminf[p] ? fp : pminf[p]; }
    const u64 pos = wave_alloc(&ctl->n_list);
    if (pos < list_cap) list[pos] = fp;
  }
  // the end of the launch: every lane of the wave is here (the loop above only `continue`s), one reduction and one atomic per counter and wave
  const u64 w_kept = wave_sum64(kept), w_pruned = wave_sum64(pruned);
  if (w_kept) {
    const u64 w_words = wave_sum64(kwords), w_bag = wave_max64(bag), w_xor = wave_xor64(kxor), w_sum = wave_sum64(ksum);
    if (lane_id() == 0) {
      atomicAdd((unsigned long long*)&ctl->kept, (unsigned long long)w_kept);
      atomicAdd((unsigned long long*)&ctl->kept_words, (unsigned long long)w_words);
      atomicMax((unsigned long long*)&ctl->kept_max_bag, (unsigned long long)w_bag);
      if (w_xor) atomicXor((unsigned long long*)&ctl->kept_xor, (unsigned long long)w_xor);
      if (w_sum) atomicAdd((unsigned long long*)&ctl->kept_sum, (unsigned long long)w_sum);
    }
  }
  if (w_pruned) {                                                  // (wave-uniform)
    const u64 w_min = wave_min64(pmin);
    if (lane_id() == 0) {
      atomicAdd((unsigned long long*)&ctl->pruned, (unsigned long long)w_pruned);
      atomicMin((unsigned long long*)&ctl->pruned_min_fp, (unsigned long long)w_min);
    }
#pragma unroll
    for (int p = 0; p < WHERE_MAX_EXPORTS; p++) {
      if (p >= n_exports) break;
      const u64 w_c = wave_sum64(pcnt[p]);
      if (w_c == 0) continue;
      const u64 w_m = wave_min64(pminf[p]);
      if (lane_id() == 0) {
        atomicAdd((unsigned long long*)&ctl->p_count[p], (unsigned long long)w_c);
        atomicMin((unsigned long long*)&ctl->p_min_fp[p], (unsigned long long)w_m);
      }
    }
  }
}

#endif  // __HIPCC__

}  // namespace vsr
