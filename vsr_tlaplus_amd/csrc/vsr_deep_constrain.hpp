// vsr_deep_constrain.hpp — k_constrain_slice: the state constraint (vsr_constrain.hpp) on one scratch slice of a level beyond the record
// buffers (vsr_deep.hpp: every state of every seen-set-only level sits in a scratch buffer once per descent, before anything reads it).
// The shape and the preconditions of k_constrain: one lane per index of the slice, grid-stride over whole waves, refs[i] == 0 = a hole, where_run (the
// interpreter of vsr_where.hpp, not a copy) with the operand stack [slot][lane] in static LDS, lanes without a record run with valid = false, message
// loops run to the wave's largest bag.  A record whose constraint bit is clear gets refs[i] = 0 and fps[i] = 0, what k_constrain does to a stored level.
//
// What differs from k_constrain is where the figures go.  A descent launches this kernel once per slice, hundreds of times per level, and the host needs
// nothing from the filter of a regenerated slice (the slicer observes the index range and the words k_expand wrote, which the filter leaves alone): the
// counters of a launch — accumulated in registers over the grid-stride loop, reduced across the wave once, one atomic per counter and wave at the end —
// are ADDED to the level's own control block, which lives on the device for the whole descent, is reset once before it and read once after it.  The
// cursor of the pruned list lives in that block too, so the slices of a level append to one list.  list_cap == 0 (wave-uniform): a level whose figures were
// recorded by an earlier descent is filtered again — its pruned states come back with every regeneration — without a list and without the list's atomic.
// No scratch, no scalar memory writes.
#pragma once
#include "vsr_constrain.hpp"

namespace vsr {

#if defined(__HIPCC__)

template <int MODEL>
__global__ void __launch_bounds__(256)
k_constrain_slice(Model M, const u32* __restrict__ prog, int n_exports, int k_bit, const u64* __restrict__ words, u64* refs, u64* fps, u64 n, ConstrainCtl* ctl,
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
    const int wmax = wave_max_uniform(nmsg);
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
    refs[i] = 0;                                                   // out of model: withdrawn from the slice before the descent reads it
    fps[i] = 0;
    pruned++;
    pmin = fp < pmin ? fp : pmin;
#pragma unroll
    for (int p = 0; p < WHERE_MAX_EXPORTS; p++)
      if (p < n_exports && ((bits >> p) & 1)) { pcnt[p]++; pminf[p] = fp < pminf[p] ? fp : pminf[p]; }
    if (list_cap) {
      const u64 pos = wave_alloc(&ctl->n_list);
      if (pos < list_cap) list[pos] = fp;
    }
  }
  // the end of the launch: every lane of the wave is here (the loop above only `continue`s), one reduction and one atomic per counter and wave, into a
  // block that keeps the sums of the level's earlier slices
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
