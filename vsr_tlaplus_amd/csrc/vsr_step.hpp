// vsr_step.hpp — step predicates: user-written predicates over a state AND its successor (primed variables, UNCHANGED, step_action; compiled by
// vsr_where_parse.hpp's step entry) evaluated on every transition out of the records of a level (§9e for the two analysis models).  One
// instantiation of each kernel per model, as k_where<MODEL>: <0> is VSR.tla's and compiles what it compiled before.
//
// The interpreter (where_run, vsr_where.hpp) needs a wave-uniform program counter and wants its lanes busy.  A record has M.m0 + nmsg * (R + 1) ordinals
// of which a handful are enabled, so a lane-per-parent loop over ordinals would run the program with most lanes idle.  Two kernels instead, run by the
// host over slices of the level (host_step.hpp):
//
//   k_step_list   one lane per parent record (refs[i] == 0 = a hole): guards only — ModelOps<MODEL>::guard_pre, the statement k_terminal and k_expand's
//                 enumeration use — and every enabled instance appended as parent index | ordinal << 40 to a global list, wave-aggregated (one atomic per wave and
//                 round: wave_alloc).  The wave walks the slots together, so that the lanes that have an instance in a round allocate together.
//   k_step_apply  one lane per list entry: ModelOps<MODEL>::gen_<false> on the parent gives the Delta; an entry whose action raises an evaluation error (D.err) is counted
//                 and not evaluated.  The program then runs over a PAIR VIEW of (parent record, Delta) — no child record is written anywhere:
//                   word w of the child   = D.hdr for w = 0, D.rep[w - base] inside the block of replica D.r (w - base < wpr: a block of the analysis
//                                           models has one or two words, and the word after it is the NEXT replica's), the parent's word otherwise;
//                   bag entry j of the child = for j < the parent's nmsg the parent's entry, replaced by D.pnew[s] where patch slot s names j;
//                                           beyond that the appended slots in slot order (the order write_child_serial writes them).
//                 D.rep and D.pnew are picked by unrolled selects, never by a run-time subscript, so that the Delta stays in registers.  The operand stack
//                 is in LDS as [slot][lane], as in k_where.  A message loop runs to the wave's largest bag, parent's or child's.
//
// Output per exported predicate k < 8 (the contract of k_where, over pairs): an exact count (ballots summed per wave, one atomic per wave at the end), the
// smallest PARENT fingerprint among the pairs that satisfy it (one atomicMin per wave with a hit), and for pairs with any bit set a
// (parent fingerprint, parent index, ordinal, bits) quadruple appended wave-wise to a list of which the first hit_cap that arrive are kept
// (StepCtl::n_hits = the true number).  `rows`, when given (a caller's batch), receives action | bits << 8 | err << 16 per list entry.
#pragma once
#include "vsr_kernels.hpp"
#include "vsr_where.hpp"

namespace vsr {

// the successor as where_run sees it: the parent record and the Delta of one instance (host-callable like where_run itself)
template <int MODEL>
struct StepPair {
  static constexpr bool is_pair = true;
  const u64* rec;
  const Delta& D;
  int fixed, rbase, wpr, nmsg_p, nmsg_c, action;
  VSR_HD u64 word(int w) const {
    const int k = w - rbase;
    u64 v = rec[w];
    // every substitution needs k < wpr; VSR.tla's blocks have 3 or 4 words, so its first three need no test
    v = k == 0 ? D.rep[0] : (k == 1 && (MODEL == 0 || wpr > 1)) ? D.rep[1] : (k == 2 && (MODEL == 0 || wpr > 2)) ? D.rep[2] : (k == 3 && wpr > 3) ? D.rep[3] : v;
    return w == 0 ? D.hdr : v;
  }
  VSR_HD u64 msg(int j) const {
    u64 v = j < nmsg_p ? rec[fixed + j] : (u64)0;
    const int a = j - nmsg_p;                                      // which appended entry (negative: none)
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < VSR_NSLOT; s++) {
      const bool used = (D.used >> s) & 1;
      const int pj = D.pj(s);
      const bool take = used && (pj >= 0 ? pj == j : cnt == a);
      v = take ? D.pnew[s] : v;
      cnt += (used && pj < 0) ? 1 : 0;
    }
    return v;
  }
};

#if defined(__HIPCC__)

struct StepCtl {
  u64 n_list;                         // instances offered to the list by k_step_list since the host last cleared it (one slice)
  u64 scanned;                        // parent records looked at (holes excluded)
  u64 n_pairs, n_err, n_internal;     // pairs evaluated; instances whose action raises an evaluation error; listed instances gen<false> calls disabled (never)
  u64 count[WHERE_MAX_EXPORTS];       // pairs that satisfy predicate k
  u64 min_fp[WHERE_MAX_EXPORTS];      // the smallest parent fingerprint among them, ~0 = none
  u64 n_hits;                         // pairs with any bit set offered to the hit list
};

template <int MODEL>
__global__ void __launch_bounds__(256)
k_step_list(Model M, const u64* __restrict__ words, const u64* __restrict__ refs, u64 lo, u64 hi, u64* list, u64 list_cap, StepCtl* ctl) {
  u32 n_scanned = 0;
  const u64 n = hi - lo;
  const u64 step = (u64)gridDim.x * blockDim.x;
  const u64 n_round = (n + 63) & ~(u64)63;                         // whole waves stay together
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += step) {
    const u64 pidx = lo + i;
    const u64 ref = i < n ? refs[pidx] : 0;
    const bool valid = ref != 0;
    const u64* rec = words + (ref >> 8);
    n_scanned += (u32)__popcll(__ballot(valid));
    u64 hdr = 0;
    u64 Areg[6] = {0, 0, 0, 0, 0, 0};
    if (valid) {
      hdr = rec[0];
#pragma unroll
      for (int r = 1; r <= 5; r++)
        if (r <= M.R) Areg[r] = rec[1 + (r - 1) * M.wpr];
    }
    const int nslots = valid ? M.m0 + hdr_nmsg(hdr) : 0;
    const int wslots = wave_max_uniform(nslots);
    for (int slot = 0; slot < wslots; slot++) {
      int kind0 = 0;
      u32 mask = slot < nslots ? ModelOps<MODEL>::guard_pre(M, rec, hdr, Areg, slot, &kind0, -1) : 0u;
      while (__ballot(mask != 0) != 0) {                           // (wave-uniform) bit k of a message slot: k = 0 the receive, k = d SendGetState(r, d, m) (AnyDest: replica d receives)
        if (mask != 0) {
          const int k = __ffs((int)mask) - 1;
          mask &= mask - 1;
          const int ord = slot < M.m0 ? slot : M.m0 + (slot - M.m0) * (M.R + 1) + k;
          const u64 pos = wave_alloc(&ctl->n_list);
          if (pos < list_cap) list[pos] = origin_make(pidx, ord);
        }
      }
    }
  }
  if (lane_id() == 0 && n_scanned) atomicAdd((unsigned long long*)&ctl->scanned, (unsigned long long)n_scanned);
}

template <int MODEL>
__global__ void __launch_bounds__(256)
k_step_apply(Model M, const u32* __restrict__ prog, int n_exports, const u64* __restrict__ words, const u64* __restrict__ refs, const u64* __restrict__ fps,
             const u64* __restrict__ list, u64 n_entries, StepCtl* ctl, u64* hits, u64 hit_cap, u32* rows) {
  __shared__ int stack[WHERE_MAX_DEPTH * 256];
  WhereLdsStack S{stack + threadIdx.x};
  u32 cnt[WHERE_MAX_EXPORTS];                                      // wave-uniform (ballot popcounts); indexed by unrolled constants only
#pragma unroll
  for (int k = 0; k < WHERE_MAX_EXPORTS; k++) cnt[k] = 0;
  u32 n_pairs = 0, n_err = 0, n_internal = 0;
  const u64 step = (u64)gridDim.x * blockDim.x;
  const u64 n_round = (n_entries + 63) & ~(u64)63;                 // whole waves stay together
  for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < n_round; e += step) {
    const bool have = e < n_entries;
    const u64 entry = have ? list[e] : 0;
    const u64 pidx = origin_pidx(entry);
    const int ord = origin_ord(entry);
    const u64 ref = have ? refs[pidx] : 0;
    const u64* rec = words + (ref >> 8);
    Delta D = Delta();
    bool enabled = false;
    if (have) enabled = ModelOps<MODEL>::template gen_<false>(M, rec, ord, D);
    const bool err = have && enabled && D.err != 0;
    const bool valid = have && enabled && D.err == 0;
    const int nmsg_p = valid ? hdr_nmsg(rec[0]) : 0, nmsg_c = valid ? hdr_nmsg(D.hdr) : 0;
    // (wave_max_uniform written out: through the helper this kernel compiles to one v_xor fewer, and the change that introduced the helper left every
    // kernel's code as it was)
    int wmax = max(nmsg_p, nmsg_c);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wmax = max(wmax, __shfl_xor(wmax, d));
    wmax = (int)VSR_WHERE_UNI(wmax);
    const StepPair<MODEL> pair{rec, D, M.fixed, 1 + ((int)D.r - 1) * M.wpr, M.wpr, nmsg_p, nmsg_c, (int)D.action};
    const u32 raw = where_run<WhereLdsStack, const u64*, StepPair<MODEL>, MODEL>(prog, M.fixed, rec, valid, nmsg_p, wmax, S, pair);
    const u32 bits = valid ? raw : 0;                              // (a lane without a pair ran the program over zeros: TRUE would count it)
    if (rows && have) rows[e] = (u32)D.action | (bits << 8) | ((u32)(D.err & 0xFF) << 16) | (enabled ? 0u : 1u << 31);
    n_pairs += (u32)__popcll(__ballot(valid));
    n_err += (u32)__popcll(__ballot(err));
    n_internal += (u32)__popcll(__ballot(have && !enabled));
    if (__ballot(bits != 0) == 0) continue;                        // (wave-uniform)
    const u64 fp = (fps && have) ? fps[pidx] : ~(u64)0;
#pragma unroll
    for (int k = 0; k < WHERE_MAX_EXPORTS; k++) {
      if (k >= n_exports) break;
      const bool hit = (bits >> k) & 1;
      const u64 b = __ballot(hit);
      if (b == 0) continue;
      cnt[k] += (u32)__popcll(b);
      if (fps) {
        const u64 m = wave_min64(hit ? fp : ~(u64)0);
        if (lane_id() == 0) atomicMin((unsigned long long*)&ctl->min_fp[k], (unsigned long long)m);
      }
    }
    if (fps && hits && bits != 0) {
      const u64 k = wave_alloc(&ctl->n_hits);
      if (k < hit_cap) {
        hits[4 * k] = fp;
        hits[4 * k + 1] = pidx;
        hits[4 * k + 2] = (u64)ord;
        hits[4 * k + 3] = (u64)bits;
      }
    }
  }
  if (lane_id() == 0) {                                            // one atomic per counter and wave
    if (n_pairs) atomicAdd((unsigned long long*)&ctl->n_pairs, (unsigned long long)n_pairs);
    if (n_err) atomicAdd((unsigned long long*)&ctl->n_err, (unsigned long long)n_err);
    if (n_internal) atomicAdd((unsigned long long*)&ctl->n_internal, (unsigned long long)n_internal);
#pragma unroll
    for (int k = 0; k < WHERE_MAX_EXPORTS; k++)
      if (cnt[k]) atomicAdd((unsigned long long*)&ctl->count[k], (unsigned long long)cnt[k]);
  }
}

#endif  // __HIPCC__

}  // namespace vsr
