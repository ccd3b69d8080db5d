// vsr_sim_where.hpp — k_simulate_where: simulation mode (k_simulate, vsr_kernels.hpp) with the user's own questions on every walk — a state program
// (vsr_where_parse.hpp) evaluated on every state a walker stands on, a step program on every (state, successor) pair it takes.  It reaches
// the depths the stored BFS levels never do: a walk has no seen-set and no frontier.  k_simulate itself is not touched and keeps its own entry point.
//
// Why a kernel of its own: where_run (vsr_where.hpp) reads its ops at a wave-uniform program counter and runs a message loop to the WAVE's largest bag,
// so the 64 lanes that call it must call it together.  k_simulate's lanes leave the loop one by one (break / continue).  Here a wave stays in LOCKSTEP:
// every lane runs every iteration, a lane with nothing to evaluate runs the interpreter with valid = false and its result is dropped (over zeros TRUE
// would count), the test that ends a launch early is a wave-wide ballot.  Guards, the draw, gen_ and the in-place apply are lane-private and may diverge;
// the two where_run calls, the wave reductions in front of them and the ballots behind them are reached by all 64 lanes.
//
// THE ITERATION CONTRACT (include/vsrmc.h states it for callers; tests/sim_where_model.py restates it in Python).  In one iteration a walker does one of
//   start   it has no walk yet, or its depth equals max_depth, or its state has no enabled instance: Init goes into its record, depth = 0, walks + 1.
//           The state program is evaluated on Init.  No random draw is taken.
//   step    one draw of sim_rng (xorshift64*); pick = draw % total over the enabled instances in ordinal order, as k_simulate; gen_<false>; the STEP
//           program on (record, Delta) through StepPair BEFORE the in-place apply; the apply; the STATE program on the record the walker now stands on;
//           the built-in invariants (Ops::invariants) as in k_simulate.
// Without a stop every walker evaluates exactly one state per iteration: states == steps + walks == iterations x walkers.
//
// Output per exported predicate k < 8, separately for the two programs: an exact count — wave ballots summed in registers, one atomic per wave at the end
// of the launch (k_where's contract).  stop != 0: the first walker with any bit set (or a violated built-in invariant) publishes its ordinals with a CAS
// on `found`, as k_simulate's violation does; kinds 3 (state predicate) and 4 (step predicate; the published walk INCLUDES the offending step) beside
// k_simulate's 1 (built-in invariant) and 2 (error).  An iteration that finds several reports the first in the order of the contract: step program, state
// program, built-in invariants.  stop == 0 counts only; the built-in invariants are not looked at; an evaluation error still ends the run (kind 2).
//
// The walker records are lane-private in HBM with stride fixed + max_bag words, as in k_simulate.  The operand stack is LDS, [slot][lane]:
// WHERE_MAX_DEPTH x 64 words per block of one wave.  HAS_STATE / HAS_STEP compile an absent program out.
#pragma once
#include "vsr_kernels.hpp"
#include "vsr_step.hpp"
#include "vsr_where.hpp"

namespace vsr {

#if defined(__HIPCC__)

enum { SIMW_BLOCK = 64 };

struct SimWhereCtl {
  u32 found;                          // 0 = walking, 1 built-in invariant, 2 error, 3 state predicate, 4 step predicate
  u32 viol_mask;                      // found 1: invariant bits; 2: 0x80000000 | error; 3 / 4: the predicate bits of the hit
  u32 viol_depth;                     // steps of the published walk
  u32 pad;
  u64 steps, walks;                   // steps taken / walks started by all walkers
  u64 n_states, n_pairs;              // evaluations of the state program / the step program
  u64 count_state[WHERE_MAX_EXPORTS]; // states that satisfy state predicate k
  u64 count_step[WHERE_MAX_EXPORTS];  // pairs that satisfy step predicate k
  u32 ords[512];                      // the published walk
};

struct SimWhereStack {                // [slot][lane of the block]
  int* base;
  __device__ __forceinline__ int& operator[](int slot) const { return base[slot * SIMW_BLOCK]; }
};

// cnt[k] += lanes with bit k; reached by the whole wave
__device__ __forceinline__ void simw_count(u32 bits, int n_exports, u32* cnt) {
  if (__ballot(bits != 0) == 0) return;                            // (wave-uniform)
#pragma unroll
  for (int k = 0; k < WHERE_MAX_EXPORTS; k++) {
    if (k >= n_exports) break;
    cnt[k] += (u32)__popcll(__ballot((bits >> k) & 1));
  }
}

template <int SPEC, bool HAS_STATE, bool HAS_STEP>
__global__ void __launch_bounds__(SIMW_BLOCK)
k_simulate_where(Model Marg, const u64* __restrict__ init_rec, int init_len, u64* walker_words, int stride, u32* walker_depth, u16* walker_ords,
                 u64* walker_rng, u32 n_walkers, int max_depth, int iters, const u32* __restrict__ state_prog, int n_state, const u32* __restrict__ step_prog,
                 int n_step, int stop, SimWhereCtl* ctl) {
  constexpr int MODEL = SPEC / 1000;
  typedef ModelOps<MODEL> Ops;
  __shared__ int stack[WHERE_MAX_DEPTH * SIMW_BLOCK];
  SimWhereStack S{stack + threadIdx.x};
  Model M = Marg;
  specialise<SPEC>(M, Marg);
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool mine = t < n_walkers;                                 // a lane past the last walker stays in the wave and never touches memory
  u64* w = walker_words + (u64)(mine ? t : 0) * stride;
  u16* my_ords = walker_ords + (u64)(mine ? t : 0) * max_depth;
  u64 rng = mine ? walker_rng[t] : 1;
  u32 depth = mine ? walker_depth[t] : 0xFFFFFFFFu;
  bool done = !mine;                                               // this lane published (or lost the CAS), or raised an error: it walks no further
  u32 cs[WHERE_MAX_EXPORTS], cp[WHERE_MAX_EXPORTS];                // wave-uniform (ballot popcounts); indexed by unrolled constants only
#pragma unroll
  for (int k = 0; k < WHERE_MAX_EXPORTS; k++) cs[k] = cp[k] = 0;
  u32 n_steps = 0, n_walks = 0, n_states = 0, n_pairs = 0;         // wave-uniform too
  // publish this lane's walk of `d` steps as the result of kind `kind`; the first walker wins, as in k_simulate
  auto publish = [&](u32 kind, u32 mask, u32 d) {
    if (atomicCAS(&ctl->found, 0u, kind) == 0u) {
      ctl->viol_mask = mask;
      ctl->viol_depth = d;
      for (u32 k = 0; k < d && k < 512; k++) ctl->ords[k] = my_ords[k];
    }
    done = true;
  };
  for (int it = 0; it < iters; it++) {
    const u32 seen = __hip_atomic_load(&ctl->found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__ballot(seen != 0 || (done && mine)) != 0) break;         // (wave-uniform) some walker anywhere has ended the run
    // ---- start or step?  (lane-private: the guards of this lane's record)
    bool start = mine && (depth == 0xFFFFFFFFu || depth >= (u32)max_depth);
    int total = 0, nslots = 0;
    if (mine && !start) {
      nslots = M.m0 + hdr_nmsg(w[0]);
      for (int slot = 0; slot < nslots; slot++) {
        int kind0;
        total += __builtin_popcount(Ops::guard(M, (const u64*)w, slot, &kind0));
      }
      start = total == 0;                                          // terminal state: the walk ends (TLC -deadlock), the next one starts now
    }
    bool step = mine && !start;
    Delta D = Delta();
    int ord = -1;
    if (step) {
      int pick = (int)(sim_rng(&rng) % (u64)total);
      for (int slot = 0; slot < nslots && ord < 0; slot++) {
        int kind0;
        u32 mask = Ops::guard(M, (const u64*)w, slot, &kind0);
        const int c = __builtin_popcount(mask);
        if (pick >= c) { pick -= c; continue; }
        while (pick--) mask &= mask - 1;
        const int k = __ffs((int)mask) - 1;
        ord = slot < M.m0 ? slot : M.m0 + (slot - M.m0) * (M.R + 1) + k;
      }
      if (ord < 0 || !Ops::template gen_<false>(M, (const u64*)w, ord, D)) {
        publish(2u, 0x80000000u | (u32)ERR_INTERNAL, depth);
        step = false;
      } else if (D.err) {                                          // evaluation / representation error: reported like k_simulate's
        publish(2u, 0x80000000u | (u32)D.err, depth);
        step = false;
      }
    }
    // ---- the step program on (record, Delta), before the apply.  The whole wave is here.
    u32 sbits = 0;
    if constexpr (HAS_STEP) {
      const int nmsg_p = step ? hdr_nmsg(w[0]) : 0, nmsg_c = step ? hdr_nmsg(D.hdr) : 0;
      const int wmax = wave_max_uniform(max(nmsg_p, nmsg_c));
      const StepPair<MODEL> pair{(const u64*)w, D, M.fixed, 1 + ((int)D.r - 1) * M.wpr, M.wpr, nmsg_p, nmsg_c, (int)D.action};
      const u32 raw = where_run<SimWhereStack, const u64*, StepPair<MODEL>, MODEL>(step_prog, M.fixed, (const u64*)w, step, nmsg_p, wmax, S, pair);
      sbits = step ? raw : 0;                                      // (a lane without a pair ran the program over zeros: TRUE would count it)
      n_pairs += (u32)__popcll(__ballot(step));
      simw_count(sbits, n_step, cp);
    }
    // ---- the built-in invariants (of the successor, from the record and the Delta), then the apply in place
    int bad = 0;
    if (step) {
      if (stop) bad = Ops::invariants(M, (const u64*)w, D);
      const int plen = M.fixed + hdr_nmsg(w[0]);
      w[0] = D.hdr;
      u64* pb = w + 1 + (D.r - 1) * M.wpr;
      pb[0] = D.rep[0];
      if (M.wpr > 1) pb[1] = D.rep[1];
      if (M.wpr > 2) pb[2] = D.rep[2];
      if (M.wpr > 3) pb[3] = D.rep[3];
      int a = 0;
#pragma unroll
      for (int k = 0; k < VSR_NSLOT; k++)
        if ((D.used >> k) & 1) {
          if (D.pj(k) >= 0) w[M.fixed + D.pj(k)] = D.pnew[k];
          else w[plen + (a++)] = D.pnew[k];
        }
      my_ords[depth] = (u16)ord;
      depth++;
    } else if (start) {
      for (int k = 0; k < init_len; k++) w[k] = init_rec[k];
      depth = 0;
    }
    n_steps += (u32)__popcll(__ballot(step));
    n_walks += (u32)__popcll(__ballot(start));
    // ---- the state program on the record the walker now stands on.  The whole wave is here.
    const bool stands = step || start;
    u32 wbits = 0;
    if constexpr (HAS_STATE) {
      const int nmsg = stands ? hdr_nmsg(w[0]) : 0;
      const int wmax = wave_max_uniform(nmsg);
      const u32 raw = where_run<SimWhereStack, const u64*, WhereNoPair, MODEL>(state_prog, M.fixed, (const u64*)w, stands, nmsg, wmax, S);
      wbits = stands ? raw : 0;                                    // (a lane without a state ran the program over zeros: TRUE would count it)
      n_states += (u32)__popcll(__ballot(stands));
      simw_count(wbits, n_state, cs);
    }
    if (stop && stands) {                                          // (lane-private) in the order of the contract
      if (sbits) publish(4u, sbits, depth);
      else if (wbits) publish(3u, wbits, depth);
      else if (bad) publish(1u, (u32)bad, depth);
    }
  }
  if (mine) {
    walker_rng[t] = rng;
    walker_depth[t] = depth;
  }
  if (lane_id() == 0) {                                            // one atomic per counter and wave
    if (n_steps) atomicAdd((unsigned long long*)&ctl->steps, (unsigned long long)n_steps);
    if (n_walks) atomicAdd((unsigned long long*)&ctl->walks, (unsigned long long)n_walks);
    if (n_states) atomicAdd((unsigned long long*)&ctl->n_states, (unsigned long long)n_states);
    if (n_pairs) atomicAdd((unsigned long long*)&ctl->n_pairs, (unsigned long long)n_pairs);
#pragma unroll
    for (int k = 0; k < WHERE_MAX_EXPORTS; k++) {
      if (cs[k]) atomicAdd((unsigned long long*)&ctl->count_state[k], (unsigned long long)cs[k]);
      if (cp[k]) atomicAdd((unsigned long long*)&ctl->count_step[k], (unsigned long long)cp[k]);
    }
  }
}

#endif  // __HIPCC__

}  // namespace vsr
