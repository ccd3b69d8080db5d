// vsr_sim_constrain.hpp — k_simulate_constrained: random walks under a state constraint (TLC's CONSTRAINT, §9h) and / or an action constraint
// (ACTION_CONSTRAINT, §9i), with the user's queries on every walk as in k_simulate_where (vsr_sim_where.hpp, which it leaves alone).  DESIGN.md §9j.
// A walk moves only along PERMITTED transitions into IN-MODEL states; the stored BFS levels are the only other place the two constraints apply, and
// they end where the record buffers do.  [TLC-RECALLED]: the semantics are TLC's simulator's as recalled, nothing here is pinned against a TLC run.
//
// The shape is k_simulate_where's: blocks of one wave in LOCKSTEP — every lane runs every iteration, the two where_run calls, the wave reductions in
// front of them and the ballots behind them are reached by all 64 lanes, a lane with nothing to evaluate runs the interpreter with valid = false and
// its result is dropped; operand stack in LDS [slot][lane]; walker records lane-private in HBM; HAS_STATE / HAS_STEP compile an absent program out.
//
// The state program exports the queries and, at index state_con (or -1), the state constraint; the step program likewise with step_con.  The
// constraint exports are counted like every export and never stop a run.
//
// THE TRIED SET (sim_tried.hpp).  Choosing uniformly among the permitted-and-in-model successors needs their number, which only evaluating every
// instance gives.  Instead a walker draws among the instances it has not been refused yet: a bitmask over the enabled instances of the state it stands
// on, by position in ordinal order, cleared when it moves or starts, kept across launches.  Sampling without replacement up to the first acceptance is
// uniform over the acceptable ones, and a state is left, or found terminal in the constrained model, after at most `total` iterations.
//
// THE ITERATION CONTRACT (include/vsrmc.h states it for callers; tests/sim_constrained_model.py restates it in Python).  In one iteration a walker does
//   start    it has no walk yet, or depth == max_depth, or its state has no enabled instance, or every enabled instance has been tried (`stuck` + 1:
//            terminal in the constrained model): Init into the record, tried set cleared, walks + 1; the state program on Init, its bits counted.  No draw.
//   try      one draw of sim_rng; pick = draw % (total - |tried|) over the UNTRIED enabled instances in ordinal order; gen_<false>; the STEP program on
//            (record, Delta) before any move.  Then one of
//   blocked  the step_con bit is false: the instance is marked tried, blocked + 1, nothing else is evaluated, the walker stays.
//   (move)   the in-place apply, the overwritten words kept in registers — header, replica block (<= 4 words), the <= VSR_NSLOT patched bag words;
//            appended words need no log: the restored header's nmsg drops them.  The STATE program on the new record.  Then one of
//   pruned   the state_con bit is false: the record is restored from the undo log, the instance is marked tried, pruned + 1, depth unchanged, the step
//            query bits are dropped.  stop: the state bits in pruned_stop_mask (kind 3), then the built-in invariants of that successor (kind 1) publish
//            the walk INCLUDING the step into the pruned state — the BFS checks invariants on pruned states too (§9h).
//   step     the move stands: steps, n_pairs, n_states + 1, the bits of both programs counted, tried set cleared.  stop: step query (4), state query (3),
//            built-in invariants (1), in this order.
// Without a stop: steps + walks + blocked + pruned == iterations x walkers; n_states == steps + walks; n_pairs == steps.
// A state with more than SIM_TRIED_BITS enabled instances ends the run: found = 2, error ERR_SIM_TRIED_WIDTH.
#pragma once
#include "vsr_kernels.hpp"
#include "vsr_step.hpp"
#include "vsr_where.hpp"
#include "vsr_sim_where.hpp"
#if defined(__HIPCC__)
#define SIM_TRIED_FN __host__ __device__ __forceinline__
#endif
#include "sim_tried.hpp"

namespace vsr {

enum { ERR_SIM_TRIED_WIDTH = 40 };    // VSRMC_SIM_ERR_TRIED_WIDTH of include/vsrmc.h

#if defined(__HIPCC__)

struct SimConCtl {
  u32 found;                          // 0 = walking, 1 built-in invariant, 2 error, 3 state predicate, 4 step predicate
  u32 viol_mask;                      // found 1: invariant bits; 2: 0x80000000 | error; 3 / 4: the predicate bits of the hit
  u32 viol_depth;                     // steps of the published walk
  u32 pad;
  u64 steps, walks;                   // moves that stand / walks started by all walkers
  u64 n_states, n_pairs;              // states stood on / pairs taken (each evaluated by the program that is present)
  u64 blocked, pruned, stuck;         // tries the action constraint refused / the state constraint refused; starts out of a state with every instance tried
  u64 count_state[WHERE_MAX_EXPORTS]; // states stood on that satisfy state predicate k
  u64 count_step[WHERE_MAX_EXPORTS];  // pairs taken that satisfy step predicate k
  u32 ords[512];                      // the published walk
};

template <int SPEC, bool HAS_STATE, bool HAS_STEP>
__global__ void __launch_bounds__(SIMW_BLOCK)
k_simulate_constrained(Model Marg, const u64* __restrict__ init_rec, int init_len, u64* walker_words, int stride, u32* walker_depth, u16* walker_ords,
                       u64* walker_rng, u64* walker_tried, u32 n_walkers, int max_depth, int iters, const u32* __restrict__ state_prog, int n_state,
                       int state_con, const u32* __restrict__ step_prog, int n_step, int step_con, u32 pruned_stop_mask, int stop, SimConCtl* ctl) {
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
  u64* const my_tried = walker_tried + (u64)(mine ? t : 0) * SIM_TRIED_WORDS;
  TriedSet tried;
  tried.w0 = mine ? my_tried[0] : 0;
  tried.w1 = mine ? my_tried[1] : 0;
  tried.w2 = mine ? my_tried[2] : 0;
  tried.w3 = mine ? my_tried[3] : 0;
  bool done = !mine;                                               // this lane published (or lost the CAS), or raised an error: it walks no further
  const u32 state_con_bit = (HAS_STATE && state_con >= 0) ? 1u << state_con : 0u;
  const u32 step_con_bit = (HAS_STEP && step_con >= 0) ? 1u << step_con : 0u;
  u32 cs[WHERE_MAX_EXPORTS], cp[WHERE_MAX_EXPORTS];                // wave-uniform (ballot popcounts); indexed by unrolled constants only
#pragma unroll
  for (int k = 0; k < WHERE_MAX_EXPORTS; k++) cs[k] = cp[k] = 0;
  u32 n_steps = 0, n_walks = 0, n_states = 0, n_pairs = 0, n_blocked = 0, n_pruned = 0, n_stuck = 0;   // wave-uniform too
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
    // ---- start or try?  (lane-private: the guards of this lane's record and its tried set)
    bool start = mine && (depth == 0xFFFFFFFFu || depth >= (u32)max_depth);
    bool stuck = false, attempt = false;
    int total = 0, nslots = 0;
    if (mine && !start) {
      nslots = M.m0 + hdr_nmsg(w[0]);
      for (int slot = 0; slot < nslots; slot++) {
        int kind0;
        total += __builtin_popcount(Ops::guard(M, (const u64*)w, slot, &kind0));
      }
      if (!tried_fits(total)) publish(2u, 0x80000000u | (u32)ERR_SIM_TRIED_WIDTH, depth);
      else {
        stuck = total != 0 && tried_all(tried, total);             // terminal in the constrained model
        start = total == 0 || stuck;                               // (total == 0: terminal, as in k_simulate_where)
        attempt = !start;
      }
    }
    Delta D = Delta();
    int ord = -1, pos = -1;
    if (attempt) {
      pos = tried_pick(tried, total, (int)(sim_rng(&rng) % (u64)(total - tried_count(tried))));
      int pick = pos;
      for (int slot = 0; slot < nslots && ord < 0 && pick >= 0; slot++) {
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
        attempt = false;
      } else if (D.err) {                                          // evaluation / representation error: reported like k_simulate's
        publish(2u, 0x80000000u | (u32)D.err, depth);
        attempt = false;
      }
    }
    // ---- the step program on (record, Delta), before any move.  The whole wave is here.
    u32 sbits = 0;
    if constexpr (HAS_STEP) {
      const int nmsg_p = attempt ? hdr_nmsg(w[0]) : 0, nmsg_c = attempt ? hdr_nmsg(D.hdr) : 0;
      const int wmax = wave_max_uniform(max(nmsg_p, nmsg_c));
      const StepPair<MODEL> pair{(const u64*)w, D, M.fixed, 1 + ((int)D.r - 1) * M.wpr, M.wpr, nmsg_p, nmsg_c, (int)D.action};
      const u32 raw = where_run<SimWhereStack, const u64*, StepPair<MODEL>, MODEL>(step_prog, M.fixed, (const u64*)w, attempt, nmsg_p, wmax, S, pair);
      sbits = attempt ? raw : 0;                                   // (a lane without a pair ran the program over zeros: TRUE would count it)
    }
    const bool blocked = attempt && step_con_bit != 0 && (sbits & step_con_bit) == 0;
    const bool move = attempt && !blocked;
    // ---- the built-in invariants (of the successor, from the record and the Delta), then the apply in place with its undo log
    int bad = 0;
    u64 u_hdr = 0, u_rep0 = 0, u_rep1 = 0, u_rep2 = 0, u_rep3 = 0, u_bag[VSR_NSLOT];
#pragma unroll
    for (int k = 0; k < VSR_NSLOT; k++) u_bag[k] = 0;
    u64* const pb = w + 1 + (move ? (int)D.r - 1 : 0) * M.wpr;
    if (move) {
      if (stop) bad = Ops::invariants(M, (const u64*)w, D);
      const int plen = M.fixed + hdr_nmsg(w[0]);
      u_hdr = w[0];
      w[0] = D.hdr;
      u_rep0 = pb[0];
      pb[0] = D.rep[0];
      if (M.wpr > 1) { u_rep1 = pb[1]; pb[1] = D.rep[1]; }
      if (M.wpr > 2) { u_rep2 = pb[2]; pb[2] = D.rep[2]; }
      if (M.wpr > 3) { u_rep3 = pb[3]; pb[3] = D.rep[3]; }
      int a = 0;
#pragma unroll
      for (int k = 0; k < VSR_NSLOT; k++)
        if ((D.used >> k) & 1) {
          if (D.pj(k) >= 0) { u_bag[k] = w[M.fixed + D.pj(k)]; w[M.fixed + D.pj(k)] = D.pnew[k]; }
          else w[plen + (a++)] = D.pnew[k];
        }
    } else if (start) {
      for (int k = 0; k < init_len; k++) w[k] = init_rec[k];
      depth = 0;
      tried_clear(tried);
    }
    // ---- the state program on the record the walker now stands on, or has moved into on trial.  The whole wave is here.
    const bool looks = move || start;
    u32 wbits = 0;
    if constexpr (HAS_STATE) {
      const int nmsg = looks ? hdr_nmsg(w[0]) : 0;
      const int wmax = wave_max_uniform(nmsg);
      const u32 raw = where_run<SimWhereStack, const u64*, WhereNoPair, MODEL>(state_prog, M.fixed, (const u64*)w, looks, nmsg, wmax, S);
      wbits = looks ? raw : 0;                                     // (a lane without a state ran the program over zeros: TRUE would count it)
    }
    const bool pruned = move && state_con_bit != 0 && (wbits & state_con_bit) == 0;
    const bool step = move && !pruned;
    if (pruned) {                                                  // (lane-private)
      if (stop) {
        my_ords[depth] = (u16)ord;                                 // depth < max_depth here: the published walk includes the step into the pruned state
        if (wbits & pruned_stop_mask) publish(3u, wbits & pruned_stop_mask, depth + 1);
        else if (bad) publish(1u, (u32)bad, depth + 1);
      }
      // undo: the patched bag words in reverse order (two slots may patch one word), the replica block, the header — its nmsg drops the appended words
#pragma unroll
      for (int k = VSR_NSLOT - 1; k >= 0; k--)
        if (((D.used >> k) & 1) && D.pj(k) >= 0) w[M.fixed + D.pj(k)] = u_bag[k];
      pb[0] = u_rep0;
      if (M.wpr > 1) pb[1] = u_rep1;
      if (M.wpr > 2) pb[2] = u_rep2;
      if (M.wpr > 3) pb[3] = u_rep3;
      w[0] = u_hdr;
    }
    if (blocked || pruned) tried_mark(tried, pos);
    if (step) {
      my_ords[depth] = (u16)ord;
      depth++;
      tried_clear(tried);
    }
    // ---- the counters: wave ballots.  The whole wave is here.
    const bool stands = step || start;
    n_steps += (u32)__popcll(__ballot(step));
    n_walks += (u32)__popcll(__ballot(start));
    n_blocked += (u32)__popcll(__ballot(blocked));
    n_pruned += (u32)__popcll(__ballot(pruned));
    n_stuck += (u32)__popcll(__ballot(stuck));
    if constexpr (HAS_STEP) {
      sbits = step ? sbits : 0;                                    // the bits of a blocked or pruned try are dropped
      n_pairs += (u32)__popcll(__ballot(step));
      simw_count(sbits, n_step, cp);
    }
    if constexpr (HAS_STATE) {
      wbits = stands ? wbits : 0;
      n_states += (u32)__popcll(__ballot(stands));
      simw_count(wbits, n_state, cs);
    }
    if (stop && stands && !done) {                                 // (lane-private) in the order of the contract; the constraint exports stop nothing
      if (sbits & ~step_con_bit) publish(4u, sbits & ~step_con_bit, depth);
      else if (wbits & ~state_con_bit) publish(3u, wbits & ~state_con_bit, depth);
      else if (bad) publish(1u, (u32)bad, depth);
    }
  }
  if (mine) {
    walker_rng[t] = rng;
    walker_depth[t] = depth;
    my_tried[0] = tried.w0;
    my_tried[1] = tried.w1;
    my_tried[2] = tried.w2;
    my_tried[3] = tried.w3;
  }
  if (lane_id() == 0) {                                            // one atomic per counter and wave
    if (n_steps) atomicAdd((unsigned long long*)&ctl->steps, (unsigned long long)n_steps);
    if (n_walks) atomicAdd((unsigned long long*)&ctl->walks, (unsigned long long)n_walks);
    if (n_states) atomicAdd((unsigned long long*)&ctl->n_states, (unsigned long long)n_states);
    if (n_pairs) atomicAdd((unsigned long long*)&ctl->n_pairs, (unsigned long long)n_pairs);
    if (n_blocked) atomicAdd((unsigned long long*)&ctl->blocked, (unsigned long long)n_blocked);
    if (n_pruned) atomicAdd((unsigned long long*)&ctl->pruned, (unsigned long long)n_pruned);
    if (n_stuck) atomicAdd((unsigned long long*)&ctl->stuck, (unsigned long long)n_stuck);
#pragma unroll
    for (int k = 0; k < WHERE_MAX_EXPORTS; k++) {
      if (cs[k]) atomicAdd((unsigned long long*)&ctl->count_state[k], (unsigned long long)cs[k]);
      if (cp[k]) atomicAdd((unsigned long long*)&ctl->count_step[k], (unsigned long long)cp[k]);
    }
  }
}

#endif  // __HIPCC__

}  // namespace vsr
