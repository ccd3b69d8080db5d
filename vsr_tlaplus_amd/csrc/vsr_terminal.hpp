// vsr_terminal.hpp — k_terminal: which records of a level are TERMINAL states (TLC's deadlock check, -deadlock / CHECK_DEADLOCK), and in which of them
// the view change has not completed.  A streaming scan: it reads every record once, evaluates guards only (ModelOps<MODEL>::guard, the statement k_select
// and k_simulate use), never applies an action and never touches the seen-set.  k_expand is not involved: the scan is a launch of its own that runs only
// when a caller asks for it (vsrmc_terminal_batch, vsrmc_checker_terminal_scan; host_terminal.hpp).
//
// Per record one flag byte:
//   bit 0  terminal: no (action, binding) instance is enabled — the popcount of the guard masks over all M.m0 + nmsg slots is 0.  This is the definition
//          k_simulate ends a walk by and the one k_expand's LevelCtl::deadlocks counts, so terminal(level L) == deadlocks(the step that expands L).
//   bit 1  unsettled: AllReplicasMoveToSameView (VSR.tla:958-962: every rep_status = Normal, all rep_view_number equal) is FALSE.  Read from the A word of
//          each replica block (status bits 0-1 with Normal = 0, view bits 2-4: a_status / a_view, vsr_model.hpp).  All three models keep both fields in
//          that word — VSR.tla at rec[1 + (r-1) wpr], VR_STATE_TRANSFER at rec[r] (wpr = 1), VR_APP_STATE at rec[c_ia(r)] = rec[1 + 2 (r-1)] (wpr = 2) —
//          so bit 1 is computed for every model (tests/test_terminal_states.py compares it with the Python restatements' decoders for all three).
// A terminal state with bit 1 set is a counter-example to ViewChangeCompletes == []<>AllReplicasMoveToSameView under WF_vars(Next) (the behaviour that
// reaches it and stutters is fair); that none exists proves nothing about behaviours that loop — loops are not examined here.
//
// Input: `refs[i]` = word offset << 8 | record length, 0 = a withdrawn index (the frontier's own ref array); `fps[i]` = the record's fingerprint (the
// level's lvl_fp array) or nullptr (a caller's batch: no minima, no list).  Output: `flags` (optional), the counters of TermCtl, the smallest
// fingerprint of the terminal / terminal-and-unsettled records (atomicMin, one per wave that has one), and a list of (fingerprint, index, flags)
// triples of the terminal records, appended wave-wise (wave_alloc: one atomicAdd per wave), of which the first list_cap that arrive are kept;
// TermCtl::n_list is the true number.
//
// Shape: one lane per record, straight from global memory (the k_select shape), grid-stride over whole waves.  A wave-cooperative variant — 64 records
// staged into LDS the way k_expand stages its tiles, the block's four waves sharing each record's slots — was built and measured against it (DESIGN.md
// §9a, profiles/terminal_scan.json): 25-38 % slower where the scan is bound by the record stream (the README configuration, the levels that grow towards
// the headline's 6e8 records), 2-12 % faster only on config 2's dying levels; it lost on the sum and was removed.
#pragma once

namespace vsr {

struct TermCtl {
  u64 scanned, terminal, unsettled;   // records looked at (holes excluded), terminal ones, terminal-and-unsettled ones
  u64 min_fp, min_fp_unsettled;       // ~0 = none
  u64 n_list;                         // terminal records offered to the list (= terminal when there is a list)
};

template <typename PTR>
VSR_HD int term_unsettled(const Model& M, PTR rec) {
  const u64 A1 = rec[1];
  int bad = a_status(A1) != ST_NORMAL;
  for (int r = 2; r <= M.R; r++) {
    const u64 A = rec[1 + (r - 1) * M.wpr];
    bad |= (a_status(A) != ST_NORMAL) | (a_view(A) != a_view(A1));
  }
  return bad;
}

// what every lane does with its record's verdict (valid = the lane has a record); all 64 lanes of the wave call it together
__device__ __forceinline__ void term_emit(bool valid, bool terminal, int unsettled, u64 i, const u64* __restrict__ fps, uint8_t* flags, TermCtl* ctl,
                                          u64* list, u64 list_cap, u64& n_scanned, u64& n_term, u64& n_uns) {
  const int f = valid ? ((terminal ? 1 : 0) | (unsettled ? 2 : 0)) : 0;
  if (valid && flags) flags[i] = (uint8_t)f;
  n_scanned += valid ? 1 : 0;
  const bool t = valid && terminal;
  n_term += t ? 1 : 0;
  n_uns += (t && unsettled) ? 1 : 0;
  if (!fps) return;
  if (__ballot(t) == 0) return;                                  // (wave-uniform)
  const u64 fp = t ? fps[i] : ~(u64)0;
  const u64 m = wave_min64(fp);
  const u64 mu = wave_min64((t && unsettled) ? fp : ~(u64)0);
  if (lane_id() == 0) {
    atomicMin((unsigned long long*)&ctl->min_fp, (unsigned long long)m);
    if (mu != ~(u64)0) atomicMin((unsigned long long*)&ctl->min_fp_unsettled, (unsigned long long)mu);
  }
  if (t) {
    const u64 k = wave_alloc(&ctl->n_list);
    if (k < list_cap) {
      list[3 * k] = fp;
      list[3 * k + 1] = i;
      list[3 * k + 2] = (u64)f;
    }
  }
}

__device__ __forceinline__ void term_flush(TermCtl* ctl, u64 n_scanned, u64 n_term, u64 n_uns) {   // one atomic per counter and wave
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    n_scanned += (u64)__shfl_xor((unsigned long long)n_scanned, d);
    n_term += (u64)__shfl_xor((unsigned long long)n_term, d);
    n_uns += (u64)__shfl_xor((unsigned long long)n_uns, d);
  }
  if (lane_id() == 0) {
    if (n_scanned) atomicAdd((unsigned long long*)&ctl->scanned, (unsigned long long)n_scanned);
    if (n_term) atomicAdd((unsigned long long*)&ctl->terminal, (unsigned long long)n_term);
    if (n_uns) atomicAdd((unsigned long long*)&ctl->unsettled, (unsigned long long)n_uns);
  }
}

template <int MODEL>
__global__ void __launch_bounds__(256)
k_terminal(Model M, const u64* __restrict__ words, const u64* __restrict__ refs, const u64* __restrict__ fps, u64 n, uint8_t* flags, TermCtl* ctl,
           u64* list, u64 list_cap) {
  typedef ModelOps<MODEL> Ops;
  u64 n_scanned = 0, n_term = 0, n_uns = 0;
  const u64 step = (u64)gridDim.x * blockDim.x;
  const u64 n_round = (n + 63) & ~(u64)63;                       // whole waves stay together: term_emit is a wave-wide call
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += step) {
    const u64 ref = i < n ? refs[i] : 0;
    const bool valid = ref != 0;
    bool any = false;
    int uns = 0;
    if (valid) {
      const u64* rec = words + (ref >> 8);
      const int nslots = M.m0 + hdr_nmsg(rec[0]);
      for (int slot = 0; slot < nslots && !any; slot++) {
        int kind0 = 0;
        any = Ops::guard(M, rec, slot, &kind0) != 0;
      }
      uns = term_unsettled(M, rec);
    }
    term_emit(valid, !any, uns, i, fps, flags, ctl, list, list_cap, n_scanned, n_term, n_uns);
  }
  term_flush(ctl, n_scanned, n_term, n_uns);
}

}  // namespace vsr
