// vsr_action_constrain.hpp — action constraints: a BFS level expanded through a step predicate (TLC's ACTION_CONSTRAINT).  A transition
// whose verdict is false is generated and counted but NOT TAKEN: its successor is neither fingerprinted into the seen-set nor written, so the same state
// can still enter the model through a permitted transition, of this level or a later one.  That is why the gate cannot be a filter behind k_expand: a
// successor whose blocked edge arrived first would hold the seen-set slot already.
//
// Three kernels per slice of parents (host_action_constrain.hpp), the first two unchanged:
//   k_step_list    (vsr_step.hpp) the enabled instances of the slice as parent index | ordinal << 40
//   k_step_apply   (vsr_step.hpp) the step program over every listed pair, no hit list: rows[e] = action | bits << 8 | err << 16
//   k_step_expand  (here) one lane per list entry, whole waves together, no interpreter and therefore no LDS operand stack:
//     err bits set          the level error is raised as k_expand raises it (first one wins, parent index << 16 | ordinal beside it)
//     constraint bit clear  BLOCKED: counted in total and per action; the built-in invariants are evaluated on the successor only to count
//                           (blocked_violating, the or of the masks, the smallest parent fingerprint) — no violation is reported for a state outside the model
//     constraint bit set    gen_<false>, hash_child_, canonical_fp, key = meta_make(level, auxkey, parent fingerprint), table_claim_fused; the lane that
//                           inserted the fingerprint writes the successor (write_child_serial's stores) and nx_off[idx] = word offset << 8 | length, lvl_fp[idx] = fp.
//   The parent fingerprint is computed from the hashes the parent record carries (canonical_fp, as k_expand's staging does): lvl_fp is ONE array, and the
//   successors of an earlier slice have overwritten the entries of this slice's parents by the time it runs.
//   Room: one atomicAdd per wave and trip on LevelCtl::n_new for the indices (ballot + rank) and one on LevelCtl::words_new for the words (wave prefix sum of
//   the lengths).  The next level is therefore DENSE: no chunk slack, no withdrawn index, n_new == n_written.  A wave whose reservation does not fit raises
//   LevelCtl::full and writes nothing.  Every other counter lives in registers (ballot popcounts, per-lane minima) or, per action id, in 2 x 16 LDS words the
//   wave's leader lanes add to, and reaches the control blocks once per wave resp. block at the end of the launch.
//   `live` (one u32 per parent of the slice, zeroed by the host): the first listed instance of a parent flips it, so that the host has the level's
//   deadlocks as parents scanned minus parents with an instance — the figure k_expand's enumeration leaves in LevelCtl::deadlocks.
//
// Beyond the record buffers (expand_pass_gated, host_action_constrain.hpp) the same kernel runs in one of three compile-time modes:
//   GATE_STORED  the code above, unchanged: a stored level, and the level a descent inserts into a scratch buffer (the destination and its caps are the buffer's)
//   GATE_INSERT  the record-less first pass: the permitted successors are claimed exactly as above and NOTHING is written — no room is reserved, so the two
//                atomics per wave and trip are gone.  The claiming lane evaluates the invariants; n_new, fp_xor, fp_sum and max_bag live in registers over the
//                grid-stride loop and reach LevelCtl with one atomic per counter and wave at the end of the launch.  A violator is appended to `pending` as
//                (fingerprint, key) through wave_alloc — only a trip in which a lane has one issues that atomic.
//   GATE_PROBE   no claim: a permitted successor is looked up and dropped if it is a state of an earlier level; otherwise the invariants are evaluated and a
//                violator goes to `pending` and viol_fp / viol_mask, for deep_resolve (vsr_deep.hpp) as k_expand's MODE_PROBE leaves them.
//   In the last two modes nx_words / nx_words_cap carry the pending list and its capacity in ENTRIES (the kernel writes no record), nx_off, nx_cap and lvl_fp
//   are unused, and under VSRMC_TEST_HOOKS the state Model::test_bad_fp names fails Model::test_bad_mask, as in the general k_expand.
#pragma once
#include "vsr_kernels.hpp"
#include "vsr_step.hpp"

namespace vsr {

#if defined(__HIPCC__)

struct ActionCtl {
  u64 blocked;                        // transitions not taken
  u64 blocked_act[16];                // ... per action id
  u64 blocked_violating;              // blocked successors that fail a built-in invariant (counted, never reported)
  u64 blocked_viol_mask;              // the or of their masks
  u64 blocked_min_pfp;                // the smallest PARENT fingerprint of a blocked pair, ~0 = none
  u64 blocked_viol_min_pfp;           // ... of a blocked pair whose successor fails a built-in invariant
  u64 live_parents;                   // parents with at least one listed instance
};

// add one per lane of `who` to s_cnt[action]: one LDS atomic per distinct action of the wave, issued by the first lane that has it
__device__ __forceinline__ void actc_count_actions(unsigned long long* s_cnt, bool who, int action, int lane) {
  u64 rem = __ballot(who);
  while (rem) {                                                    // (wave-uniform)
    const int l = __ffsll((long long)rem) - 1;
    const int a = __builtin_amdgcn_readlane(action, l);
    const u64 m = __ballot(who && action == a);
    if (lane == l) atomicAdd(&s_cnt[a & 15], (unsigned long long)__popcll(m));
    rem &= ~m;
  }
}

// write_child_serial (vsr_kernels.hpp) with every subscript of the Delta and of the hashes a constant: its loops over M.wpr and M.np index D.rep and Hc
// at run time, which puts both in scratch memory; the stores are the same
__device__ __forceinline__ void actc_write_child(const Model& M, const u64* rec, const Delta& D, const u64* Hc, u64* dst) {
  const int nmsg = hdr_nmsg(rec[0]);
  const int len = M.fixed + nmsg;
  for (int k = 0; k < len; k++) dst[k] = rec[k];
  dst[0] = D.hdr;
  u64* ob = dst + 1 + ((int)D.r - 1) * M.wpr;
  ob[0] = D.rep[0];
  if (M.wpr > 1) ob[1] = D.rep[1];
  if (M.wpr > 2) ob[2] = D.rep[2];
  if (M.wpr > 3) ob[3] = D.rep[3];
#pragma unroll
  for (int k = 0; k < 6; k++)
    if (k < M.np) dst[M.h0 + k] = Hc[k];
  int a = 0;
#pragma unroll
  for (int k = 0; k < VSR_NSLOT; k++)
    if ((D.used >> k) & 1) {
      if (D.pj(k) >= 0) dst[M.fixed + D.pj(k)] = D.pnew[k];
      else dst[len + (a++)] = D.pnew[k];
    }
}

enum { GATE_STORED = 0, GATE_INSERT = 1, GATE_PROBE = 2 };

template <int MODEL, int GATE = GATE_STORED>
__global__ void __launch_bounds__(256)
k_step_expand(Model M, const u64* __restrict__ words, const u64* __restrict__ refs, const u64* __restrict__ list, const u32* __restrict__ rows, u64 n_entries,
              int k_bit, int level, u64 lo, Slot* table, u64 tmask, u64* nx_words, u64 nx_words_cap, u64* nx_off, u64 nx_cap, u64* lvl_fp, LevelCtl* ctl,
              ActionCtl* actl, u32* live) {
  typedef ModelOps<MODEL> Ops;
  __shared__ unsigned long long s_gen[16], s_blk[16];
  if (threadIdx.x < 16) { s_gen[threadIdx.x] = 0; s_blk[threadIdx.x] = 0; }
  __syncthreads();
  const int lane = lane_id();
  u32 n_gen = 0, n_written = 0, n_blocked = 0, n_bviol = 0, n_live = 0;              // wave-uniform (ballot popcounts)
  u64 rec_words = 0;                                                                 // wave-uniform
  u32 probes = 0, n_ties = 0, bag = 0, bmask = 0, vmask = 0;                         // per lane, reduced at the end
  u64 vmin = ~(u64)0, bmin = ~(u64)0, bvmin = ~(u64)0;
  u32 n_claimed = 0;                                                                 // GATE_INSERT, per lane: the level's states, their xor and sum
  u64 fxor = 0, fsum = 0;
  const u64 step = (u64)gridDim.x * blockDim.x;
  const u64 n_round = (n_entries + 63) & ~(u64)63;                 // whole waves stay together
  for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < n_round; e += step) {
    const bool have = e < n_entries;
    const u64 entry = have ? list[e] : 0;
    const u32 row = have ? rows[e] : 0;
    const u64 pidx = origin_pidx(entry);
    const int ord = origin_ord(entry);
    const u64 ref = have ? refs[pidx] : 0;
    const u64* rec = words + (ref >> 8);
    const int err = (int)((row >> 16) & 0xFF);
    const bool listed = have && ref != 0 && !(row >> 31);
    if (listed && err) raise_error(ctl, err, (pidx << 16) | (u64)ord);   // an evaluation error ends the run, as in k_expand
    const bool first = listed && atomicExch(&live[pidx - lo], 1u) == 0u;   // (the lanes of a wave hold different parents nearly always: k_step_list appends a round of one slot per parent)
    n_live += (u32)__popcll(__ballot(first));
    Delta D = Delta();
    bool valid = listed && !err;
    if (valid && (!Ops::template gen_<false>(M, rec, ord, D) || D.err)) {   // (k_step_apply ran the same statement on the same record: never)
      raise_error(ctl, ERR_INTERNAL, (pidx << 16) | (u64)ord);
      valid = false;
    }
    const int action = (int)D.action;
    n_gen += (u32)__popcll(__ballot(valid));
    actc_count_actions(s_gen, valid, action, lane);
    const bool permitted = valid && ((row >> (8 + k_bit)) & 1u);
    const bool blocked = valid && !permitted;
    u64 pfp = 0;
    u32 pak = 0;
    if (valid) canonical_fp(M, rec[0], rec + M.h0, &pfp, &pak);
    const u64 bb = __ballot(blocked);
    if (bb) {                                                      // (wave-uniform)
      n_blocked += (u32)__popcll(bb);
      actc_count_actions(s_blk, blocked, action, lane);
      int bad = blocked ? Ops::invariants(M, rec, D) : 0;
#ifdef VSRMC_TEST_HOOKS
      if (blocked && M.test_bad_mask) {                            // test hook (Model::test_bad_fp): a blocked successor is not fingerprinted — except here, to count it
        u64 Hb[6], bfp;
        u32 bak;
        Ops::hash_child_(M, rec, D, Hb);
        canonical_fp(M, D.hdr, Hb, &bfp, &bak);
        if (bfp == M.test_bad_fp) bad |= (int)M.test_bad_mask;
      }
#endif
      n_bviol += (u32)__popcll(__ballot(bad != 0));
      if (blocked) {
        bmin = pfp < bmin ? pfp : bmin;
        if (bad) { bmask |= (u32)bad; bvmin = pfp < bvmin ? pfp : bvmin; }
      }
    }
    // the transitions taken: fingerprint, claim (GATE_PROBE: lookup), and the claiming lane's reservation
    bool claimed = false;
    u64 fp = 0, Hc[6];
    int clen = 0;
    [[maybe_unused]] u64 key = 0;
    if (permitted) {
      Ops::hash_child_(M, rec, D, Hc);
      u32 ak;
      canonical_fp(M, D.hdr, Hc, &fp, &ak);
      key = meta_make(level, ak, pfp);
      if constexpr (GATE == GATE_PROBE) {
        u64 m = META_EMPTY;
        claimed = !(probe_lookup(table, tmask, fp, &m, CntReg{&probes}) && meta_level(m) < level);   // (here: not a state of an earlier level — a candidate)
      } else {
        bool full = false;
        u64 prev_meta = META_EMPTY;
        table_claim_fused(table, tmask, fp, key, level, &claimed, &prev_meta, CntReg{&probes}, &full);
        if (full) {
          raise_error(ctl, ERR_TABLE_FULL, fp);
          claimed = false;
        }
        if (!full && prev_meta != META_EMPTY && meta_level(prev_meta) == level && meta_auxkey(prev_meta) != meta_auxkey(key)) n_ties++;
        if (claimed) clen = M.fixed + hdr_nmsg(D.hdr);
      }
    }
    if constexpr (GATE != GATE_STORED) {                           // nothing is written: counted and checked in registers, a violator listed
      int bad = 0;
      if (claimed) {
        bad = Ops::invariants(M, rec, D);
#ifdef VSRMC_TEST_HOOKS
        if (M.test_bad_mask && fp == M.test_bad_fp) bad |= (int)M.test_bad_mask;   // test hook (Model::test_bad_fp)
#endif
        if constexpr (GATE == GATE_INSERT) {
          n_claimed++;
          fxor ^= fp;
          fsum += fp;
          bag = max(bag, (u32)hdr_nmsg(D.hdr));
        }
        if (bad) { vmask |= (u32)bad; vmin = fp < vmin ? fp : vmin; }
      }
      if (bad) {                                                   // (divergent: wave_alloc counts the lanes that are here; no lane, no atomic)
        const u64 i = wave_alloc(&ctl->n_pending);
        if (i < nx_words_cap) {
          nx_words[2 * i] = fp;
          nx_words[2 * i + 1] = key;
        }
      }
      continue;                                                    // (every lane of the wave: nothing above leaves the loop)
    }
    const u64 cb = __ballot(claimed);
    if (cb == 0) continue;                                         // (wave-uniform)
    // one atomic per wave for the indices, one for the words
    int incl = clen;                                               // inclusive prefix sum of the lengths over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    const u32 total = (u32)__shfl(incl, 63);
    const u32 cnt = (u32)__popcll(cb);
    u64 ibase = 0, wbase = 0;
    if (lane == 0) {
      ibase = atomicAdd((unsigned long long*)&ctl->n_new, (unsigned long long)cnt);
      wbase = atomicAdd((unsigned long long*)&ctl->words_new, (unsigned long long)total);
    }
    ibase = readlane64(ibase, 0);
    wbase = readlane64(wbase, 0);
    // the claiming lane checks its state BEFORE the room is looked at: a level that overflows the buffers is complete in the seen-set, counted in n_new and
    // checked all the same, so that the host can keep it as a seen-set-only level (adopt_overflowed_level)
    if (claimed) {
      bag = max(bag, (u32)hdr_nmsg(D.hdr));
      int bad = Ops::invariants(M, rec, D);
#ifdef VSRMC_TEST_HOOKS
      if (M.test_bad_mask && fp == M.test_bad_fp) bad |= (int)M.test_bad_mask;   // test hook (Model::test_bad_fp): a violator on a level that overflows
#endif
      if (bad) { vmask |= (u32)bad; vmin = fp < vmin ? fp : vmin; }
    }
    if (ibase + cnt > nx_cap || wbase + total > nx_words_cap) {    // (wave-uniform) out of index or word room: nothing of this wave is written
      if (lane == 0) raise_full(ctl, pidx);
      continue;
    }
    n_written += cnt;
    rec_words += total;
    if (claimed) {
      const u64 idx = ibase + (u64)__popcll(cb & (((u64)1 << lane) - 1));
      const u64 dst = wbase + (u64)(incl - clen);
      actc_write_child(M, rec, D, Hc, nx_words + dst);
      nx_off[idx] = (dst << 8) | (u64)clen;
      lvl_fp[idx] = fp;
    }
  }
  // the end of the launch: every lane of the wave is here (the loop above only `continue`s at wave-uniform points); one reduction and one atomic per counter and wave
  const u32 w_probes = wave_sum32(probes), w_ties = wave_sum32(n_ties), w_bag = wave_max32(bag), w_vmask = wave_or32(vmask), w_bmask = wave_or32(bmask);
  const u64 w_vmin = wave_min64(vmin), w_bmin = wave_min64(bmin), w_bvmin = wave_min64(bvmin);
  [[maybe_unused]] u32 w_claimed = 0;
  [[maybe_unused]] u64 w_fxor = 0, w_fsum = 0;
  if constexpr (GATE == GATE_INSERT) { w_claimed = wave_sum32(n_claimed); w_fxor = wave_xor64(fxor); w_fsum = wave_sum64(fsum); }
  if (lane == 0) {
    if (n_gen) atomicAdd((unsigned long long*)&ctl->generated, (unsigned long long)n_gen);
    if (n_written) atomicAdd((unsigned long long*)&ctl->n_written, (unsigned long long)n_written);
    if (rec_words) atomicAdd((unsigned long long*)&ctl->rec_words, (unsigned long long)rec_words);
    if (w_probes) atomicAdd((unsigned long long*)&ctl->probes, (unsigned long long)w_probes);
    if (w_ties) atomicAdd((unsigned long long*)&ctl->ties, (unsigned long long)w_ties);
    if (w_bag) atomicMax((unsigned long long*)&ctl->max_bag, (unsigned long long)w_bag);
    if (w_vmask) {
      atomicMin((unsigned long long*)&ctl->viol_fp, (unsigned long long)w_vmin);
      atomicOr(&ctl->viol_mask, w_vmask);
    }
    if constexpr (GATE == GATE_INSERT) {                           // the level's size and checksums: what k_expand's MODE_INSERT leaves (no lvl_fp array exists)
      if (w_claimed) {
        atomicAdd((unsigned long long*)&ctl->n_new, (unsigned long long)w_claimed);
        atomicXor((unsigned long long*)&ctl->fp_xor, (unsigned long long)w_fxor);
        atomicAdd((unsigned long long*)&ctl->fp_sum, (unsigned long long)w_fsum);
      }
    }
    if (n_live) atomicAdd((unsigned long long*)&actl->live_parents, (unsigned long long)n_live);
    if (n_blocked) {
      atomicAdd((unsigned long long*)&actl->blocked, (unsigned long long)n_blocked);
      atomicMin((unsigned long long*)&actl->blocked_min_pfp, (unsigned long long)w_bmin);
    }
    if (n_bviol) {
      atomicAdd((unsigned long long*)&actl->blocked_violating, (unsigned long long)n_bviol);
      atomicOr((unsigned long long*)&actl->blocked_viol_mask, (unsigned long long)w_bmask);
      atomicMin((unsigned long long*)&actl->blocked_viol_min_pfp, (unsigned long long)w_bvmin);
    }
  }
  __syncthreads();
  if (threadIdx.x < 16 && s_gen[threadIdx.x]) atomicAdd((unsigned long long*)&ctl->act_generated[threadIdx.x], s_gen[threadIdx.x]);
  if (threadIdx.x >= 16 && threadIdx.x < 32 && s_blk[threadIdx.x - 16]) atomicAdd((unsigned long long*)&actl->blocked_act[threadIdx.x - 16], s_blk[threadIdx.x - 16]);
}

// The step scan of a constrained checker (host_step.hpp): of the listed instances of a slice the ones the action constraint does not block, out of place, so
// that k_step_apply with the user's query runs over transitions of the model only.  `rows` is what k_step_apply left for the CONSTRAINT's program.  An
// instance whose action raises an evaluation error stays (it is no transition, and the scan counts it as before); order is not kept (the list has none).
// One atomicAdd per wave and trip (ballot + rank); kept[] holds as many entries as list[], so no index is out of range.
__global__ void __launch_bounds__(256)
k_step_keep(const u64* __restrict__ list, const u32* __restrict__ rows, u64 n_entries, int k_bit, u64* kept, u64* n_kept) {
  const int lane = lane_id();
  const u64 step = (u64)gridDim.x * blockDim.x;
  const u64 n_round = (n_entries + 63) & ~(u64)63;                 // whole waves stay together
  for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < n_round; e += step) {
    const bool have = e < n_entries;
    const u32 row = have ? rows[e] : 0;
    const bool keep = have && !(row >> 31) && (((row >> 16) & 0xFF) || ((row >> (8 + k_bit)) & 1u));
    const u64 kb = __ballot(keep);
    if (kb == 0) continue;                                         // (wave-uniform)
    u64 base = 0;
    if (lane == 0) base = atomicAdd((unsigned long long*)n_kept, (unsigned long long)__popcll(kb));
    base = readlane64(base, 0);
    if (keep) kept[base + (u64)__popcll(kb & (((u64)1 << lane) - 1))] = list[e];
  }
}

#endif  // __HIPCC__

}  // namespace vsr
