// vsr_deep_terminal.hpp — k_probe_children: the states of the PROBED level of the search beyond the record buffers (vsr_deep.hpp) as records, chunk by
// chunk, so that k_terminal (vsr_terminal.hpp) can ask each of them "are you terminal, and if so, is the view change complete?" (DESIGN.md §9k).
//
// The probed level has no records: its states exist only as the successors the probe pass generates from a sub-slice of the inserted level and drops.
// The guards are written against records (template <typename PTR> over a pointer that supports rec + k; the analysis models' guard_slot runs gen<true>
// over it), so they are not evaluated through a view of (parent, Delta) here: the fresh successors are MATERIALISED into a buffer of the terminal
// attachment (host_deep_terminal.hpp) and k_terminal, unchanged, reads them.  The kernel has the shape of k_probe_where (vsr_deep_where.hpp) and the
// writing half of k_step_expand (vsr_action_constrain.hpp): one lane per entry [e_lo, e_hi) of the instance list k_step_list (vsr_step.hpp) wrote for
// the sub-slice, grid-stride over whole waves.  Per entry:
//
//   ModelOps<MODEL>::gen_<false>          the Delta (an instance whose action raises an evaluation error — a bag over the cap, ERR_REP_BAG, among them —
//                                          has no successor: counted, not written; a listed instance that is not enabled is counted as internal);
//   hash_child_, canonical_fp, meta_make  the successor's fingerprint and key, as the search's probe computes them;
//   probe_lookup                           read-only: a successor the seen-set holds (a state of a level below the probed one) is dropped, as TLC drops it.
//
// Room: the fresh lanes of a wave reserve with ONE atomic for the indices and ONE for the words per wave and trip (ballot + rank, wave prefix sum of the
// lengths), so the chunk is dense: refs[idx] = word offset << 8 | length, fps[idx] = fingerprint, keys[idx] = key.  A wave whose reservation would not fit
// writes nothing and raises `dropped`; the host sizes the launches so that it cannot happen (entries x (fixed + child bag bound) <= the buffer) and turns a
// non-zero `dropped` into an error.  Nothing is ever stored past the buffers.  The records are written by actc_write_child, whose constant subscripts keep
// the Delta out of scratch memory.  Every other counter lives in registers (ballot popcounts: wave-uniform) and takes one atomic per wave at the end.
//
// The same state arrives from several parents, and some copies turn out to be states of the inserted level once it is complete: the host drops those
// (k_table_seen) and de-duplicates by fingerprint, keeping the smallest key (host_deep_terminal.hpp) — what deep_resolve does for the invariants.
#pragma once
#include "vsr_action_constrain.hpp"

namespace vsr {

#if defined(__HIPCC__)

struct ProbeChildCtl {
  u64 n_idx, n_words;                 // this launch: records written, words written (the host clears both before every launch)
  u64 n_entries;                      // the whole pass: list entries looked at
  u64 n_fresh;                        // successors that are not in the seen-set (copies of one state counted each)
  u64 n_err, n_internal;              // instances whose action raises an evaluation error; listed instances gen_<false> calls disabled (never)
  u64 dropped;                        // fresh successors of waves whose reservation did not fit (never: the host sizes the launches)
};

template <int MODEL>
__global__ void __launch_bounds__(256)
k_probe_children(Model M, const u64* __restrict__ words, const u64* __restrict__ refs, const u64* __restrict__ list, u64 e_lo, u64 e_hi, const Slot* table,
                 u64 tmask, int level, u64* out_words, u64 out_words_cap, u64* out_refs, u64* out_fps, u64* out_keys, u64 out_cap, ProbeChildCtl* ctl) {
  typedef ModelOps<MODEL> Ops;
  const int lane = lane_id();
  u32 n_seen = 0, n_fresh = 0, n_err = 0, n_internal = 0, n_dropped = 0;   // wave-uniform (ballot popcounts)
  const u64 step = (u64)gridDim.x * blockDim.x;
  const u64 e_round = e_lo + ((e_hi - e_lo + 63) & ~(u64)63);     // whole waves stay together
  for (u64 e = e_lo + (u64)blockIdx.x * blockDim.x + threadIdx.x; e < e_round; e += step) {
    const bool have = e < e_hi;
    const u64 entry = have ? list[e] : 0;
    const u64 ref = have ? refs[origin_pidx(entry)] : 0;
    const u64* rec = words + (ref >> 8);
    Delta D = Delta();
    bool enabled = false;
    if (have) enabled = Ops::template gen_<false>(M, rec, origin_ord(entry), D);
    const bool ok = have && enabled && D.err == 0;
    u64 fp = 0, key = 0, Hc[6];
    bool fresh = false;
    if (ok) {
      Ops::hash_child_(M, rec, D, Hc);
      u64 pfp;
      u32 ak, pak;
      canonical_fp(M, D.hdr, Hc, &fp, &ak);
      canonical_fp(M, rec[0], rec + M.h0, &pfp, &pak);
      key = meta_make(level, ak, pfp);
      u64 m = META_EMPTY;
      u32 np = 0;
      fresh = !(probe_lookup(table, tmask, fp, &m, CntReg{&np}) && meta_level(m) < level);
    }
    n_seen += (u32)__popcll(__ballot(have));
    n_err += (u32)__popcll(__ballot(have && enabled && D.err != 0));
    n_internal += (u32)__popcll(__ballot(have && !enabled));
    const bool valid = ok && fresh;
    const u64 vb = __ballot(valid);
    if (vb == 0) continue;                                         // (wave-uniform) every successor of this wave is a state the search has seen
    const u32 cnt = (u32)__popcll(vb);
    n_fresh += cnt;
    const int clen = valid ? M.fixed + hdr_nmsg(D.hdr) : 0;
    int incl = clen;                                               // inclusive prefix sum of the lengths over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    const u32 total = (u32)__shfl(incl, 63);
    u64 ibase = 0, wbase = 0;
    if (lane == 0) {                                               // one atomic per wave for the indices, one for the words
      ibase = atomicAdd((unsigned long long*)&ctl->n_idx, (unsigned long long)cnt);
      wbase = atomicAdd((unsigned long long*)&ctl->n_words, (unsigned long long)total);
    }
    ibase = readlane64(ibase, 0);
    wbase = readlane64(wbase, 0);
    if (ibase + cnt > out_cap || wbase + total > out_words_cap) {  // (wave-uniform) out of index or word room: nothing of this wave is written
      n_dropped += cnt;
      continue;
    }
    if (valid) {
      const u64 idx = ibase + (u64)__popcll(vb & (((u64)1 << lane) - 1));
      const u64 dst = wbase + (u64)(incl - clen);
      actc_write_child(M, rec, D, Hc, out_words + dst);
      out_refs[idx] = (dst << 8) | (u64)clen;
      out_fps[idx] = fp;
      out_keys[idx] = key;
    }
  }
  if (lane == 0) {                                                 // one atomic per counter and wave
    if (n_seen) atomicAdd((unsigned long long*)&ctl->n_entries, (unsigned long long)n_seen);
    if (n_fresh) atomicAdd((unsigned long long*)&ctl->n_fresh, (unsigned long long)n_fresh);
    if (n_err) atomicAdd((unsigned long long*)&ctl->n_err, (unsigned long long)n_err);
    if (n_internal) atomicAdd((unsigned long long*)&ctl->n_internal, (unsigned long long)n_internal);
    if (n_dropped) atomicAdd((unsigned long long*)&ctl->dropped, (unsigned long long)n_dropped);
  }
}

#endif  // __HIPCC__

}  // namespace vsr
