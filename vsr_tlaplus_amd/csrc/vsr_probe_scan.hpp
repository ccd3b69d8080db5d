// vsr_probe_scan.hpp — the probe pass of the deep search as two kernels of its own (VSR.tla configurations with R <= 3).
//
// A probe pass inserts nothing and hashes nothing: it counts the enabled instances of every parent (generated, per action, deadlocks) and checks the
// invariants of the successors of the few instances inside the invariants' footprint (ModelOps::probe_actions, 2 % on the README configuration).
//   k_probe_scan   streams the records and enumerates them, wave by wave: a wave owns a mini-tile of 16 records, nothing is shared between the waves
//                  of a block and no block barrier stands in the loop.  Instances outside the footprint are counted; the ones inside it are appended
//                  to a global list as (parent index, ordinal, action).  No action body, no Delta, no hash, no seen-set code.
//   k_probe_apply  one lane per list entry: gen + invariants on the parent's record in global memory; a failing successor goes to `pending` as an
//                  (origin, 0) pair — what k_probe_resolve (vsr_kernels.hpp) takes from there, as it did from k_expand<.., EXPAND_PROBE>.
#pragma once
#include "vsr_kernels.hpp"

namespace vsr {

constexpr int PSCAN_MT = 16;            // records of a mini-tile: 4 lanes per record while enumerating, 16 lanes per record while staging
constexpr int PSCAN_DRAW = 16;          // mini-tiles per draw from LevelCtl::tile_cursor: 256 records, the same atomics per record as k_expand (VSR_TILE_BATCH x 64)
constexpr int PSCAN_LISTQ = 128;        // entries of a wave's survivor list and of its list of footprint instances (each is emptied when it reaches 64)
constexpr int PSCAN_LIST_HDR = 16;      // u64 words in front of the global list's entries: word 0 counts the entries appended (a cache line of its own)
constexpr int PSCAN_WAVE_EXTRA = PSCAN_LISTQ + PSCAN_MT + PSCAN_LISTQ / 4 + 3 * PSCAN_MT / 2;   // u64 words of a wave's LDS region beside its 16 records
// a list entry: parent index (40 bits) | ordinal << 40 (16 bits) | action id << 56
__host__ __device__ __forceinline__ u64 pscan_entry(u64 pidx, int ord, int kind) { return pidx | ((u64)ord << 40) | ((u64)kind << 56); }
__host__ __device__ __forceinline__ size_t pscan_lds_bytes(int stride) { return (size_t)(VSR_BLOCK / 64) * (size_t)(PSCAN_MT * stride + PSCAN_WAVE_EXTRA) * 8; }

template <int SPEC>
__global__ void __launch_bounds__(VSR_BLOCK, VSR_OCC)
k_probe_scan(Model Marg, const u64* __restrict__ fr_words, const u64* __restrict__ fr_off, u64 n_parents, LevelCtl* ctl, int stride,
             u32 draw /* mini-tiles per draw, the same in every wave of the launch */, u64* list, u64 list_cap) {
  static_assert(SPEC / 1000 == 0 && SPEC % 1000 != 0 && (SPEC % 1000) / 100 <= 3, "VSR.tla, R <= 3: a record fits 64 words, a replica per lane group");
  typedef ModelOps<0> Ops;
  Model M = Marg;
  specialise<SPEC>(M, Marg);
  extern __shared__ u64 smem[];
  __shared__ unsigned int s_sum[20];                            // the block's counters, added up once, in the epilogue: 0..15 per action, 16 deadlocks, 17 limit_unchecked
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64* const s_rec = smem + wave * (PSCAN_MT * stride + PSCAN_WAVE_EXTRA);   // this wave's records ...
  u64* const s_out = s_rec + PSCAN_MT * stride;                 // ... the footprint instances it has not written out yet
  u64* const s_ref = s_out + PSCAN_LISTQ;                       // ... the records' refs
  unsigned short* const s_surv = (unsigned short*)(s_ref + PSCAN_MT);   // ... (record << 8 | bag index) pairs that passed the prefilter
  u32* const s_alive = (u32*)(s_ref + PSCAN_MT + PSCAN_LISTQ / 4);      // ... per record: an instance is enabled,
  u32* const s_nonfp = s_alive + PSCAN_MT;                      // one outside the footprint is,
  u32* const s_limit = s_nonfp + PSCAN_MT;                      // the record sits at a representation limit
  if (threadIdx.x < 20) s_sum[threadIdx.x] = 0;
  __syncthreads();

  const u64 nmt = (n_parents + PSCAN_MT - 1) / PSCAN_MT;
  const u64 lt_mask = ((u64)1 << lane) - 1;
  const u32 FOOT = Ops::probe_actions();                        // the actions whose instances are listed; the others' are counted
  constexpr u32 RECV = (1u << A_ReceiveHigherSVC) | (1u << A_ReceiveMatchingSVC) | (1u << A_ReceiveHigherDVC) | (1u << A_ReceiveMatchingDVC) | (1u << A_ReceiveSV) |
                       (1u << A_ReceivePrepareMsg) | (1u << A_ReceivePrepareOkMsg) | (1u << A_ReceiveGetState) | (1u << A_ReceiveNewState);   // what bit 0 of a bag slot's guard can be
  u32 cnt[16];                                                   // wave-uniform: enabled instances per action
#pragma unroll
  for (int a = 0; a < 16; a++) cnt[a] = 0;
  u32 ndead = 0, nlimit = 0, nout = 0;

  // ---- mini-tiles: drawn `draw` at a time, the next draw's atomic issued one batch ahead (lane 0 keeps its answer until it is needed)
  u64 cur = 0, nxt_v = 0;
  u32 left = 0;
  if (lane == 0) nxt_v = atomicAdd((unsigned long long*)&ctl->tile_cursor, 1ull);
  auto next_mt = [&]() -> u64 {
    if (left == 0) {
      cur = readlane64(nxt_v, 0) * (u64)draw;
      left = draw;
      if (lane == 0 && cur < nmt) nxt_v = atomicAdd((unsigned long long*)&ctl->tile_cursor, 1ull);
    }
    left--;
    return cur++;
  };
  // staging, 16 lanes per record: a lane moves words l16, l16 + 16, .. of records q, q + 4, q + 8, q + 12
  const int l16 = lane & 15, q0 = lane >> 4;
  auto load_refs = [&](u64 mt, u64* refq) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const u64 idx = mt * PSCAN_MT + (u64)(q0 + 4 * q);
      refq[q] = (mt < nmt && idx < n_parents) ? fr_off[idx] : 0;
    }
  };
  auto load_words = [&](const u64* refq, u64 (*v)[4]) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const u64 off = refq[q] >> 8;
      const int len = (int)(refq[q] & 255) < stride ? (int)(refq[q] & 255) : stride;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int k = l16 + 16 * j;
        v[q][j] = k < len ? fr_words[off + k] : 0;
      }
    }
  };
  auto flush = [&]() {                                           // the wave's footprint instances: one atomic on the list's counter
    lds_wave_sync();
    u64 base = 0;
    if (lane == 0) base = atomicAdd((unsigned long long*)list, (unsigned long long)nout);
    base = readlane64(base, 0);
    for (u32 i = (u32)lane; i < nout; i += 64)
      if (base + i < list_cap) list[PSCAN_LIST_HDR + base + i] = s_out[i];   // (an overflow is seen by the host in the counter: the pass is run again by k_expand)
    lds_wave_sync();
    nout = 0;
  };
  auto push = [&](bool pred, u64 entry) {                        // called by the whole wave
    const u64 bal = __ballot(pred);
    if (bal) {
      if (pred) s_out[nout + (u32)__popcll(bal & lt_mask)] = entry;
      nout += (u32)__popcll(bal);
      if (nout >= 64) flush();
    }
  };

  u64 refA[4], refB[4], v[4][4];
  u64 mt0 = next_mt();
  load_refs(mt0, refA);
  load_words(refA, v);
  u64 mt1 = next_mt();
  load_refs(mt1, refB);
  while (mt0 < nmt) {
    // ---- this mini-tile's words into LDS; the next one's loads and the refs of the one after are issued before the enumeration starts
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int p = q0 + 4 * q;
      const int len = (int)(refA[q] & 255) < stride ? (int)(refA[q] & 255) : stride;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int k = l16 + 16 * j;
        if (k < len) s_rec[p * stride + k] = v[q][j];
      }
      if (l16 == 0) s_ref[p] = refA[q];
    }
    if (lane < PSCAN_MT) { s_alive[lane] = 0; s_nonfp[lane] = 0; s_limit[lane] = 0; }
    load_words(refB, v);
#pragma unroll
    for (int q = 0; q < 4; q++) refA[q] = refB[q];
    const u64 mt2 = next_mt();
    load_refs(mt2, refB);
    lds_wave_sync();

    // ---- enumerate: record p = lane & 15, its lanes g = 0..3
    const u64 p_base = mt0 * PSCAN_MT;
    const int np = (int)((n_parents - p_base) < (u64)PSCAN_MT ? (n_parents - p_base) : (u64)PSCAN_MT);
    const int p = lane & (PSCAN_MT - 1), g = lane >> 4;
    const u64 ref = s_ref[p];
    const bool valid = p < np && ref != 0;
    const u64* rec = s_rec + p * stride;
    if (valid && g == 0 && (int)(ref & 255) > stride) raise_error(ctl, ERR_INTERNAL, (p_base + (u64)p) << 16);   // LDS slots sized for shorter records
    u64 hdr = 0, lut[4] = {0, 0, 0, 0};
    int nmsg = 0;
    u32 m = 0;
    if (valid) {
      hdr = rec[0];
      nmsg = hdr_nmsg(hdr);
      u64 Areg[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int r = 1; r <= 3; r++)
        if (r <= M.R) { Areg[r] = rec[1 + (r - 1) * M.wpr]; lut[r] = prefilter_lut(M, Areg[r], r); }
      if (g < M.R) m = rep_slots_mask(M, rec, hdr, areg_of(Areg, g + 1), g + 1);
      if (nmsg + M.R - 1 > M.max_bag) s_limit[p] = 1;           // a bag within R - 1 entries of its capacity
    }
    // the replica-bound instances of replica g + 1: bit 0 TimerSendSVC, 1 SendDVC, 2 SendSV, 3 ExecuteOp, 4.. ReceiveClientRequest(c, v)
    {
      const u64 pidx = p_base + (u64)p;
      auto rep_bit = [&](bool on, int kind, int ord) {           // (kind is a constant at every call: the footprint test folds)
        cnt[kind] += (u32)__popcll(__ballot(on));
        if ((FOOT >> kind) & 1u) push(on, pscan_entry(pidx, ord, kind));
        else if (on) s_nonfp[p] = 1;
      };
      if (m) s_alive[p] = 1;
      rep_bit((m & 1u) != 0, A_TimerSendSVC, g);
      rep_bit((m & 2u) != 0, A_SendDVC, M.R + g);
      rep_bit((m & 4u) != 0, A_SendSV, 2 * M.R + g);
      rep_bit((m & 8u) != 0, A_ExecuteOp, 3 * M.R + g);
      if (__ballot((m >> 4) != 0)) {
#pragma unroll
        for (int b = 0; b < 9; b++)
          if (b < M.C * M.n) rep_bit(((m >> (4 + b)) & 1u) != 0, A_ReceiveClientRequest, 4 * M.R + g * M.C * M.n + b);
      }
    }
    // the exact guard on up to 64 (record, bag entry) pairs of the survivor list; a lane takes a pair of any record
    auto process = [&](u32 first, u32 count) {
      lds_wave_sync();
      u32 mask = 0;
      int kind0 = 0, pp = 0, j = 0;
      if ((u32)lane < count) {
        const u32 e = s_surv[first + (u32)lane];
        pp = (int)(e >> 8);
        j = (int)(e & 255);
        mask = Ops::guard(M, (const u64*)(s_rec + pp * stride), M.m0 + j, &kind0);
      }
      const bool en0 = (mask & 1u) != 0;
#pragma unroll
      for (int a = 1; a < 16; a++)
        if ((RECV >> a) & 1u) cnt[a] += (u32)__popcll(__ballot(en0 && kind0 == a));
      const bool foot0 = en0 && ((FOOT >> kind0) & 1u) != 0;
      if (mask) s_alive[pp] = 1;
      if (en0 && !foot0) s_nonfp[pp] = 1;
      const u64 pidx = p_base + (u64)pp;
      const int ordbase = M.m0 + j * (M.R + 1);
      push(foot0, pscan_entry(pidx, ordbase, kind0));
      if (__ballot((mask >> 1) != 0)) {                          // SendGetState(r, d, m), one bit per destination (rare)
#pragma unroll
        for (int d = 1; d <= 3; d++)
          if (d <= M.R) {
            const bool on = ((mask >> d) & 1u) != 0;
            cnt[A_SendGetState] += (u32)__popcll(__ballot(on));
            if ((FOOT >> A_SendGetState) & 1u) push(on, pscan_entry(pidx, ordbase + d, A_SendGetState));
            else if (on) s_nonfp[pp] = 1;
          }
      }
    };
    // the bag: prefilter (delivery count > 0 and one bit of the destination's table) on four entries of every record per trip
    int maxbag = nmsg;
#pragma unroll
    for (int s = 1; s < PSCAN_MT; s <<= 1) {
      const int o = __shfl_xor(maxbag, s);
      maxbag = o > maxbag ? o : maxbag;
    }
    maxbag = __builtin_amdgcn_readfirstlane(maxbag);
    u32 nsurv = 0;
    for (int jj = 0; jj < maxbag; jj += 4) {
      const int j = jj + g;
      bool pass = false;
      if (j < nmsg) {                                            // (nmsg is 0 for an invalid record)
        const u64 w = rec[M.fixed + j];
        const int r = m_dest(w);
        const u64 l = r == 1 ? lut[1] : r == 2 ? lut[2] : lut[3];
        pass = m_count(w) != 0 && ((l >> (w & 63)) & 1);
        if (m_count(w) == 3) s_limit[p] = 1;                     // one more Send of this key would not fit the count field
      }
      const u64 bal = __ballot(pass);
      if (bal) {
        if (pass) s_surv[nsurv + (u32)__popcll(bal & lt_mask)] = (unsigned short)((p << 8) | j);
        nsurv += (u32)__popcll(bal);
        if (nsurv >= 64) { nsurv -= 64; process(nsurv, 64u); }
      }
    }
    if (nsurv) process(0u, nsurv);
    lds_wave_sync();
    {
      const bool v16 = lane < np && s_ref[lane & (PSCAN_MT - 1)] != 0 && lane < PSCAN_MT;
      ndead += (u32)__popcll(__ballot(v16 && s_alive[lane & (PSCAN_MT - 1)] == 0));
      // LevelCtl::limit_unchecked, per record: a record at a representation limit with an enabled instance the footprint filter does not apply
      nlimit += (u32)__popcll(__ballot(v16 && s_limit[lane & (PSCAN_MT - 1)] != 0 && s_nonfp[lane & (PSCAN_MT - 1)] != 0));
    }
    lds_wave_sync();                                             // the flags and the records are rewritten at the top of the loop
    mt0 = mt1;
    mt1 = mt2;
  }
  if (nout) flush();
  // ---- epilogue: the four waves' counters through LDS, one set of global atomics per block
  {
    u32 mine = 0;
#pragma unroll
    for (int a = 0; a < 16; a++)
      if (lane == a) mine = cnt[a];
    if (lane == 16) mine = ndead;
    if (lane == 17) mine = nlimit;
    if (lane < 18 && mine) atomicAdd(&s_sum[lane], mine);
    __syncthreads();
    if (threadIdx.x < 16 && s_sum[threadIdx.x]) {
      atomicAdd((unsigned long long*)&ctl->act_generated[threadIdx.x], (unsigned long long)s_sum[threadIdx.x]);
      atomicAdd((unsigned long long*)&ctl->generated, (unsigned long long)s_sum[threadIdx.x]);
    }
    if (threadIdx.x == 16 && s_sum[16]) atomicAdd((unsigned long long*)&ctl->deadlocks, (unsigned long long)s_sum[16]);
    if (threadIdx.x == 17 && s_sum[17]) atomicAdd((unsigned long long*)&ctl->limit_unchecked, (unsigned long long)s_sum[17]);
  }
}

// The footprint instances k_probe_scan listed, one lane per entry (the list's counter is read on the device: no host round trip between the two kernels).
template <int SPEC>
__global__ void __launch_bounds__(VSR_BLOCK)
k_probe_apply(Model Marg, const u64* __restrict__ src_words, const u64* __restrict__ src_off, const u64* __restrict__ list, u64 list_cap, u64* pending,
              u64 pending_cap, LevelCtl* ctl) {
  typedef ModelOps<SPEC / 1000> Ops;
  Model M = Marg;
  specialise<SPEC>(M, Marg);
  const u64 n = list[0] < list_cap ? list[0] : list_cap;        // (more than the list holds: the host discards this pass)
  for (u64 i = (u64)blockIdx.x * VSR_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * VSR_BLOCK) {
    const u64 e = list[PSCAN_LIST_HDR + i];
    const u64 pidx = origin_pidx(e);
    const int ord = (int)((e >> 40) & 0xFFFF), kind = (int)(e >> 56);
    const u64 ref = src_off[pidx];
    const u64* rec = src_words + (ref >> 8);
    Delta D;
    if (!Ops::template gen_<false>(M, rec, ord, D) || D.action != kind) {   // the guards of the enumeration and of gen<> disagree
      raise_error(ctl, ERR_INTERNAL, (pidx << 16) | (u64)ord);
      continue;
    }
    if (D.err) {
      raise_error(ctl, D.err, (pidx << 16) | (u64)ord);
      continue;
    }
    if (Ops::invariants(M, rec, D) != 0) {                      // written down for k_probe_resolve, like k_expand<.., EXPAND_PROBE> did
      const u64 k = atomicAdd((unsigned long long*)&ctl->n_pending, 1ull);
      if (k < pending_cap) { pending[2 * k] = origin_make(pidx, ord); pending[2 * k + 1] = 0; }
    }
  }
}

}  // namespace vsr
