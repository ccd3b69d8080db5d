// vsr_regen_bits.hpp — the regenerating pass of the deep search over the claim bitmap as a kernel of its own (VSR.tla configurations with R <= 3).
//
// The pass that inserted the first seen-set-only level left one bit per (parent of the stored base, ordinal) whose lane made a state (vsr_deep.hpp).  A
// regenerating pass rebuilds exactly those states: no guards, no bag scans, no seen-set access and no invariants (the virtual pass checked them when it
// inserted the level; a violation there ends the search before anything is regenerated) — one gen<>, one hash, one record written per set bit.
// k_expand<true, SPEC, EXPAND_REGEN_BITS> does that inside the general tile loop: 64 records and six or more block barriers per tile, for 112 instances on the
// README configuration.  Here a wave owns a mini-tile of 16 parents, as in k_probe_scan: nothing is shared between the waves of a block and no block barrier
// stands in the loop.  The set bits of the 16 bitmap rows ARE the work list: a prefix sum over the lanes' popcounts hands every lane of a trip one
// (parent, ordinal), densely; the children of a trip are packed into the wave's own chunks of the destination by a prefix sum over their lengths.
// The order of the records inside a regenerated slice differs from k_expand's; nothing a caller sees depends on it.
#pragma once
#include "vsr_kernels.hpp"
#define REGEN_ORD_FN __host__ __device__ __forceinline__
#include "regen_ord.hpp"

// Two choices were measured on the README configuration (the eleven regenerating passes of a run; k_expand<true, 313, EXPAND_REGEN_BITS>: 108.3 ms;
// profiles/regen_bits_bench.txt) and only the winners are in this file:
//   the store shape   the parent words of a trip's children are copied by the whole wave, lane k moving word k of one record per instruction, and the owning
//                     lane patches on top: 87.7 ms.  Every lane copying its own child's parent, 16 bytes per store (what k_expand's regenerating instantiation
//                     does, and where the cooperative copy LOST 13 %) took 123.0 ms — here every lane of a trip writes and no wave idles meanwhile.
//   the prefetch      refs and bitmap rows of the next mini-tile are in registers before the current one is processed; its record words are loaded at the top
//                     of the loop, the other three waves of the SIMD cover the latency.  Prefetching the words too holds 32 registers across gen<> and the hash,
//                     of which the README configuration's instantiation (six permutations) spilled 30 (120 bytes of scratch per lane): 130.1 ms.

namespace vsr {

constexpr int RGB_MT = 16;              // parents of a mini-tile: 16 lanes per record while staging, 4 lanes per bitmap row
constexpr int RGB_DRAW = 16;            // mini-tiles per draw from LevelCtl::tile_cursor: 256 parents per returning atomic on that address
constexpr int RGB_ROW_WORDS = 8;        // bitmap words per parent the kernel handles: two per lane (deep_claim_bits_alloc offers no more)
constexpr int RGB_WAVE_EXTRA = RGB_MT + 64 / 2 + 2 * 64 / 2;   // u64 words of a wave's LDS region beside its 16 records: refs, 64 prefix sums, 128 bitmap words
constexpr u32 RGB_ICHUNK = 512;         // indices / words of the destination a wave reserves per atomic on n_new / words_new: a mini-tile of the README configuration
constexpr u32 RGB_WCHUNK = 32768;       // yields 28 children of 45 words — one reservation of either kind per 18 / 26 mini-tiles
__host__ __device__ __forceinline__ size_t rgb_lds_bytes(int stride) { return (size_t)(VSR_BLOCK / 64) * (size_t)(RGB_MT * stride + RGB_WAVE_EXTRA) * 8; }

template <int SPEC>
__global__ void __launch_bounds__(VSR_BLOCK, VSR_OCC)
k_regen_bits(Model Marg, const u64* __restrict__ fr_words, const u64* __restrict__ fr_off, u64 n_parents, u64 p_offset /* index of parent 0 in its level: the bitmap's row */,
             const u32* __restrict__ claim_bits, u32 claim_w, LevelCtl* ctl, int stride, u32 draw /* mini-tiles per draw, the same in every wave of the launch */,
             u32 trip /* instances a wave takes per trip, 1 .. 64 */, u64* nx_words, u64 nx_words_cap, u64* nx_off, u64 nx_cap, u64* lvl_fp,
             u32 ichunk /* >= 64 */, u32 wchunk /* >= 64 records of the longest kind */) {
  static_assert(SPEC / 1000 == 0 && SPEC % 1000 != 0 && (SPEC % 1000) / 100 <= 3, "VSR.tla, R <= 3: a record fits 64 words");
  typedef ModelOps<0> Ops;
  Model M = Marg;
  specialise<SPEC>(M, Marg);
  extern __shared__ u64 smem[];
  __shared__ unsigned long long s_sum[3];                        // the block's counters, added up once, in the epilogue: records written, their words, the largest bag
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64* const s_rec = smem + wave * (RGB_MT * stride + RGB_WAVE_EXTRA);   // this wave's records ...
  u64* const s_ref = s_rec + RGB_MT * stride;                   // ... their refs
  u32* const s_pre = (u32*)(s_ref + RGB_MT);                    // ... per lane: the set bits of lanes 0 .. lane (inclusive)
  u32* const s_bits = s_pre + 64;                               // ... per lane: its two bitmap words
  if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
  __syncthreads();

  const u64 nmt = (n_parents + RGB_MT - 1) / RGB_MT;
  const u64 lt_mask = ((u64)1 << lane) - 1;
  u64 n_written = 0, rec_words = 0;                             // wave-uniform
  u32 maxbag = 0;                                               // per lane
  // this wave's chunks of the destination (wave-uniform): indices [idx_base, idx_base + idx_left), words [w_base, w_base + w_left)
  u64 idx_base = 0, w_base = 0;
  u32 idx_left = 0, w_left = 0;

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
  // staging, 16 lanes per record: a lane moves words l16, l16 + 16, .. of records q, q + 4, q + 8, q + 12.  A lane keeps ONE ref of a mini-tile across the
  // work (record l16's) and gets the four it stages by from the lanes that hold them: 2 registers per prefetched mini-tile instead of 8
  const int l16 = lane & 15, q0 = lane >> 4;
  auto load_ref = [&](u64 mt) -> u64 {
    const u64 idx = mt * RGB_MT + (u64)l16;
    return (mt < nmt && idx < n_parents) ? fr_off[idx] : 0;
  };
  auto spread = [&](u64 ref1, u64* refq) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const u32 lo = (u32)__shfl((int)(u32)ref1, q0 + 4 * q), hi = (u32)__shfl((int)(u32)(ref1 >> 32), q0 + 4 * q);
      refq[q] = ((u64)hi << 32) | lo;
    }
  };
  auto load_words = [&](u64 ref1, u64 (*v)[4]) {
    u64 refq[4];
    spread(ref1, refq);
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
  // the bitmap, 4 lanes per row: lane 4 p + w holds words w and w + 4 of parent p's row
  const int bp = lane >> 2, bw = lane & 3;
  auto load_bits = [&](u64 mt, u32* cb) {
    const u64 idx = mt * RGB_MT + (u64)bp;
    cb[0] = cb[1] = 0;
    if (mt < nmt && idx < n_parents) {
      const u32* row = claim_bits + (p_offset + idx) * (u64)claim_w;
      if ((u32)bw < claim_w) cb[0] = row[bw];
      if ((u32)bw + 4 < claim_w) cb[1] = row[bw + 4];
    }
  };

  u64 refA, refB, v[4][4];
  u32 cbA[2], cbB[2];
  u64 mt0 = next_mt();
  refA = load_ref(mt0);
  load_bits(mt0, cbA);
  u64 mt1 = next_mt();
  refB = load_ref(mt1);
  while (mt0 < nmt) {
    // ---- this mini-tile's words into LDS; the next one's bitmap rows and the refs of the one after are issued before the work starts
    load_words(refA, v);
    {
      u64 refq[4];
      spread(refA, refq);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int p = q0 + 4 * q;
        const int len = (int)(refq[q] & 255) < stride ? (int)(refq[q] & 255) : stride;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int k = l16 + 16 * j;
          if (k < len) s_rec[p * stride + k] = v[q][j];
        }
      }
      if (lane < RGB_MT) s_ref[lane] = refA;
    }
    const u32 cb0 = cbA[0], cb1 = cbA[1];
    load_bits(mt1, cbB);
    refA = refB;
    cbA[0] = cbB[0];
    cbA[1] = cbB[1];
    const u64 mt2 = next_mt();
    refB = load_ref(mt2);
    lds_wave_sync();

    // ---- the work list: the set bits of the 16 rows, counted per lane and summed over the wave
    const u64 p_base = mt0 * RGB_MT;
    u32 total;
    {
      const u64 ref = s_ref[bp];
      const bool fits = (int)(ref & 255) <= stride;                // (LDS slots sized for shorter records: an error, and nothing of such a parent is written)
      const bool valid = p_base + (u64)bp < n_parents && ref != 0 && fits;   // ref 0: a hole a chunk tail of the stored level left — it has no bits and yields nothing
      if (!fits && bw == 0) raise_error(ctl, ERR_INTERNAL, (p_base + (u64)bp) << 16);
      const u32 b0 = valid ? cb0 : 0u, b1 = valid ? cb1 : 0u;
      u32 incl = (u32)__popc(b0) + (u32)__popc(b1);
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const u32 t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
      }
      s_pre[lane] = incl;
      s_bits[2 * lane] = b0;
      s_bits[2 * lane + 1] = b1;
      total = (u32)__builtin_amdgcn_readlane((int)incl, 63);
    }
    lds_wave_sync();

    for (u32 first = 0; first < total; first += trip) {
      // ---- instance first + lane: the lane that holds its bit (the first whose inclusive sum exceeds it), then the bit
      const bool active = (u32)lane < trip && first + (u32)lane < total;
      const u32 i = active ? first + (u32)lane : 0u;
      int L = 0;
#pragma unroll
      for (int s = 32; s > 0; s >>= 1)
        if (s_pre[L + s - 1] <= i) L += s;
      u32 k = i - (L ? s_pre[L - 1] : 0u);
      u64 w = (u64)s_bits[2 * L] | ((u64)s_bits[2 * L + 1] << 32);
      if (!active) { w = 1; k = 0; }
      for (; k; k--) w &= w - 1;
      const int b = __ffsll((long long)w) - 1;
      const int p = L >> 2;
      const int ord = 32 * ((L & 3) + (b >= 32 ? 4 : 0)) + (b & 31);
      const u64* rec = s_rec + p * stride;

      // ---- the action id from the ordinal (regen_ord.hpp), the successor, its view hashes and fingerprint
      bool ok = active;
      Delta D;
      u64 Hc[6];
      u64 fp = 0;
      int plen = 0, clen = 0;
      if (active) {
        const RegenOrd o = regen_ord(M.R, M.C, M.n, ord);
        int kind;
        if (o.cls != REGEN_ORD_MESSAGE) {
          kind = o.cls == REGEN_ORD_TIMER_SEND_SVC ? A_TimerSendSVC : o.cls == REGEN_ORD_SEND_DVC ? A_SendDVC : o.cls == REGEN_ORD_SEND_SV ? A_SendSV
               : o.cls == REGEN_ORD_EXECUTE_OP ? A_ExecuteOp : A_ReceiveClientRequest;
        } else {
          int kind0 = 0;
          (void)Ops::guard(M, rec, M.m0 + o.j, &kind0);
          kind = o.k2 == 0 ? kind0 : Ops::other_kind(kind0);
        }
        if (!Ops::template gen_<false>(M, rec, ord, D) || D.action != kind) {
          raise_error(ctl, ERR_INTERNAL, ((p_base + (u64)p) << 16) | (u64)ord);
          ok = false;
        } else if (D.err) {
          raise_error(ctl, D.err, ((p_base + (u64)p) << 16) | (u64)ord);
          ok = false;
        }
      }
      if (ok) {
        Ops::hash_child_(M, rec, D, Hc);
        u32 ak;
        canonical_fp(M, D.hdr, Hc, &fp, &ak);
        plen = (int)(s_ref[p] & 255);
        clen = M.fixed + hdr_nmsg(D.hdr);
        if ((u32)hdr_nmsg(D.hdr) > maxbag) maxbag = (u32)hdr_nmsg(D.hdr);
      }

      // ---- room in the wave's chunks: an index per child, its words packed behind the words of the lanes below
      const u64 okm = __ballot(ok);
      const u32 nwin = (u32)__popcll(okm);
      if (nwin == 0) continue;
      u32 wincl = (u32)clen;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const u32 t = __shfl_up(wincl, o);
        if (lane >= o) wincl += t;
      }
      const u32 wtotal = (u32)__builtin_amdgcn_readlane((int)wincl, 63);
      if (idx_left < nwin) {                                     // the rest of the old index chunk: invalid refs, like the tail of a block's chunk in k_expand
        for (u32 t = (u32)lane; t < idx_left; t += 64) { nx_off[idx_base + t] = 0; lvl_fp[idx_base + t] = 0; }
        u64 nb = 0;
        if (lane == 0) {
          nb = atomicAdd((unsigned long long*)&ctl->n_new, (unsigned long long)ichunk);
          if (nb + ichunk > nx_cap) { raise_full(ctl, nb); nb = 0; }   // keep writing inside the buffer; nothing but records is lost
        }
        idx_base = readlane64(nb, 0);
        idx_left = ichunk;
      }
      const u64 idx = idx_base + (u64)__popcll(okm & lt_mask);
      idx_base += nwin;
      idx_left -= nwin;
      // records do not straddle word chunks: the lanes whose children still fit the old chunk stay there, the others start a new one
      const u64 fitm = __ballot(wincl <= w_left);                // (monotone: a prefix of the lanes)
      const u32 cut = fitm ? (u32)__builtin_amdgcn_readlane((int)wincl, 63 - __clzll((long long)fitm)) : 0u;
      u64 dst = w_base + (u64)(wincl - (u32)clen);
      if (cut < wtotal) {
        u64 nb = 0;
        if (lane == 0) {
          nb = atomicAdd((unsigned long long*)&ctl->words_new, (unsigned long long)wchunk);
          if (nb + wchunk > nx_words_cap) { raise_full(ctl, nb); nb = 0; }
        }
        nb = readlane64(nb, 0);
        if (wincl > cut) dst = nb + (u64)(wincl - (u32)clen - cut);
        w_base = nb + (u64)(wtotal - cut);
        w_left = wchunk - (wtotal - cut);
      } else {
        w_base += wtotal;
        w_left -= wtotal;
      }
      n_written += nwin;
      rec_words += wtotal;

      // ---- the child: the parent's words from LDS by the whole wave, lane k moving word k, then the Delta's patches on top by the owning lane (same wave,
      // program order): the layout write_child_serial specifies
      for (u64 wm = okm; wm;) {                                  // two records per trip: their LDS reads are in flight together
        const int l0 = __ffsll((long long)wm) - 1;
        wm &= wm - 1;
        const int l1 = wm ? __ffsll((long long)wm) - 1 : l0;
        wm &= wm - 1;
        const int n0 = __builtin_amdgcn_readlane(plen, l0), n1 = l1 != l0 ? __builtin_amdgcn_readlane(plen, l1) : 0;
        const u64* r0 = s_rec + __builtin_amdgcn_readlane(p, l0) * stride;
        const u64* r1 = s_rec + __builtin_amdgcn_readlane(p, l1) * stride;
        u64* o0 = nx_words + readlane64(dst, l0);
        u64* o1 = nx_words + readlane64(dst, l1);
        for (int t = lane; t < n0 || t < n1; t += 64) {
          const u64 v0 = t < n0 ? r0[t] : 0, v1 = t < n1 ? r1[t] : 0;
          if (t < n0) o0[t] = v0;
          if (t < n1) o1[t] = v1;
        }
      }
      if (ok) {
        u64* out = nx_words + dst;
        out[0] = D.hdr;
        u64* ob = out + 1 + (D.r - 1) * M.wpr;
        ob[0] = D.rep[0];
        if (M.wpr > 1) ob[1] = D.rep[1];
        if (M.wpr > 2) ob[2] = D.rep[2];
        if (M.wpr > 3) ob[3] = D.rep[3];
#pragma unroll
        for (int h = 0; h < 6; h++)
          if (h < M.np) out[M.h0 + h] = Hc[h];
        int a = 0;
#pragma unroll
        for (int s = 0; s < VSR_NSLOT; s++)
          if ((D.used >> s) & 1) {
            if (D.pj(s) >= 0) out[M.fixed + D.pj(s)] = D.pnew[s];
            else out[plen + (a++)] = D.pnew[s];
          }
        nx_off[idx] = (dst << 8) | (u64)clen;
        lvl_fp[idx] = fp;
      }
    }
    lds_wave_sync();                                             // the records, the sums and the bitmap words are rewritten at the top of the loop
    mt0 = mt1;
    mt1 = mt2;
  }
  // ---- epilogue: the unused tail of the wave's index chunk as invalid refs; the four waves' counters through LDS, one set of global atomics per block
  for (u32 t = (u32)lane; t < idx_left; t += 64) { nx_off[idx_base + t] = 0; lvl_fp[idx_base + t] = 0; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u32 t = __shfl_down(maxbag, o);
    maxbag = t > maxbag ? t : maxbag;
  }
  if (lane == 0) {
    if (n_written) atomicAdd(&s_sum[0], (unsigned long long)n_written);
    if (rec_words) atomicAdd(&s_sum[1], (unsigned long long)rec_words);
    if (maxbag) atomicMax(&s_sum[2], (unsigned long long)maxbag);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_sum[0]) atomicAdd((unsigned long long*)&ctl->n_written, s_sum[0]);
  if (threadIdx.x == 1 && s_sum[1]) atomicAdd((unsigned long long*)&ctl->rec_words, s_sum[1]);
  if (threadIdx.x == 2 && s_sum[2]) atomicMax((unsigned long long*)&ctl->max_bag, s_sum[2]);
}

}  // namespace vsr
