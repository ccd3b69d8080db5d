// vsr_where.hpp — k_where: user-written state predicates (vsr_where_parse.hpp compiles them) evaluated on every record of a level.  A streaming scan
// with the shape of k_terminal (vsr_terminal.hpp): one lane per record, straight from global memory, grid-stride over whole waves,
// refs[i] == 0 = a hole.  It reads records only: nothing is applied, the seen-set is not touched, k_expand / k_terminal / k_select are not involved.
//
// The program is a straight-line postfix sequence of 32-bit ops (opcode << 24 | argument), the same for every lane: quantifiers over replicas, clients,
// Values, ranges and log indices were unfolded by the compiler, only quantifiers over DOMAIN messages remain as loops (W_MBEGIN .. W_MEND, at most two
// nested).  Ops are read at a wave-uniform address (scalar loads), dispatch is a uniform branch.  The operand stack lives in LDS, laid out
// [slot][lane] in 32-bit words: the stack pointer is uniform, so the 64 lanes of a wave touch 64 consecutive words — no bank conflict — and no
// runtime-indexed private array exists that would go to scratch.  A message loop runs to the wave's largest nmsg; a lane past its own bag does not fold
// its body value into the accumulator (it contributes the quantifier's neutral element).
//
// Output per exported predicate k < 8: bit k of an optional flag byte per record, an exact counter (wave ballots summed in scalar registers, one atomic
// per wave at the end), the smallest fingerprint that satisfies it (wave reduction, one atomicMin per wave with a hit) and, for records with any bit
// set, a (fingerprint, index, bits) triple appended wave-wise to a list of which the first list_cap that arrive are kept (WhereCtl::n_list = true number).
//
// One instantiation per model, as k_terminal<MODEL>: k_where<0> is VSR.tla's and compiles exactly what it compiled before; k_where<1> (VR_STATE_TRANSFER.tla)
// and k_where<2> (VR_APP_STATE.tla) add five ops for what those records store differently — an entry normalised from either encoding, the 9-bit log's length,
// m.log with its first_op domain, an application-state entry — behind `if constexpr (MODEL != 0)`.  The slots of the held DoViewChanges are plain W_LDBITS.
#pragma once
#include "vsr_model.hpp"

namespace vsr {

enum {
  W_END = 0,
  W_PUSH,      // arg: 24-bit signed immediate
  W_LDBITS,    // arg: word(8) | shift(6) << 8 | width(6) << 14 | primed(1) << 20 : (rec[word] >> shift) & mask; primed (step programs only): of the child's word
  W_LDM,       // arg: loop(1) | shift(6) << 1 | width(6) << 7 : the same of the current bag word of message loop `loop`
  W_LDMENT,    // arg: loop : m.message — the entry byte of a PrepareMsg, 0 for every other type
  W_ENTF,      // arg: 0 view_number, 1 operation (value index + 1), 2 client_id, 3 request_number : field of the entry byte on top; an absent entry (0) reads 0
  W_LOGLEN,    // number of entries of the 24-bit log on top
  W_POPC,
  W_ADD, W_SUB, W_DIV,
  W_EQ, W_NE, W_LT, W_LE, W_GT, W_GE,
  W_AND, W_OR, W_NOT, W_IMP,
  W_SEL,       // pops a, c, acc; pushes c ? a : acc
  W_MBEGIN,    // arg: pc of the matching W_MEND (12) | loop << 12 | forall << 13 | primed << 14 (step programs only: the loop runs over the child's bag)
  W_MEND,      // arg: loop | forall << 1 | pc of the first body op << 2 | primed << 14
  W_OUT,       // arg: k : pops a boolean into bit k of the result
  W_STEPACT,   // step programs only (vsr_step.hpp): pushes the action id of the pair
  // the analysis models (model_id 1, 2: vrst_actions.hpp / vras_actions.hpp), in k_where<1> / k_where<2> only.  A log entry there is [operation |-> v]; every
  // entry, wherever it is stored, is brought to ONE form before anything looks at it: value index + 1, 0 = absent.
  W_ENTN,      // arg: 0 the replica-side entry (1 | value << 1, 3 bits) on top, 1 the message-side entry byte (1 | value << 3) on top : -> value + 1, or 0
  W_BLOGLEN,   // number of entries of the 9-bit log (3 entries x 3 bits) on top
  W_MLOGENT,   // arg: loop(1) | i(2) << 1, i in 1..3 : m.log[i] normalised — of a DoViewChangeMsg / StartViewMsg the sequence's entry i, of a NewStateMsg the
               // entry i with first_op <= i <= op_number, 0 for every other type and outside the domain
  W_MLOGLEN,   // arg: loop : the number of entries m.log holds (the sum of W_MLOGENT != 0 over i)
  W_APPENT,    // arg: word(8) | i(2) << 8 | primed(1) << 20 : rep_app_state[r][i] normalised, read from the A word rec[word] (primed, step programs only: of the
               // child's word — entry and commit number of the same side): present iff i <= commit number (model 2)
  W_OPCOUNT
};
enum { WHERE_MAX_OPS = 4096, WHERE_MAX_DEPTH = 32, WHERE_MAX_EXPORTS = 8 };

VSR_HD u32 w_op(int code, u32 arg) { return ((u32)code << 24) | (arg & 0xFFFFFFu); }

#if defined(__HIP_DEVICE_COMPILE__)
#define VSR_WHERE_UNI(x) ((u32)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define VSR_WHERE_UNI(x) (x)
#endif

// what a state program runs over: one record, no successor.  A step program (vsr_step.hpp) passes a pair view instead: is_pair = true, word(w) = word w
// of the child, msg(j) = bag word j of the child, nmsg_c = the child's bag size, action = the action id.  Everything that looks at the pair is under
// `if constexpr (PAIR::is_pair)`: k_where's instantiation contains none of it.
struct WhereNoPair { static constexpr bool is_pair = false; };

// One record through the program.  `S` is the operand stack (S[slot] -> int&); valid = the lane has a record; wmax = the largest nmsg of the lanes that
// run together (on the host: nmsg).  Returns the exported bits.
// m.log[i] of the bag word w, normalised (W_MLOGENT)
VSR_HD int where_mlog_entry(u64 w, int i) {
  const int t = m_type(w);
  const bool in_dom = t == T_DVC || t == T_SV || (t == T_NEWSTATE && i >= m_first_op(w) && i <= m_op(w));
  const int b = (int)((m_lg(w) >> (8 * (i - 1))) & 0xFF);
  return (in_dom && (b & 7)) ? ((b >> 3) & 3) + 1 : 0;
}

// MODEL: the model id the program was compiled for.  0 (VSR.tla) compiles none of the analysis models' ops.  W_MLOGENT / W_MLOGLEN read the loop's current bag word,
// whichever bag the loop runs over; W_ENTN and W_BLOGLEN work on the value on top: the four are the same in a step program.
template <typename STACK, typename PTR, typename PAIR = WhereNoPair, int MODEL = 0>
VSR_HD u32 where_run(const u32* __restrict__ prog, int fixed, PTR rec, bool valid, int nmsg, int wmax, STACK& S, const PAIR& pair = PAIR()) {
  u32 bits = 0;
  int sp = 0, pc = 0;
  int j0 = 0, j1 = 0, acc0 = 0, acc1 = 0;
  u64 mw0 = 0, mw1 = 0;
  // bag word j of the loop's bag and that bag's size, for this lane (a state program: always the record's own bag)
  auto bag_n = [&](u32 primed) -> int {
    if constexpr (PAIR::is_pair) return primed ? pair.nmsg_c : nmsg;
    else { (void)primed; return nmsg; }
  };
  auto bag_word = [&](u32 primed, int j) -> u64 {
    if constexpr (PAIR::is_pair) { if (primed) return (valid && j < pair.nmsg_c) ? pair.msg(j) : (u64)0; }
    else (void)primed;
    return (valid && j < nmsg) ? rec[fixed + j] : (u64)0;
  };
  for (;;) {
    const u32 op = VSR_WHERE_UNI(prog[pc]);
    pc++;
    const u32 arg = op & 0xFFFFFFu;
    switch (op >> 24) {
      case W_END: return bits;
      case W_PUSH: S[sp++] = (int)(arg << 8) >> 8; break;
      case W_LDBITS: {
        u64 w = valid ? rec[arg & 0xFF] : (u64)0;
        if constexpr (PAIR::is_pair) { if (valid && ((arg >> 20) & 1)) w = pair.word((int)(arg & 0xFF)); }
        S[sp++] = (int)((u32)(w >> ((arg >> 8) & 63)) & (u32)((((u64)1) << ((arg >> 14) & 63)) - 1));
        break;
      }
      case W_LDM: {
        const u64 w = (arg & 1) ? mw1 : mw0;
        S[sp++] = (int)((u32)(w >> ((arg >> 1) & 63)) & (u32)((((u64)1) << ((arg >> 7) & 63)) - 1));
        break;
      }
      case W_LDMENT: {
        const u64 w = (arg & 1) ? mw1 : mw0;
        S[sp++] = m_type(w) == T_PREPARE ? (int)(m_lg(w) & 0xFF) : 0;
        break;
      }
      case W_ENTF: {
        const int b = S[sp - 1];
        const int f = arg == 0 ? (b & 7) : arg == 1 ? entry_val(b) + 1 : arg == 2 ? entry_client(b) : entry_req(b);
        S[sp - 1] = b ? f : 0;
        break;
      }
      case W_LOGLEN: S[sp - 1] = log_len((u32)S[sp - 1]); break;
      case W_POPC: {
        u32 x = (u32)S[sp - 1];
        int n = 0;
        for (int k = 0; k < 8; k++) n += (int)((x >> k) & 1);
        S[sp - 1] = n;
        break;
      }
      case W_NOT: S[sp - 1] = S[sp - 1] ? 0 : 1; break;
      case W_SEL: {
        const int a = S[sp - 1], c = S[sp - 2], acc = S[sp - 3];
        sp -= 2;
        S[sp - 1] = c ? a : acc;
        break;
      }
      case W_MBEGIN: {
        const int forall = (int)((arg >> 13) & 1);
        const u32 pr = (arg >> 14) & 1;
        if ((arg >> 12) & 1) { j1 = 0; acc1 = forall; mw1 = bag_word(pr, 0); }
        else { j0 = 0; acc0 = forall; mw0 = bag_word(pr, 0); }
        if (wmax == 0) { S[sp++] = forall; pc = (int)(arg & 0xFFF) + 1; }
        break;
      }
      case W_MEND: {
        const int forall = (int)((arg >> 1) & 1);
        const int v = S[--sp];
        const u32 pr = (arg >> 14) & 1;
        const int nm = bag_n(pr);
        if (arg & 1) {
          if (j1 < nm) acc1 = forall ? (acc1 & v) : (acc1 | v);
          j1++;
          if (j1 < wmax) { mw1 = bag_word(pr, j1); pc = (int)((arg >> 2) & 0xFFF); }
          else S[sp++] = acc1;
        } else {
          if (j0 < nm) acc0 = forall ? (acc0 & v) : (acc0 | v);
          j0++;
          if (j0 < wmax) { mw0 = bag_word(pr, j0); pc = (int)((arg >> 2) & 0xFFF); }
          else S[sp++] = acc0;
        }
        break;
      }
      case W_OUT: bits |= (S[--sp] ? 1u : 0u) << (arg & 7); break;
      default: {                                                    // the binary operators
        if constexpr (PAIR::is_pair) {
          if ((op >> 24) == W_STEPACT) { S[sp++] = pair.action; break; }
        }
        if constexpr (MODEL != 0) {
          const u32 code = op >> 24;
          if (code >= (u32)W_ENTN) {
            if (code == W_ENTN) {
              const int e = S[sp - 1];
              S[sp - 1] = (arg & 1) ? ((e & 7) ? ((e >> 3) & 3) + 1 : 0) : ((e & 1) ? ((e >> 1) & 3) + 1 : 0);
            } else if (code == W_BLOGLEN) {
              const int lg = S[sp - 1];
              S[sp - 1] = (lg & 1) + ((lg >> 3) & 1) + ((lg >> 6) & 1);
            } else if (code == W_MLOGENT) {
              S[sp++] = where_mlog_entry((arg & 1) ? mw1 : mw0, (int)((arg >> 1) & 3));
            } else if (code == W_MLOGLEN) {
              const u64 w = (arg & 1) ? mw1 : mw0;
              S[sp++] = (where_mlog_entry(w, 1) != 0) + (where_mlog_entry(w, 2) != 0) + (where_mlog_entry(w, 3) != 0);
            } else {                                                  // W_APPENT
              u64 A = valid ? rec[arg & 0xFF] : (u64)0;
              if constexpr (PAIR::is_pair) { if (valid && ((arg >> 20) & 1)) A = pair.word((int)(arg & 0xFF)); }
              const int i = (int)((arg >> 8) & 3);
              S[sp++] = i <= a_commit(A) ? (int)((A >> (34 + 2 * (i - 1))) & 3) + 1 : 0;
            }
            break;
          }
        }
        const int b = S[--sp], a = S[sp - 1];
        int r = 0;
        switch (op >> 24) {
          case W_ADD: r = a + b; break;
          case W_SUB: r = a - b; break;
          case W_DIV: {                                             // TLA+'s \div rounds towards minus infinity; a zero divisor gives 0
            if (b != 0) { r = a / b; if ((a % b != 0) && ((a < 0) != (b < 0))) r--; }
            break;
          }
          case W_EQ: r = a == b; break;
          case W_NE: r = a != b; break;
          case W_LT: r = a < b; break;
          case W_LE: r = a <= b; break;
          case W_GT: r = a > b; break;
          case W_GE: r = a >= b; break;
          case W_AND: r = (a != 0) & (b != 0); break;
          case W_OR: r = (a != 0) | (b != 0); break;
          case W_IMP: r = (a == 0) | (b != 0); break;
        }
        S[sp - 1] = r;
      }
    }
  }
}

#if defined(__HIPCC__)

struct WhereCtl {
  u64 scanned;                        // records looked at (holes excluded)
  u64 count[WHERE_MAX_EXPORTS];       // records that satisfy predicate k
  u64 min_fp[WHERE_MAX_EXPORTS];      // the smallest fingerprint among them, ~0 = none
  u64 n_list;                         // records with any bit set offered to the list
};

struct WhereLdsStack {                // [slot][lane of the block]
  int* base;
  __device__ __forceinline__ int& operator[](int slot) const { return base[slot * 256]; }
};

template <int MODEL>
__global__ void __launch_bounds__(256)
k_where(Model M, const u32* __restrict__ prog, int n_exports, const u64* __restrict__ words, const u64* __restrict__ refs, const u64* __restrict__ fps,
        u64 n, uint8_t* flags, WhereCtl* ctl, u64* list, u64 list_cap) {
  __shared__ int stack[WHERE_MAX_DEPTH * 256];
  WhereLdsStack S{stack + threadIdx.x};
  u32 cnt[WHERE_MAX_EXPORTS];                                      // wave-uniform (ballot popcounts); indexed by unrolled constants only
#pragma unroll
  for (int k = 0; k < WHERE_MAX_EXPORTS; k++) cnt[k] = 0;
  u32 n_scanned = 0;
  const u64 step = (u64)gridDim.x * blockDim.x;
  const u64 n_round = (n + 63) & ~(u64)63;                         // whole waves stay together
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += step) {
    const u64 ref = i < n ? refs[i] : 0;
    const bool valid = ref != 0;
    const u64* rec = words + (ref >> 8);
    const int nmsg = valid ? hdr_nmsg(rec[0]) : 0;
    const int wmax = wave_max_uniform(nmsg);
    const u32 raw = where_run<WhereLdsStack, const u64*, WhereNoPair, MODEL>(prog, M.fixed, rec, valid, nmsg, wmax, S);
    const u32 bits = valid ? raw : 0;                              // (a lane without a record ran the program over zeros: TRUE would count it)
    if (valid && flags) flags[i] = (uint8_t)bits;
    n_scanned += (u32)__popcll(__ballot(valid));
    if (__ballot(bits != 0) == 0) continue;                        // (wave-uniform)
#pragma unroll
    for (int k = 0; k < WHERE_MAX_EXPORTS; k++) {
      if (k >= n_exports) break;
      const bool hit = (bits >> k) & 1;
      const u64 b = __ballot(hit);
      if (b == 0) continue;
      cnt[k] += (u32)__popcll(b);
      if (fps) {
        const u64 m = wave_min64(hit ? fps[i] : ~(u64)0);
        if (lane_id() == 0) atomicMin((unsigned long long*)&ctl->min_fp[k], (unsigned long long)m);
      }
    }
    if (fps && list && bits != 0) {
      const u64 k = wave_alloc(&ctl->n_list);
      if (k < list_cap) {
        list[3 * k] = fps[i];
        list[3 * k + 1] = i;
        list[3 * k + 2] = (u64)bits;
      }
    }
  }
  if (lane_id() == 0) {                                            // one atomic per counter and wave
    if (n_scanned) atomicAdd((unsigned long long*)&ctl->scanned, (unsigned long long)n_scanned);
#pragma unroll
    for (int k = 0; k < WHERE_MAX_EXPORTS; k++)
      if (cnt[k]) atomicAdd((unsigned long long*)&ctl->count[k], (unsigned long long)cnt[k]);
  }
}

#endif  // __HIPCC__

}  // namespace vsr
