// host_deep_terminal.hpp — the deadlock check on the levels beyond the record buffers: the TERMINAL ATTACHMENT of a checker, the three
// hooks a descent of the deep search calls beside the predicate attachment's (vsr_deep.hpp: deep_term_begin / _slice / _end), the per-level results and
// the witnesses (included by vsrmc.hip after host_deep_where.hpp: one translation unit, the sections share its anonymous-namespace helpers).
//
// Every state of a seen-set-only level sits once per descent in a scratch buffer as (words, off, fp, index range with holes): k_terminal's input, so the
// kernel runs unchanged over every slice.  A level K beyond the base is scanned in the FIRST descent after the attachment that regenerates or inserts it
// (the rule of host_deep_where.hpp); per level one TermCtl on the device, reset once per level: counters and the two minima accumulate over the slices, the
// list cursor n_list is each launch's.  The probed level has no records: k_probe_children (vsr_deep_terminal.hpp) materialises the fresh successors of
// every sub-slice of the inserted level, chunk by chunk, into a buffer of the attachment and k_terminal reads the chunk.  The slice hook allocates nothing.
#pragma once
#include <map>

struct DeepTermScan {
  int level = 0, kind = DEEP_KIND_REGEN;
  int exact = 1;
  u64 slices = 0;                      // scratch slices scanned (probed: instance lists consumed)
  u64 chunks = 0;                      // probed: k_probe_children launches; else = slices
  u64 n_states = 0;                    // states scanned (probed: fresh copies scanned)
  u64 n_terminal = 0, n_unsettled = 0;
  u64 min_fp = ~(u64)0, min_fp_unsettled = ~(u64)0;
  u64 n_listed = 0;                    // the true number offered to the list (probed: terminal copies offered)
  u64 bytes_written = 0;               // probed: bytes of child records k_probe_children wrote
  double ms = 0, children_ms = 0;      // host time around the launches: k_terminal (+ read-back); probed: k_step_list + k_probe_children beside it
  std::vector<u64> raw;                // while the descent runs: 3 words per kept entry (fingerprint, index | key, flags)
  std::vector<u64> fps, keys;          // published: fingerprints ascending (probed: the smallest key of each beside it)
  std::vector<uint8_t> flags;
};

struct vsrmc_deep_terminal {
  int scanned_through = 0;             // every level <= this one is either stored or has been scanned
  u64 list_cap = 0, inst_cap = 0, child_words = 0, child_idx = 0;
  DevMem mem;                          // the device buffers below: allocated once per attachment, freed with it
  TermCtl* d_ctl = nullptr;            // DEEP_MAX_LEVELS blocks: block i = level first + i of the descent in flight
  TermCtl* d_pctl = nullptr;           // the probed level's
  ProbeChildCtl* d_cctl = nullptr;
  StepCtl* d_sctl = nullptr;           // k_step_list's (its own listing: the predicate attachment's list is not shared)
  u64 *d_list = nullptr, *d_plist = nullptr, *d_inst = nullptr;
  u64 *d_child = nullptr, *d_refs = nullptr, *d_fps = nullptr, *d_keys = nullptr;
  // the descent in flight
  int first = 0;
  std::vector<DeepTermScan> cur;
  DeepTermScan probed;
  bool probe_skipped = false;
  std::vector<u64> h_keys;             // a chunk's keys, fetched when the chunk listed a terminal copy
  std::map<std::pair<int, int>, DeepTermScan> results;   // (level, 1 = as the probed level) -> figures
};

namespace {

void deep_term_free(vsrmc_checker* c) {
  if (!c->deep_term) return;
  delete c->deep_term;
  c->deep_term = nullptr;
}

void deep_term_restart(vsrmc_checker* c) {
  vsrmc_deep_terminal* A = c->deep_term;
  if (!A) return;
  A->scanned_through = 1;              // (checker_seed: level 1 is the stored level)
  A->cur.clear();
  A->results.clear();
}

TermCtl fresh_term_ctl() {
  TermCtl h;
  std::memset(&h, 0, sizeof(h));
  h.min_fp = h.min_fp_unsettled = ~(u64)0;
  return h;
}

// one launch of k_terminal that goes on from the block's counters and minima: only the list cursor is this launch's.  Appends what the launch kept (at most
// `cap` entries in S.raw over the level) and adds the true number.
int deep_term_launch(vsrmc_checker* c, vsrmc_deep_terminal* A, const u64* words, const u64* refs, const u64* fps, u64 n, TermCtl* ctl, u64* d_list, DeepTermScan& S,
                     u64* kept_out) {
  const Model& M = c->model.M;
  const u64 room = A->list_cap - std::min<u64>(A->list_cap, S.raw.size() / 3);
  HIPCHK(hipMemsetAsync(&ctl->n_list, 0, 8, c->stream));
  hipLaunchKernelGGL(KERNEL_OF(k_terminal, M), dim3(scan_grid(n, c->num_cus)), dim3(256), 0, c->stream, M, words, refs, fps, n, (uint8_t*)nullptr, ctl, d_list, room);
  HIPCHK(hipGetLastError());
  u64 n_list = 0;
  HIPCHK(hipMemcpyAsync(&n_list, &ctl->n_list, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  S.n_listed += n_list;
  const u64 kept = std::min<u64>(n_list, room);
  if (kept) {
    const size_t at = S.raw.size();
    S.raw.resize(at + 3 * kept);
    HIPCHK(hipMemcpy(S.raw.data() + at, d_list, kept * 24, hipMemcpyDeviceToHost));
  }
  if (kept_out) *kept_out = kept;
  return 0;
}

// before a descent that regenerates / inserts the levels up to last_level: one control block per level that has not been scanned yet
int deep_term_begin(vsrmc_checker* c, int last_level) {
  vsrmc_deep_terminal* A = c->deep_term;
  A->cur.clear();
  A->probed = DeepTermScan();
  A->probe_skipped = false;
  A->first = A->scanned_through + 1;
  if (last_level < A->first) return 0;
  const int n = last_level - A->first + 1;
  if (n > DEEP_MAX_LEVELS) return fail(VSRMC_E_REP, "deep terminal scan: more than 512 levels to scan in one descent");
  A->cur.resize((size_t)n);
  for (int i = 0; i < n; i++) A->cur[(size_t)i].level = A->first + i;
  const std::vector<TermCtl> t((size_t)n + 1, fresh_term_ctl());
  const StepCtl s = fresh_ctl<StepCtl>();
  HIPCHK(hipMemcpyAsync(A->d_ctl, t.data(), sizeof(TermCtl) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(A->d_pctl, t.data() + n, sizeof(TermCtl), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(A->d_sctl, &s, sizeof(StepCtl), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(A->d_cctl, 0, sizeof(ProbeChildCtl), c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));                         // (the sources are locals)
  return 0;
}

// the successors of the sub-slice B[0, part) of the inserted level `level` = a part of the probed level: materialised chunk by chunk, each chunk scanned
int deep_term_probe(vsrmc_checker* c, const PassDst& B, u64 part, int level, u64 bag) {
  vsrmc_deep_terminal* A = c->deep_term;
  const Model& M = c->model.M;
  DeepTermScan& P = A->probed;
  auto* const child_kernel = KERNEL_OF(k_probe_children, M);
  const int bag_bound = bag ? (int)std::min<u64>(bag, (u64)M.max_bag) : M.max_bag;
  // a launch covers the entries whose children fit the buffer whatever they are: a child's bag is its parent's plus the patch slots that append, at most max_bag
  // (a child over that carries ERR_REP_BAG and is not written)
  const u64 child_len = (u64)M.fixed + (u64)std::min(M.max_bag, bag_bound + VSR_NSLOT);
  const u64 per = std::min<u64>(A->child_idx, std::max<u64>(1, A->child_words / child_len));
  SlicePolicy sp(0, part, A->inst_cap, step_slice_default(M, bag_bound, A->inst_cap));
  const StepListing listing{B.words, B.off, c->stream, c->num_cus, A->d_inst, A->d_sctl};
  u64 scanned = 0;
  const double t0 = now_s();
  double term_ms = 0;
  const int rc = step_slices(M, listing, sp, "deep terminal scan", &scanned, nullptr, [&](u64, u64, u64 n_inst) -> int {
    P.slices++;
    for (u64 e = 0; e < n_inst; e += per) {
      const u64 e_hi = std::min<u64>(n_inst, e + per);
      HIPCHK(hipMemsetAsync(A->d_cctl, 0, 16, c->stream));         // n_idx, n_words: this launch's
      hipLaunchKernelGGL(child_kernel, dim3(scan_grid(e_hi - e, c->num_cus)), dim3(256), 0, c->stream, M, (const u64*)B.words, (const u64*)B.off, (const u64*)A->d_inst, e, e_hi,
                         (const Slot*)c->table, c->tmask, level + 1, A->d_child, A->child_words, A->d_refs, A->d_fps, A->d_keys, A->child_idx, A->d_cctl);
      HIPCHK(hipGetLastError());
      ProbeChildCtl h;
      HIPCHK(hipMemcpyAsync(&h, A->d_cctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      P.chunks++;
      if (h.dropped || h.n_idx > A->child_idx || h.n_words > A->child_words)
        return fail(VSRMC_E_HIP, "k_probe_children: " + std::to_string(h.dropped) + " successors did not fit the child buffer (" + std::to_string(e_hi - e) + " entries, " +
                                     std::to_string(A->child_words) + " words)");
      if (h.n_internal) return fail(VSRMC_E_HIP, "k_probe_children: " + std::to_string(h.n_internal) + " listed instances are not enabled (guard_slot_pre and gen disagree)");
      P.bytes_written += h.n_words * 8 + h.n_idx * 24;
      if (!h.n_idx) continue;
      const double t1 = now_s();
      const size_t at = P.raw.size();
      u64 kept = 0;
      const int r2 = deep_term_launch(c, A, A->d_child, A->d_refs, A->d_fps, h.n_idx, A->d_pctl, A->d_plist, P, &kept);
      if (r2) return r2;
      if (kept) {                                                  // a listed copy's key comes from the chunk's keys (the list holds its index in the chunk)
        // (terminal copies are rare: the keys of a few are fetched one by one, the chunk's whole key array only when many were listed)
        const bool whole = kept > 64;
        if (whole) {
          A->h_keys.resize((size_t)h.n_idx);
          HIPCHK(hipMemcpy(A->h_keys.data(), A->d_keys, h.n_idx * 8, hipMemcpyDeviceToHost));
        }
        for (u64 k = 0; k < kept; k++) {
          const u64 i = P.raw[at + 3 * k + 1];
          if (i >= h.n_idx) return fail(VSRMC_E_HIP, "k_terminal: a listed index beyond the chunk");
          if (whole) P.raw[at + 3 * k + 1] = A->h_keys[(size_t)i];
          else HIPCHK(hipMemcpy(&P.raw[at + 3 * k + 1], A->d_keys + i, 8, hipMemcpyDeviceToHost));
        }
      }
      term_ms += (now_s() - t1) * 1e3;
    }
    return 0;
  });
  if (rc) return rc;
  P.ms += term_ms;
  P.children_ms += (now_s() - t0) * 1e3 - term_ms;
  return 0;
}

// `part` indices (holes included) of level `level` in the scratch buffer B
int deep_term_slice(vsrmc_checker* c, const PassDst& B, u64 part, int level, int kind, u64 bag, bool probe_next) {
  vsrmc_deep_terminal* A = c->deep_term;
  if (!part || level <= A->scanned_through) return 0;
  const int idx = level - A->first;
  if (idx < 0 || (size_t)idx >= A->cur.size()) return fail(VSRMC_E_STATE, "deep terminal scan: level " + std::to_string(level) + " is not a level of this descent");
  DeepTermScan& L = A->cur[(size_t)idx];
  L.kind = kind;
  L.slices++;
  L.chunks++;
  const double t0 = now_s();
  int rc = deep_term_launch(c, A, B.words, B.off, B.fp, part, A->d_ctl + idx, A->d_list, L, nullptr);
  if (rc) return rc;
  L.ms += (now_s() - t0) * 1e3;
  if (kind != DEEP_KIND_INSERTED) return 0;
  if (!probe_next) { A->probe_skipped = true; return 0; }          // (a violating inserted level: it is completed, nothing deeper is examined)
  return deep_term_probe(c, B, part, level, bag);
}

// kept entries (3 words each) -> fingerprints ascending with their flags
void deep_term_publish(DeepTermScan& L) {
  const u64 kept = L.raw.size() / 3;
  const std::vector<u64> order = sorted_order(kept, [&](u64 a, u64 b) { return L.raw[3 * a] < L.raw[3 * b]; });
  L.fps.resize(kept);
  L.flags.resize(kept);
  for (u64 k = 0; k < kept; k++) { L.fps[k] = L.raw[3 * order[k]]; L.flags[k] = (uint8_t)L.raw[3 * order[k] + 2]; }
  std::vector<u64>().swap(L.raw);
}

// the probed level of the descent that is over: the collected terminal copies (fingerprint, key, flags) -> distinct states of that level
int deep_term_resolve_probed(vsrmc_checker* c, int plevel) {
  vsrmc_deep_terminal* A = c->deep_term;
  DeepTermScan& P = A->probed;
  TermCtl h;
  HIPCHK(hipMemcpy(&h, A->d_pctl, sizeof(h), hipMemcpyDeviceToHost));
  P.level = plevel;
  P.kind = DEEP_KIND_PROBED;
  P.n_states = h.scanned;                                          // copies scanned, not states
  const u64 kept = P.raw.size() / 3;
  P.exact = P.n_listed <= kept ? 1 : 0;
  const std::vector<u64> order = sorted_order(kept, [&](u64 a, u64 b) {       // by fingerprint, then key: the first copy of a state carries its smallest key
    if (P.raw[3 * a] != P.raw[3 * b]) return P.raw[3 * a] < P.raw[3 * b];
    return P.raw[3 * a + 1] < P.raw[3 * b + 1];
  });
  std::vector<u64> fps, keys, flags;
  for (u64 k = 0; k < kept; k++)
    if (k == 0 || P.raw[3 * order[k]] != P.raw[3 * order[k - 1]]) { fps.push_back(P.raw[3 * order[k]]); keys.push_back(P.raw[3 * order[k] + 1]); flags.push_back(P.raw[3 * order[k] + 2]); }
  std::vector<u64>().swap(P.raw);
  std::vector<uint8_t> seen8(fps.size(), 0);
  // (copies collected while the inserted level was incomplete: the ones that are by now states of a level below the probed one are dropped)
  int rc = vsrmc_checker_seen_batch(c, fps.data(), (u64)fps.size(), plevel, seen8.data());
  if (rc) return rc;
  for (size_t g = 0; g < fps.size(); g++) {
    if (seen8[g]) continue;
    P.fps.push_back(fps[g]);
    P.keys.push_back(keys[g]);
    P.flags.push_back((uint8_t)flags[g]);
    P.n_terminal++;
    P.min_fp = std::min<u64>(P.min_fp, fps[g]);
    if (flags[g] & 2) { P.n_unsettled++; P.min_fp_unsettled = std::min<u64>(P.min_fp_unsettled, fps[g]); }
  }
  if (P.exact) P.n_listed = (u64)P.fps.size();                     // (an overflowed list: the copies offered, an upper bound of the states; the counts are lower bounds)
  return 0;
}

int deep_term_end(vsrmc_checker* c, int rc_in) {
  vsrmc_deep_terminal* A = c->deep_term;
  if (rc_in) { A->cur.clear(); return rc_in; }                    // (the checker has failed: nothing of this descent is reported)
  const size_t n = A->cur.size();
  if (!n) return 0;
  std::vector<TermCtl> t(n);
  HIPCHK(hipMemcpy(t.data(), A->d_ctl, sizeof(TermCtl) * n, hipMemcpyDeviceToHost));
  int deepest = A->scanned_through, inserted = -1;
  for (size_t i = 0; i < n; i++) {
    DeepTermScan& L = A->cur[i];
    if (!L.slices) continue;
    deepest = std::max(deepest, L.level);
    if (L.kind == DEEP_KIND_INSERTED) inserted = L.level;
    L.n_states = t[i].scanned;
    L.n_terminal = t[i].terminal;
    L.n_unsettled = t[i].unsettled;
    L.min_fp = t[i].min_fp;
    L.min_fp_unsettled = t[i].min_fp_unsettled;
    if (L.n_listed != L.n_terminal) return fail(VSRMC_E_HIP, "deep terminal scan: level " + std::to_string(L.level) + " has " + std::to_string(L.n_terminal) + " terminal states, " +
                                                                 std::to_string(L.n_listed) + " were offered to the list");
    const int di = L.level - c->level - 1;                         // the level's size is known exactly: a scan that saw another number of states is a bug
    // (the inserted level's size: deep_pass files it before this hook runs)
    if (di >= 0 && (size_t)di < c->deep_lv.size() && L.n_states != c->deep_lv[(size_t)di].n_new)
      return fail(VSRMC_E_HIP, "deep terminal scan: level " + std::to_string(L.level) + " has " + std::to_string(c->deep_lv[(size_t)di].n_new) + " states, the scan saw " +
                                   std::to_string(L.n_states));
    deep_term_publish(L);
    A->results[std::make_pair(L.level, 0)] = std::move(L);
  }
  A->cur.clear();
  A->scanned_through = deepest;
  if (inserted >= 0 && !A->probe_skipped && A->probed.slices) {
    int rc = deep_term_resolve_probed(c, inserted + 1);
    if (rc) return rc;
    A->results[std::make_pair(inserted + 1, 1)] = std::move(A->probed);
  }
  A->probed = DeepTermScan();
  return 0;
}

const DeepTermScan* deep_term_find(vsrmc_checker* c, int level, int probed) {
  if (!c->deep_term) { (void)fail(VSRMC_E_STATE, "no terminal attachment (vsrmc_checker_deep_terminal_attach)"); return nullptr; }
  const auto it = c->deep_term->results.find(std::make_pair(level, probed ? 1 : 0));
  if (it == c->deep_term->results.end()) {
    (void)fail(VSRMC_E_ARG, "deep terminal scan: level " + std::to_string(level) + " has not been examined" + (probed ? " as a probed level" : ""));
    return nullptr;
  }
  return &it->second;
}

}  // namespace

extern "C" {

int32_t vsrmc_checker_deep_terminal_attach(vsrmc_checker* c) {
  if (!c) return fail(VSRMC_E_ARG, "NULL argument");
  if (deep_constrain_on(c)) return fail(VSRMC_E_STATE, "deep terminal scan: the constraint is applied beyond the record buffers (vsrmc_checker_constrain_deep): the probed level's successors are judged on arrival, which the terminal attachment does not know about");
  if (c->constraint) return fail(VSRMC_E_STATE, "deep terminal scan: a constraint is attached (vsrmc_checker_constrain_attach): the levels beyond the record buffers are not constrained");
  if (action_deep_on(c)) return fail(VSRMC_E_STATE, "deep terminal scan: the action constraint is applied beyond the record buffers (vsrmc_checker_action_constrain_deep): the attached scans read transitions the gate does not take");
  if (c->action_constraint) return fail(VSRMC_E_STATE, "deep terminal scan: an action constraint is attached (vsrmc_checker_action_constrain_attach): the levels beyond the record buffers are not constrained");
  if (c->opt.world > 1) return fail(VSRMC_E_STATE, "deep terminal scan: sharded checkers are not scanned (their terminal states stay counted: vsrmc_level_info.deadlocks)");
  if (c->opt.exact_ties) return fail(VSRMC_E_STATE, "deep terminal scan: levels beyond the record buffers need a single-pass checker");
  if (c->deep_term) return 0;                                      // a second attachment is a no-op
  HIPCHK(hipSetDevice(c->opt.device));
  const Model& M = c->model.M;
  vsrmc_deep_terminal* A = new vsrmc_deep_terminal();
  A->scanned_through = c->level;                                   // the stored levels are vsrmc_checker_terminal_scan's
  A->list_cap = (u64)1 << 20;
  A->inst_cap = STEP_LIST_CAP;
  const u64 rec_max = (u64)M.fixed + (u64)M.max_bag;
  A->child_words = std::max<u64>((u64)1 << 26, 64 * rec_max);     // 512 MB of child records per chunk
  // TEST KNOBS (documented in include/vsrmc.h): a smaller list and child buffer, so that a test reaches the overflow and the several-chunk paths
  if (const char* e = std::getenv("VSRMC_TERMINAL_LIST_CAP")) A->list_cap = std::min<u64>(A->list_cap, std::max<u64>(1, std::strtoull(e, nullptr, 10)));
  if (const char* e = std::getenv("VSRMC_DEEP_CHILD_WORDS")) A->child_words = std::min<u64>(A->child_words, std::max<u64>(64 * rec_max, std::strtoull(e, nullptr, 10)));
  A->child_idx = A->child_words / (u64)std::max(1, M.fixed) + 64;  // (a child has at least `fixed` words)
  DevMem& mem = A->mem;
  (void)mem.alloc(&A->d_ctl, sizeof(TermCtl) * DEEP_MAX_LEVELS);
  (void)mem.alloc(&A->d_pctl, sizeof(TermCtl));
  (void)mem.alloc(&A->d_cctl, sizeof(ProbeChildCtl));
  (void)mem.alloc(&A->d_sctl, sizeof(StepCtl));
  (void)mem.alloc(&A->d_list, A->list_cap * 24);
  (void)mem.alloc(&A->d_plist, A->list_cap * 24);
  (void)mem.alloc(&A->d_inst, A->inst_cap * 8);
  (void)mem.alloc(&A->d_child, A->child_words * 8);
  (void)mem.alloc(&A->d_refs, A->child_idx * 8);
  (void)mem.alloc(&A->d_fps, A->child_idx * 8);
  (void)mem.alloc(&A->d_keys, A->child_idx * 8);
  if (mem.err != hipSuccess) {
    (void)hipGetLastError();
    delete A;
    return fail(VSRMC_E_HIP, "deep terminal scan: hipMalloc of the attachment's buffers failed");
  }
  c->deep_term = A;
  return 0;
}

int32_t vsrmc_checker_deep_terminal_levels(vsrmc_checker* c, int32_t* levels, int32_t* probed, uint64_t cap, uint64_t* n) {
  if (!c || !n) return fail(VSRMC_E_ARG, "NULL argument");
  *n = 0;
  if (!c->deep_term) return fail(VSRMC_E_STATE, "no terminal attachment (vsrmc_checker_deep_terminal_attach)");
  *n = (u64)c->deep_term->results.size();
  if (!levels) return 0;                                           // levels == NULL: only the number is asked for
  if (cap < *n) return fail(VSRMC_E_ARG, "buffer too small");
  u64 i = 0;
  for (const auto& kv : c->deep_term->results) {
    levels[i] = kv.first.first;
    if (probed) probed[i] = kv.first.second;
    i++;
  }
  return 0;
}

int32_t vsrmc_checker_deep_terminal_result(vsrmc_checker* c, int32_t level, int32_t probed, vsrmc_deep_terminal_info* info) {
  if (!c || !info) return fail(VSRMC_E_ARG, "NULL argument");
  const DeepTermScan* L = deep_term_find(c, level, probed);
  if (!L) return c->deep_term ? VSRMC_E_ARG : VSRMC_E_STATE;
  std::memset(info, 0, sizeof(*info));
  info->level = L->level;
  info->kind = L->kind;
  info->exact = L->exact;
  info->slices = L->slices;
  info->chunks = L->chunks;
  info->n_states = L->n_states;
  info->n_terminal = L->n_terminal;
  info->n_unsettled = L->n_unsettled;
  info->min_fp = L->min_fp;
  info->min_fp_unsettled = L->min_fp_unsettled;
  info->n_listed = L->n_listed;
  info->bytes_written = L->bytes_written;
  info->ms = L->ms;
  info->children_ms = L->children_ms;
  return 0;
}

int32_t vsrmc_checker_deep_terminal_states(vsrmc_checker* c, int32_t level, int32_t probed, uint64_t* fps, uint8_t* flags, uint64_t cap, uint64_t* n) {
  if (!c || !n) return fail(VSRMC_E_ARG, "NULL argument");
  *n = 0;
  const DeepTermScan* L = deep_term_find(c, level, probed);
  if (!L) return c->deep_term ? VSRMC_E_ARG : VSRMC_E_STATE;
  *n = L->n_listed;
  const u64 kept = L->fps.size();
  if (fps) {
    if (cap < kept) return fail(VSRMC_E_ARG, "buffer too small");
    std::copy(L->fps.begin(), L->fps.end(), fps);
    if (flags) std::copy(L->flags.begin(), L->flags.end(), flags);
  }
  if (L->n_listed > kept || !L->exact)
    return fail(VSRMC_E_REP, "deep terminal states: level " + std::to_string(level) + " has " + std::to_string(L->n_listed) + ", the list holds the " + std::to_string(kept) +
                                 " that arrived first" + (L->exact ? " (counters and minima of the scan are exact)" : " (a probed level: the figures are lower bounds)"));
  return 0;
}

int32_t vsrmc_checker_deep_terminal_witness(vsrmc_checker* c, int32_t level, int32_t probed, int32_t unsettled, uint64_t* words, uint64_t cap_words, uint64_t* off,
                                            int32_t* actions, uint64_t cap_states, uint64_t* n_states) {
  if (!c || !words || !off || !actions || !n_states) return fail(VSRMC_E_ARG, "NULL argument");
  *n_states = 0;
  const DeepTermScan* L = deep_term_find(c, level, probed);
  if (!L) return c->deep_term ? VSRMC_E_ARG : VSRMC_E_STATE;
  const u64 fp = unsettled ? L->min_fp_unsettled : L->min_fp;
  if (fp == ~(u64)0) return fail(VSRMC_E_ARG, "deep terminal witness: level " + std::to_string(level) + " has no " + (unsettled ? "unsettled " : "") + "terminal state");
  if (L->kind == DEEP_KIND_PROBED) {                               // the parent is named by the 45 bits the smallest key among the state's copies keeps of it
    const auto it = std::lower_bound(L->fps.begin(), L->fps.end(), fp);
    if (it == L->fps.end() || *it != fp) return fail(VSRMC_E_STATE, "deep terminal witness: the list of the probed level does not hold the state");
    return trace_by_parent_key(c, fp, L->keys[(size_t)(it - L->fps.begin())], level, words, cap_words, off, actions, cap_states, n_states);
  }
  return vsrmc_checker_trace_fp(c, level, fp, words, cap_words, off, actions, cap_states, n_states);
}

}  // extern "C"
