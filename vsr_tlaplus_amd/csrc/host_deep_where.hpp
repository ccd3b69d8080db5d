// host_deep_where.hpp — a user's predicates on the levels beyond the record buffers: the attachment of a state and / or a step program to a
// checker, the three hooks a descent of the deep search calls (vsr_deep.hpp: deep_where_begin / _slice / _end; _slice is a consumer of step_slices,
// host_step_slices.hpp), the per-level results and the witnesses (included by vsrmc.hip after host_step.hpp: one translation unit, the sections share its
// anonymous-namespace helpers).
//
// Every state of a seen-set-only level passes through a scratch buffer once per descent, as (words, off, fp, index range, holes included): the shape k_where
// and k_step_list / k_step_apply take.  A level K beyond the base is scanned in the FIRST descent after the attachment that regenerates or inserts it
// (scanned_through: the deepest level done), slice by slice; the figures of the slices of a level accumulate in one control block per level on the device,
// reset once per level (the list cursors n_list / n_hits are per launch).  The successors of the inserted level's sub-slices — the probed level, which has
// no records — go through k_probe_where (vsr_deep_where.hpp) from the instance list k_step_list wrote for k_step_apply.
// Buffers are allocated once per attachment; the programs are uploaded once.
#pragma once
#include <map>

enum { DEEP_KIND_REGEN = 0, DEEP_KIND_INSERTED = 1, DEEP_KIND_PROBED = 2, DEEP_MAX_LEVELS = 512 };

struct DeepLevelScan {
  int level = 0, kind = DEEP_KIND_REGEN;
  int exact = 1;
  u64 slices = 0;                      // scratch slices of the level that were scanned
  double where_ms = 0, step_ms = 0;    // host time around the launches of the state / the step program (their synchronisation included)
  WhereCtl w;                          // state program: the level's control block as the device left it (probed: filled by the host's resolution)
  u64 n_states = 0;
  u64 where_total = 0;                 // states with any bit set: the true number; the list holds the first where_cap that arrived
  std::vector<u64> where_raw;          // while the descent runs: 3 words per kept entry (fingerprint, index | key, bits)
  std::vector<u64> where_fps, where_keys;
  std::vector<uint8_t> where_bits;
  StepCtl s;                           // step program
  u64 step_scanned = 0, step_total = 0, step_launches = 0;
  std::vector<u64> step_raw;           // 4 words per kept hit pair
  std::vector<u64> step_fps;
  std::vector<uint32_t> step_ords;
  std::vector<uint8_t> step_bits;
  DeepLevelScan() { std::memset(&w, 0, sizeof(w)); std::memset(&s, 0, sizeof(s)); }
};

struct vsrmc_deep_attach {
  vsrmc_where state, step;             // copies: the caller may destroy its programs
  bool has_state = false, has_step = false;
  int scanned_through = 0;             // every level <= this one is either stored or has been scanned
  u64 where_cap = 0, hit_cap = 0, list_cap = 0;
  DevMem mem;                          // the device buffers below: allocated once per attachment, freed with it
  u32 *d_prog_state = nullptr, *d_prog_step = nullptr;
  WhereCtl* d_wctl = nullptr;          // DEEP_MAX_LEVELS blocks: block i = level first + i of the descent in flight
  StepCtl* d_sctl = nullptr;
  ProbeWhereCtl* d_pctl = nullptr;
  u64 *d_wlist = nullptr, *d_hits = nullptr, *d_list = nullptr, *d_plist = nullptr;
  // the descent in flight
  int first = 0;
  std::vector<DeepLevelScan> cur;
  DeepLevelScan probed;
  bool probe_skipped = false;
  std::map<std::pair<int, int>, DeepLevelScan> results;   // (level, 1 = as the probed level) -> figures
};

namespace {

void deep_attach_free(vsrmc_checker* c) {
  vsrmc_deep_attach* A = c->deep_attach;
  if (!A) return;
  delete A;
  c->deep_attach = nullptr;
}

void deep_attach_restart(vsrmc_checker* c) {
  vsrmc_deep_attach* A = c->deep_attach;
  if (!A) return;
  A->scanned_through = 1;              // (checker_seed: level 1 is the stored level)
  A->cur.clear();
  A->results.clear();
}

// before a descent that regenerates / inserts the levels up to last_level: one control block per level that has not been scanned yet
int deep_where_begin(vsrmc_checker* c, int last_level) {
  vsrmc_deep_attach* A = c->deep_attach;
  A->cur.clear();
  A->probed = DeepLevelScan();
  A->probe_skipped = false;
  A->first = A->scanned_through + 1;
  if (last_level < A->first) return 0;
  const int n = last_level - A->first + 1;
  if (n > DEEP_MAX_LEVELS) return fail(VSRMC_E_REP, "deep predicates: more than 512 levels to scan in one descent");
  A->cur.resize((size_t)n);
  std::vector<WhereCtl> w((size_t)n, fresh_ctl<WhereCtl>());
  std::vector<StepCtl> s((size_t)n, fresh_ctl<StepCtl>());
  for (int i = 0; i < n; i++) A->cur[(size_t)i].level = A->first + i;
  HIPCHK(hipMemcpyAsync(A->d_wctl, w.data(), sizeof(WhereCtl) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(A->d_sctl, s.data(), sizeof(StepCtl) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(A->d_pctl, 0, sizeof(ProbeWhereCtl), c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));                         // (the sources are local vectors)
  return 0;
}

// `part` indices (holes included) of level `level` in the scratch buffer B
int deep_where_slice(vsrmc_checker* c, const PassDst& B, u64 part, int level, int kind, u64 bag, bool probe_next) {
  vsrmc_deep_attach* A = c->deep_attach;
  if (!part || level <= A->scanned_through) return 0;
  const int idx = level - A->first;
  if (idx < 0 || (size_t)idx >= A->cur.size()) return fail(VSRMC_E_STATE, "deep predicates: level " + std::to_string(level) + " is not a level of this descent");
  const Model& M = c->model.M;
  DeepLevelScan& L = A->cur[(size_t)idx];
  L.kind = kind;
  L.slices++;
  if (A->has_state) {
    const double t0 = now_s();
    WhereCtl* ctl = A->d_wctl + idx;
    const u64 room = A->where_cap - L.where_raw.size() / 3;
    HIPCHK(hipMemsetAsync(&ctl->n_list, 0, 8, c->stream));         // the list cursor is this launch's; counters and minima go on from the slices before
    hipLaunchKernelGGL(KERNEL_OF(k_where, M), dim3(scan_grid(part, c->num_cus)), dim3(256), 0, c->stream, M, (const u32*)A->d_prog_state,
                       (int)A->state.prog.names.size(), (const u64*)B.words, (const u64*)B.off, (const u64*)B.fp, part, (uint8_t*)nullptr, ctl, A->d_wlist, room);
    HIPCHK(hipGetLastError());
    u64 n_list = 0;
    HIPCHK(hipMemcpyAsync(&n_list, &ctl->n_list, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    L.where_total += n_list;
    const u64 kept = std::min<u64>(n_list, room);
    if (kept) {
      const size_t at = L.where_raw.size();
      L.where_raw.resize(at + 3 * kept);
      HIPCHK(hipMemcpy(L.where_raw.data() + at, A->d_wlist, kept * 24, hipMemcpyDeviceToHost));
    }
    L.where_ms += (now_s() - t0) * 1e3;
  }
  const bool probe = A->has_state && kind == DEEP_KIND_INSERTED && probe_next;
  if (A->has_state && kind == DEEP_KIND_INSERTED && !probe_next) A->probe_skipped = true;   // (a violating inserted level: nothing deeper is examined)
  if (!A->has_step && !probe) return 0;
  // the transitions out of the slice: sub-slices of parents through step_slices (host_step_slices.hpp) over the attachment's buffers; every list feeds
  // k_step_apply and, for the inserted level, k_probe_where.  Host time, no events; the synchronisations behind k_step_apply and k_probe_where are this
  // consumer's own (the hit cursor is read per launch; the next k_step_list rewrites the instance list).
  const double t1 = now_s();
  double probe_ms = 0;
  StepCtl* sctl = A->d_sctl + idx;
  auto* const apply_kernel = KERNEL_OF(k_step_apply, M);
  auto* const probe_kernel = KERNEL_OF(k_probe_where, M);
  const int bag_bound = bag ? (int)std::min<u64>(bag, (u64)M.max_bag) : M.max_bag;
  SlicePolicy sp(0, part, A->list_cap, step_slice_default(M, bag_bound, A->list_cap));
  const StepListing listing{B.words, B.off, c->stream, c->num_cus, A->d_list, sctl};
  const int rc = step_slices(M, listing, sp, "deep predicates", &L.step_scanned, nullptr, [&](u64, u64, u64 n_inst) -> int {
    const unsigned grid_a = scan_grid(n_inst, c->num_cus);
    if (A->has_step) {
      const u64 room = A->hit_cap - L.step_raw.size() / 4;
      HIPCHK(hipMemsetAsync(&sctl->n_hits, 0, 8, c->stream));
      hipLaunchKernelGGL(apply_kernel, dim3(grid_a), dim3(256), 0, c->stream, M, (const u32*)A->d_prog_step, (int)A->step.prog.names.size(), (const u64*)B.words,
                         (const u64*)B.off, (const u64*)B.fp, (const u64*)A->d_list, n_inst, sctl, A->d_hits, room, (u32*)nullptr);
      HIPCHK(hipGetLastError());
      u64 n_hits = 0;
      HIPCHK(hipMemcpyAsync(&n_hits, &sctl->n_hits, 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      L.step_total += n_hits;
      const u64 kept = std::min<u64>(n_hits, room);
      if (kept) {
        const size_t at = L.step_raw.size();
        L.step_raw.resize(at + 4 * kept);
        HIPCHK(hipMemcpy(L.step_raw.data() + at, A->d_hits, kept * 32, hipMemcpyDeviceToHost));
      }
    }
    if (probe) {                                                   // the probed level: the cursor of its list runs through the whole pass
      const double tp = now_s();
      hipLaunchKernelGGL(probe_kernel, dim3(grid_a), dim3(256), 0, c->stream, M, (const u32*)A->d_prog_state, (const u64*)B.words, (const u64*)B.off,
                         (const u64*)A->d_list, n_inst, (const Slot*)c->table, c->tmask, level + 1, A->d_pctl, A->d_plist, A->where_cap);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(c->stream));                     // (the next k_step_list rewrites the instance list)
      A->probed.slices++;
      A->probed.where_ms += (now_s() - tp) * 1e3;                  // (k_probe_where's time is the probed level's, not the inserted level's step time)
      probe_ms += (now_s() - tp) * 1e3;
    }
    return 0;
  });
  L.step_launches += sp.listings;
  if (rc) return rc;
  L.step_ms += (now_s() - t1) * 1e3 - probe_ms;                    // k_step_list (also when it only feeds the probe) and k_step_apply
  return 0;
}

// the probed level of the descent that is over: the collected (fingerprint, key, bits) copies -> distinct states of that level
int deep_where_resolve_probed(vsrmc_checker* c, int plevel) {
  vsrmc_deep_attach* A = c->deep_attach;
  DeepLevelScan& P = A->probed;
  ProbeWhereCtl h;
  HIPCHK(hipMemcpy(&h, A->d_pctl, sizeof(h), hipMemcpyDeviceToHost));
  if (h.n_internal) return fail(VSRMC_E_HIP, "k_probe_where: " + std::to_string(h.n_internal) + " listed instances are not enabled (guard_slot_pre and gen disagree)");
  P.level = plevel;
  P.kind = DEEP_KIND_PROBED;
  P.n_states = h.n_fresh;
  P.exact = h.n_list <= A->where_cap ? 1 : 0;
  P.w = fresh_ctl<WhereCtl>();
  P.w.scanned = h.n_fresh;
  const u64 kept = std::min<u64>(h.n_list, A->where_cap);
  std::vector<u64> raw(kept * 3);
  if (kept) HIPCHK(hipMemcpy(raw.data(), A->d_plist, kept * 24, hipMemcpyDeviceToHost));
  const std::vector<u64> order = sorted_order(kept, [&](u64 a, u64 b) {       // by fingerprint, then key: the first copy of a state carries its smallest key
    if (raw[3 * a] != raw[3 * b]) return raw[3 * a] < raw[3 * b];
    if (raw[3 * a + 1] != raw[3 * b + 1]) return raw[3 * a + 1] < raw[3 * b + 1];
    return raw[3 * a + 2] < raw[3 * b + 2];
  });
  std::vector<u64> fps, keys, bits;
  for (u64 k = 0; k < kept; k++)
    if (k == 0 || raw[3 * order[k]] != raw[3 * order[k - 1]]) { fps.push_back(raw[3 * order[k]]); keys.push_back(raw[3 * order[k] + 1]); bits.push_back(raw[3 * order[k] + 2]); }
  std::vector<uint8_t> seen8(fps.size(), 0);
  // (copies collected while the inserted level was incomplete: the ones that are by now states of a level below the probed one are dropped)
  int rc = vsrmc_checker_seen_batch(c, fps.data(), (u64)fps.size(), plevel, seen8.data());
  if (rc) return rc;
  for (size_t g = 0; g < fps.size(); g++) {
    if (seen8[g]) continue;
    P.where_fps.push_back(fps[g]);
    P.where_keys.push_back(keys[g]);
    P.where_bits.push_back((uint8_t)bits[g]);
    for (int k = 0; k < WHERE_MAX_EXPORTS; k++)
      if ((bits[g] >> k) & 1) { P.w.count[k]++; P.w.min_fp[k] = std::min<u64>(P.w.min_fp[k], fps[g]); }
  }
  P.where_total = P.exact ? (u64)P.where_fps.size() : h.n_list;    // (an overflowed list: the copies offered, an upper bound of the states; the counts are lower bounds)
  return 0;
}

int deep_where_end(vsrmc_checker* c, int rc_in) {
  vsrmc_deep_attach* A = c->deep_attach;
  if (rc_in) { A->cur.clear(); return rc_in; }                    // (the checker has failed: nothing of this descent is reported)
  const size_t n = A->cur.size();
  if (!n) return 0;
  std::vector<WhereCtl> w(n);
  std::vector<StepCtl> s(n);
  HIPCHK(hipMemcpy(w.data(), A->d_wctl, sizeof(WhereCtl) * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(s.data(), A->d_sctl, sizeof(StepCtl) * n, hipMemcpyDeviceToHost));
  bool any = false;
  int deepest = A->scanned_through;
  for (size_t i = 0; i < n; i++) any = any || A->cur[i].slices != 0;
  if (any)
    for (auto& kv : A->results) {                                  // hit lists are kept for the levels the last descent scanned
      DeepLevelScan& o = kv.second;
      std::vector<u64>().swap(o.where_fps); std::vector<u64>().swap(o.where_keys); std::vector<uint8_t>().swap(o.where_bits);
      std::vector<u64>().swap(o.step_fps); std::vector<uint32_t>().swap(o.step_ords); std::vector<uint8_t>().swap(o.step_bits);
    }
  int inserted = -1;
  for (size_t i = 0; i < n; i++) {
    DeepLevelScan& L = A->cur[i];
    if (!L.slices) continue;
    deepest = std::max(deepest, L.level);
    if (L.kind == DEEP_KIND_INSERTED) inserted = L.level;
    L.w = w[i];
    L.s = s[i];
    L.s.scanned = L.step_scanned;
    L.n_states = A->has_state ? L.w.scanned : L.step_scanned;
    if (L.s.n_internal) return fail(VSRMC_E_HIP, "k_step_apply: " + std::to_string(L.s.n_internal) + " listed instances are not enabled (guard_slot_pre and gen disagree)");
    const int di = L.level - c->level - 1;                         // the level's size is known exactly: a scan that saw another number of states is a bug
    if (L.kind == DEEP_KIND_REGEN && di >= 0 && (size_t)di < c->deep_lv.size() && L.n_states != c->deep_lv[(size_t)di].n_new)
      return fail(VSRMC_E_HIP, "deep predicates: level " + std::to_string(L.level) + " has " + std::to_string(c->deep_lv[(size_t)di].n_new) + " states, the scan saw " +
                                   std::to_string(L.n_states));
    const u64 kept = L.where_raw.size() / 3;
    const std::vector<u64> order = sorted_order(kept, [&](u64 a, u64 b) { return L.where_raw[3 * a] < L.where_raw[3 * b]; });
    L.where_fps.resize(kept);
    L.where_bits.resize(kept);
    for (u64 k = 0; k < kept; k++) { L.where_fps[k] = L.where_raw[3 * order[k]]; L.where_bits[k] = (uint8_t)L.where_raw[3 * order[k] + 2]; }
    std::vector<u64>().swap(L.where_raw);
    const u64 hk = L.step_raw.size() / 4;
    const std::vector<u64> horder = sorted_order(hk, [&](u64 a, u64 b) {
      if (L.step_raw[4 * a] != L.step_raw[4 * b]) return L.step_raw[4 * a] < L.step_raw[4 * b];
      return L.step_raw[4 * a + 2] < L.step_raw[4 * b + 2];
    });
    L.step_fps.resize(hk);
    L.step_ords.resize(hk);
    L.step_bits.resize(hk);
    for (u64 k = 0; k < hk; k++) { L.step_fps[k] = L.step_raw[4 * horder[k]]; L.step_ords[k] = (uint32_t)L.step_raw[4 * horder[k] + 2]; L.step_bits[k] = (uint8_t)L.step_raw[4 * horder[k] + 3]; }
    std::vector<u64>().swap(L.step_raw);
    A->results[std::make_pair(L.level, 0)] = std::move(L);
  }
  A->cur.clear();
  A->scanned_through = deepest;
  if (A->has_state && inserted >= 0 && !A->probe_skipped && A->probed.slices) {
    int rc = deep_where_resolve_probed(c, inserted + 1);
    if (rc) return rc;
    A->results[std::make_pair(inserted + 1, 1)] = std::move(A->probed);
  }
  A->probed = DeepLevelScan();
  return 0;
}

const DeepLevelScan* deep_find(vsrmc_checker* c, int level, int probed) {
  if (!c->deep_attach) { (void)fail(VSRMC_E_STATE, "no predicates are attached (vsrmc_checker_deep_attach)"); return nullptr; }
  const auto it = c->deep_attach->results.find(std::make_pair(level, probed ? 1 : 0));
  if (it == c->deep_attach->results.end()) {
    (void)fail(VSRMC_E_ARG, "deep predicates: level " + std::to_string(level) + " has not been examined" + (probed ? " as a probed level" : ""));
    return nullptr;
  }
  return &it->second;
}

}  // namespace

extern "C" {

int32_t vsrmc_checker_deep_attach(vsrmc_checker* c, const vsrmc_where* state_prog, const vsrmc_where* step_prog) {
  if (!c) return fail(VSRMC_E_ARG, "NULL argument");
  if (!state_prog && !step_prog) {                                 // both NULL: detach
    if (c->deep_attach) { HIPCHK(hipSetDevice(c->opt.device)); deep_attach_free(c); }
    return 0;
  }
  if (deep_constrain_on(c)) return fail(VSRMC_E_STATE, "deep predicates: the constraint is applied beyond the record buffers (vsrmc_checker_constrain_deep): the probed level's successors are judged on arrival, which the attached scans do not know about");
  if (c->constraint) return fail(VSRMC_E_STATE, "deep predicates: a constraint is attached (vsrmc_checker_constrain_attach): the levels beyond the record buffers are not constrained");
  if (action_deep_on(c)) return fail(VSRMC_E_STATE, "deep predicates: the action constraint is applied beyond the record buffers (vsrmc_checker_action_constrain_deep): the attached scans read transitions the gate does not take");
  if (c->action_constraint) return fail(VSRMC_E_STATE, "deep predicates: an action constraint is attached (vsrmc_checker_action_constrain_attach): the levels beyond the record buffers are not constrained");
  if (state_prog && state_prog->prog.step) return fail(VSRMC_E_ARG, "deep predicates: a step program in the state position");
  if (step_prog && !step_prog->prog.step) return fail(VSRMC_E_ARG, "deep predicates: a state program in the step position");
  if ((state_prog && !where_fits(state_prog, c->model.M, c->model.symmetry)) || (step_prog && !where_fits(step_prog, c->model.M, c->model.symmetry)))
    return fail(VSRMC_E_ARG, "deep predicates: compiled for another model");
  if (c->opt.world > 1) return fail(VSRMC_E_STATE, "deep predicates: sharded checkers are not scanned");
  if (c->opt.exact_ties) return fail(VSRMC_E_STATE, "deep predicates: levels beyond the record buffers need a single-pass checker");
  HIPCHK(hipSetDevice(c->opt.device));
  deep_attach_free(c);
  vsrmc_deep_attach* A = new vsrmc_deep_attach();
  c->deep_attach = A;
  if (state_prog) { A->state = *state_prog; A->has_state = true; }
  if (step_prog) { A->step = *step_prog; A->has_step = true; }
  A->scanned_through = c->level;                                   // the stored levels are vsrmc_checker_where_scan's / _step_scan's
  A->where_cap = (u64)1 << 20;
  A->hit_cap = STEP_HIT_CAP;
  A->list_cap = STEP_LIST_CAP;
  // TEST KNOBS (documented in include/vsrmc.h): smaller lists, so that a test can reach the overflow paths on a small space
  if (const char* e = std::getenv("VSRMC_WHERE_LIST_CAP")) A->where_cap = std::min<u64>(A->where_cap, std::max<u64>(1, std::strtoull(e, nullptr, 10)));
  if (const char* e = std::getenv("VSRMC_STEP_LIST_CAP")) A->hit_cap = std::min<u64>(A->hit_cap, std::max<u64>(1, std::strtoull(e, nullptr, 10)));
  // ... and a smaller INSTANCE list (at least 64 entries: one record's instances must fit), so that a sub-slice overflows it and is run again in halves
  if (const char* e = std::getenv("VSRMC_DEEP_INSTANCE_CAP")) A->list_cap = std::min<u64>(A->list_cap, std::max<u64>(64, std::strtoull(e, nullptr, 10)));
  DevMem& mem = A->mem;
  (void)mem.alloc(&A->d_wctl, sizeof(WhereCtl) * DEEP_MAX_LEVELS);
  (void)mem.alloc(&A->d_sctl, sizeof(StepCtl) * DEEP_MAX_LEVELS);
  (void)mem.alloc(&A->d_pctl, sizeof(ProbeWhereCtl));
  (void)mem.alloc(&A->d_list, A->list_cap * 8);
  if (A->has_state) {
    (void)mem.alloc(&A->d_wlist, A->where_cap * 24);
    (void)mem.alloc(&A->d_plist, A->where_cap * 24);
    (void)mem.upload(&A->d_prog_state, A->state.prog.ops.data(), A->state.prog.ops.size(), WHERE_MAX_OPS);
  }
  if (A->has_step) {
    (void)mem.alloc(&A->d_hits, A->hit_cap * 32);
    (void)mem.upload(&A->d_prog_step, A->step.prog.ops.data(), A->step.prog.ops.size(), WHERE_MAX_OPS);
  }
  const bool ok = mem.err == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    deep_attach_free(c);
    return fail(VSRMC_E_HIP, "deep predicates: hipMalloc of the attachment's buffers failed");
  }
  return 0;
}

int32_t vsrmc_checker_deep_levels(vsrmc_checker* c, int32_t* levels, int32_t* probed, uint64_t cap, uint64_t* n) {
  if (!c || !n) return fail(VSRMC_E_ARG, "NULL argument");
  *n = 0;
  if (!c->deep_attach) return fail(VSRMC_E_STATE, "no predicates are attached (vsrmc_checker_deep_attach)");
  *n = (u64)c->deep_attach->results.size();
  if (!levels) return 0;                                           // levels == NULL: only the number is asked for
  if (cap < *n) return fail(VSRMC_E_ARG, "buffer too small");
  u64 i = 0;
  for (const auto& kv : c->deep_attach->results) {
    levels[i] = kv.first.first;
    if (probed) probed[i] = kv.first.second;
    i++;
  }
  return 0;
}

int32_t vsrmc_checker_deep_result(vsrmc_checker* c, int32_t level, int32_t probed, vsrmc_deep_info* info, vsrmc_where_info* w, vsrmc_step_info* s) {
  if (!c || !info) return fail(VSRMC_E_ARG, "NULL argument");
  const DeepLevelScan* L = deep_find(c, level, probed);
  if (!L) return c->deep_attach ? VSRMC_E_ARG : VSRMC_E_STATE;
  const vsrmc_deep_attach* A = c->deep_attach;
  std::memset(info, 0, sizeof(*info));
  info->level = L->level;
  info->kind = L->kind;
  info->exact = L->exact;
  info->has_state = A->has_state ? 1 : 0;
  info->has_step = (A->has_step && L->kind != DEEP_KIND_PROBED) ? 1 : 0;
  info->slices = L->slices;
  info->n_hit_states = L->where_total;
  info->n_hit_pairs = L->step_total;
  info->where_ms = L->where_ms;
  info->step_ms = L->step_ms;
  if (w) {
    std::memset(w, 0, sizeof(*w));
    w->level = L->level;
    w->n_states = L->n_states;
    w->kernel_ms = L->where_ms;
    for (int k = 0; k < WHERE_MAX_EXPORTS; k++) {
      w->count[k] = A->has_state ? L->w.count[k] : 0;
      w->min_fp[k] = A->has_state ? L->w.min_fp[k] : ~(u64)0;
      w->min_index[k] = ~(u64)0;                                   // a transient level has no index range
    }
  }
  if (s) {
    std::memset(s, 0, sizeof(*s));
    s->level = L->level;
    const bool has = info->has_step != 0;
    s->n_states = has ? L->step_scanned : 0;
    s->n_pairs = has ? L->s.n_pairs : 0;
    s->n_err = has ? L->s.n_err : 0;
    s->kernel_ms = L->step_ms;
    s->slices = L->step_launches;
    for (int k = 0; k < WHERE_MAX_EXPORTS; k++) {
      s->count[k] = has ? L->s.count[k] : 0;
      s->min_fp[k] = has ? L->s.min_fp[k] : ~(u64)0;
      s->min_index[k] = ~(u64)0;
      s->min_ordinal[k] = ~(uint32_t)0;                            // (the ordinals of a scratch slice are gone: vsrmc_checker_deep_witness finds the instance again)
      s->min_action[k] = -1;
    }
  }
  return 0;
}

int32_t vsrmc_checker_deep_where_states(vsrmc_checker* c, int32_t level, int32_t probed, uint64_t* fps, uint8_t* bits, uint64_t cap, uint64_t* n) {
  if (!c || !n) return fail(VSRMC_E_ARG, "NULL argument");
  *n = 0;
  const DeepLevelScan* L = deep_find(c, level, probed);
  if (!L) return c->deep_attach ? VSRMC_E_ARG : VSRMC_E_STATE;
  *n = L->where_total;
  const u64 kept = L->where_fps.size();
  if (L->where_total && !kept) return fail(VSRMC_E_STATE, "deep predicates: the list of level " + std::to_string(level) + " was dropped when a later descent scanned new levels");
  if (fps) {
    if (cap < kept) return fail(VSRMC_E_ARG, "buffer too small");
    std::copy(L->where_fps.begin(), L->where_fps.end(), fps);
    if (bits) std::copy(L->where_bits.begin(), L->where_bits.end(), bits);
  }
  if (L->where_total > kept || !L->exact)
    return fail(VSRMC_E_REP, "deep where states: level " + std::to_string(level) + " has " + std::to_string(L->where_total) + ", the list holds the " + std::to_string(kept) +
                                 " that arrived first");
  return 0;
}

int32_t vsrmc_checker_deep_step_pairs(vsrmc_checker* c, int32_t level, uint64_t* fps, uint32_t* ordinals, uint8_t* bits, uint64_t cap, uint64_t* n) {
  if (!c || !n) return fail(VSRMC_E_ARG, "NULL argument");
  *n = 0;
  const DeepLevelScan* L = deep_find(c, level, 0);
  if (!L) return c->deep_attach ? VSRMC_E_ARG : VSRMC_E_STATE;
  *n = L->step_total;
  const u64 kept = L->step_fps.size();
  if (L->step_total && !kept) return fail(VSRMC_E_STATE, "deep predicates: the list of level " + std::to_string(level) + " was dropped when a later descent scanned new levels");
  if (fps) {
    if (cap < kept) return fail(VSRMC_E_ARG, "buffer too small");
    std::copy(L->step_fps.begin(), L->step_fps.end(), fps);
    if (ordinals) std::copy(L->step_ords.begin(), L->step_ords.end(), ordinals);
    if (bits) std::copy(L->step_bits.begin(), L->step_bits.end(), bits);
  }
  if (L->step_total > kept)
    return fail(VSRMC_E_REP, "deep step pairs: level " + std::to_string(level) + " has " + std::to_string(L->step_total) + ", the list holds the " + std::to_string(kept) +
                                 " that arrived first (counters and minima of the scan are exact)");
  return 0;
}

int32_t vsrmc_checker_deep_witness(vsrmc_checker* c, int32_t level, int32_t which_program, int32_t k, uint64_t* words, uint64_t cap_words, uint64_t* off, int32_t* actions,
                                   uint64_t cap_states, uint64_t* n_states) {
  if (!c || !words || !off || !actions || !n_states) return fail(VSRMC_E_ARG, "NULL argument");
  *n_states = 0;
  if (which_program < 0 || which_program > 2 || k < 0 || k >= WHERE_MAX_EXPORTS) return fail(VSRMC_E_ARG, "deep witness: which_program is 0 (state), 1 (step) or 2 (state, probed level); k < 8");
  const DeepLevelScan* L = deep_find(c, level, which_program == 2);
  if (!L) return c->deep_attach ? VSRMC_E_ARG : VSRMC_E_STATE;
  const vsrmc_deep_attach* A = c->deep_attach;
  if (which_program == 1 ? !A->has_step : !A->has_state) return fail(VSRMC_E_ARG, "deep witness: no such program is attached");
  const u64 fp = which_program == 1 ? L->s.min_fp[k] : L->w.min_fp[k];
  if (fp == ~(u64)0) return fail(VSRMC_E_ARG, "deep witness: nothing in level " + std::to_string(level) + " satisfies predicate " + std::to_string(k));
  if (which_program == 2) {                                        // the parent is named by the 45 bits the smallest key among the state's copies keeps of it
    const auto it = std::lower_bound(L->where_fps.begin(), L->where_fps.end(), fp);
    if (it == L->where_fps.end() || *it != fp) return fail(VSRMC_E_STATE, "deep witness: the list of the probed level no longer holds the state");
    return trace_by_parent_key(c, fp, L->where_keys[(size_t)(it - L->where_fps.begin())], level, words, cap_words, off, actions, cap_states, n_states);
  }
  int rc = vsrmc_checker_trace_fp(c, level, fp, words, cap_words, off, actions, cap_states, n_states);
  if (rc || which_program == 0) return rc;
  // a step hit: the lowest-ordinal instance of the REPLAYED parent record whose pair has bit k (the ordinals of the scratch slice are gone, and under
  // SYMMETRY the replayed record may be another member of the state's orbit), through the batch entry points on that one record
  const u64 ns = *n_states;
  if (ns + 1 > cap_states) return fail(VSRMC_E_ARG, "buffer too small");
  const u64* parent = words + off[ns - 1];
  const u64 plen = off[ns] - off[ns - 1];
  const u64 poff[2] = {0, plen};
  u64 n_rows = 0;
  rc = vsrmc_step_batch(&c->model, c->opt.device, &A->step, parent, poff, 1, nullptr, 0, &n_rows);
  if (rc) return rc;
  std::vector<u64> rows(5 * std::max<u64>(1, n_rows));
  rc = vsrmc_step_batch(&c->model, c->opt.device, &A->step, parent, poff, 1, rows.data(), n_rows, &n_rows);
  if (rc) return rc;
  u64 ord = ~(u64)0;
  for (u64 r = 0; r < n_rows && ord == ~(u64)0; r++)               // (rows come in ordinal order)
    if (!rows[5 * r + 4] && ((rows[5 * r + 3] >> k) & 1)) ord = rows[5 * r + 1];
  if (ord == ~(u64)0) return fail(VSRMC_E_HIP, "deep witness: the witness pair was not found again");
  const u64 cap = n_rows + 1, capw = cap * 256;
  std::vector<u64> ow(capw), om(cap * 8);
  u64 n_out = 0, w_out = 0;
  rc = vsrmc_expand_batch(&c->model, c->opt.device, parent, poff, 1, ow.data(), capw, om.data(), cap, &n_out, &w_out);
  if (rc) return rc;
  for (u64 i = 0; i < n_out; i++) {
    if (om[8 * i + 1] != ord) continue;
    const u64 wo = om[8 * i + 7], len = (u64)c->model.M.h0 + (u64)hdr_nmsg(ow[wo]);
    if (off[ns] + len > cap_words) return fail(VSRMC_E_ARG, "word buffer too small");
    std::copy(&ow[wo], &ow[wo] + len, words + off[ns]);
    off[ns + 1] = off[ns] + len;
    actions[ns] = (int32_t)om[8 * i + 2];
    *n_states = ns + 1;
    return 0;
  }
  return fail(VSRMC_E_HIP, "deep witness: the successor of the witness pair was not generated again");
}

}  // extern "C"
