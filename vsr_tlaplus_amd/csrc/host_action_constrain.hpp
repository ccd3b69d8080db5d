// host_action_constrain.hpp — action constraints: the host side of k_step_expand (vsr_action_constrain.hpp) — attaching one exported
// predicate of a compiled step program to a checker, the level step that takes only the permitted transitions (phase_expand_gated, in the place of
// phase_expand: a consumer of step_slices, host_step_slices.hpp), the per-level figures, and the trace that takes only permitted steps (included by vsrmc.hip: one translation unit, the sections share
// its anonymous-namespace helpers).
#pragma once

struct vsrmc_action_constraint {
  vsrmc_where prog;                    // a copy: the caller may destroy its own
  int k = 0;                           // the exported predicate that is the constraint
  DevMem mem;                          // device buffers, allocated once per attachment, freed with it
  u32* d_prog = nullptr;               // the program (uploaded once)
  u64* d_list = nullptr;               // the instance list of one slice (list_cap entries) ..
  u32* d_rows = nullptr;               // .. the verdict beside every entry ..
  u32* d_live = nullptr;               // .. and one word per parent of the slice (live_cap of them): has it an instance?
  StepCtl* d_sctl = nullptr;
  ActionCtl* d_actl = nullptr;
  u64 list_cap = 0, live_cap = 0;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<vsrmc_action_constraint_info> levels;   // [level]: the figures of the step INTO that level (levels 0 and 1 unused)
  int newest = 0;                      // the level the last step led into
  // beyond the record buffers (vsrmc_checker_action_constrain_deep)
  bool deep_on = false;
  std::vector<vsrmc_action_constraint_deep_info> deep_levels;   // [level]: the gated passes INTO that level, kind 0 = none
  std::vector<u64> deep_epochs;        // [level]: the unit of progress (action_deep_epoch) that filed it
  u64 deep_epoch = 0;
  vsrmc_action_constraint_deep_info pass;   // what the last expand_pass_gated (or an overflowed phase_expand_gated) left for its caller to file
};

namespace {

enum : u64 { ACTION_LIST_CAP = (u64)1 << 22 };
// k_step_expand in one of its modes beyond the record buffers (KERNEL_OF, host_scan_common.hpp, names the stored mode)
#define GATED_KERNEL_OF(M, G) ((M).model_id == 1 ? k_step_expand<1, G> : (M).model_id == 2 ? k_step_expand<2, G> : k_step_expand<0, G>)

void action_constraint_free(vsrmc_checker* c) {
  vsrmc_action_constraint* a = c->action_constraint;
  if (!a) return;
  for (hipEvent_t e : a->ev)
    if (e) (void)hipEventDestroy(e);
  delete a;
  c->action_constraint = nullptr;
}

// a search that starts over (checker_seed): the attachment stays, its results go.  Init is not subject to an action constraint: no transition leads to it.
void action_constraint_restart(vsrmc_checker* c) {
  if (!c->action_constraint) return;
  c->action_constraint->levels.clear();
  c->action_constraint->newest = 0;
  c->action_constraint->deep_levels.clear();
  c->action_constraint->deep_epochs.clear();
}

bool action_deep_on(const vsrmc_checker* c) { return c->action_constraint && c->action_constraint->deep_on; }
void action_deep_epoch(vsrmc_checker* c) {
  if (c->action_constraint) c->action_constraint->deep_epoch++;
}

// the figures of one gated pass, as the info structs carry them
void action_pass_figures(vsrmc_action_constraint_deep_info* p, const ActionCtl& ah, u64 parents, u64 generated, u64 slices, u64 relisted, u64 launches, double list_ms,
                         double verdict_ms, double expand_ms) {
  std::memset(p, 0, sizeof(*p));
  p->parents = parents;
  p->pairs = generated;
  p->blocked = ah.blocked;
  p->permitted = generated - ah.blocked;
  for (int i = 0; i < 16; i++) p->blocked_act[i] = ah.blocked_act[i];
  p->blocked_violating = ah.blocked_violating;
  p->blocked_viol_mask = ah.blocked_viol_mask;
  p->blocked_min_fp = ah.blocked_min_pfp;
  p->blocked_viol_min_fp = ah.blocked_viol_min_pfp;
  p->slices = slices; p->relisted = relisted; p->launches = launches;
  p->list_ms = list_ms; p->verdict_ms = verdict_ms; p->expand_ms = expand_ms;
}

// the last pass's figures added to the level it led into (a level takes many passes: one per sub-slice of its parents)
void action_deep_file(vsrmc_checker* c, int level, int kind) {
  vsrmc_action_constraint* a = c->action_constraint;
  if (!a || level < 2) return;
  if (a->deep_levels.size() <= (size_t)level) { a->deep_levels.resize((size_t)level + 1); a->deep_epochs.resize((size_t)level + 1, 0); }
  vsrmc_action_constraint_deep_info& d = a->deep_levels[(size_t)level];
  const vsrmc_action_constraint_deep_info& p = a->pass;
  if (d.kind != kind || a->deep_epochs[(size_t)level] != a->deep_epoch) {
    std::memset(&d, 0, sizeof(d));
    d.level = level;
    d.kind = kind;
    d.blocked_min_fp = d.blocked_viol_min_fp = ~(u64)0;
    a->deep_epochs[(size_t)level] = a->deep_epoch;
  }
  d.parents += p.parents; d.pairs += p.pairs; d.permitted += p.permitted; d.blocked += p.blocked;
  for (int i = 0; i < 16; i++) d.blocked_act[i] += p.blocked_act[i];
  d.blocked_violating += p.blocked_violating;
  d.blocked_viol_mask |= p.blocked_viol_mask;
  d.blocked_min_fp = std::min(d.blocked_min_fp, p.blocked_min_fp);
  d.blocked_viol_min_fp = std::min(d.blocked_viol_min_fp, p.blocked_viol_min_fp);
  d.slices += p.slices; d.relisted += p.relisted; d.launches += p.launches;
  d.list_ms += p.list_ms; d.verdict_ms += p.verdict_ms; d.expand_ms += p.expand_ms;
}

const vsrmc_where* action_constraint_program(const vsrmc_checker* c, int* k) {
  if (!c->action_constraint) return nullptr;
  *k = c->action_constraint->k;
  return &c->action_constraint->prog;
}

// phase 1 of a level with an action constraint attached, in the place of phase_expand (unsharded single-pass levels only: the attachment refuses the
// rest).  Slices of the current level through k_step_list, k_step_apply and k_step_expand; the control block is read back once, at the end.  Leaves
// c->h, c->nx_n and c->nx_w as phase_expand does, so that phase_commit, constrain_level and find_fp_newest run unchanged.
int phase_expand_gated(vsrmc_checker* c) {
  vsrmc_action_constraint* a = c->action_constraint;
  const Model& M = c->model.M;
  HIPCHK(hipSetDevice(c->opt.device));
  if (c->level + 1 >= 511) return fail(VSRMC_E_REP, "more than 510 BFS levels");
  c->t_level0 = now_s();
  c->expand_ms = c->materialize_ms = 0;
  std::memset(&c->h, 0, sizeof(c->h));
  c->h.viol_fp = ~(u64)0;
  c->level_fused = true;
  c->nx_n = c->nx_w = 0;
  c->full_recoverable = false;
  ActionCtl ah;
  std::memset(&ah, 0, sizeof(ah));
  ah.blocked_min_pfp = ah.blocked_viol_min_pfp = ~(u64)0;
  StepCtl sh = fresh_ctl<StepCtl>();
  HIPCHK(hipMemcpyAsync(c->ctl, &c->h, sizeof(c->h), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(a->d_actl, &ah, sizeof(ah), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(a->d_sctl, &sh, sizeof(sh), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));                         // (the sources are pageable host memory on this frame)
  auto* const apply_kernel = KERNEL_OF(k_step_apply, M);            // (where_fits at attach: the program is this model's)
  auto* const expand_kernel = KERNEL_OF(k_step_expand, M);
  const int nxt = c->cur ^ 1;
  const u64 nx_wcap = c->words_cap(nxt) > 256 ? c->words_cap(nxt) - 256 : 0;   // (a margin of one record: the writer copies the parent's words before it patches them)
  // the first slice cannot overflow the list even if every ordinal of every parent were enabled; the later ones are sized from the instances per parent the
  // slices before them showed (the largest mean of any slice of this level), times 1.5 — and a slice that overflows all the same is listed again in halves
  // before anything of it is applied (SlicePolicy, adaptive).  TEST KNOB (documented in include/vsrmc.h): VSRMC_ACTION_SLICE, parents per slice, fixed (no
  // adaptation: a halved slice grows back by doubling)
  const int bag = (c->bag_known && c->cur_max_bag) ? (int)std::min<u64>(c->cur_max_bag, (u64)M.max_bag) : M.max_bag;
  bool fixed_slice = false;
  const u64 slice = slice_initial(a->list_cap, ord_count(M, bag), "VSRMC_ACTION_SLICE", &fixed_slice);
  SlicePolicy sp(0, c->n_frontier, a->list_cap, slice, !fixed_slice, a->live_cap);
  double list_ms = 0, verdict_ms = 0, expand_ms = 0;
  u64 scanned = 0, launches = 0;
  bool timed = false;                                              // events 2..5 hold a slice whose kernel times have not been read yet
  auto collect = [&]() -> int {
    if (!timed) return 0;
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, a->ev[2], a->ev[3]));
    verdict_ms += (double)ms;
    HIPCHK(hipEventElapsedTime(&ms, a->ev[4], a->ev[5]));
    expand_ms += (double)ms;
    timed = false;
    return 0;
  };
  // The only synchronisation of a slice is the one behind its listing: apply and expand of slice i run while the host sets up the listing of slice i + 1,
  // and have finished when that listing has been waited for — their event times are read then (and once more after the loop).
  const StepListing listing{c->words[c->cur], c->off[c->cur], c->stream, c->num_cus, a->d_list, a->d_sctl, a->ev[0], a->ev[1], &list_ms};
  int rc = step_slices(
      M, listing, sp, "action constraint", &scanned,
      [&](u64 lo, u64 end) -> int {
        HIPCHK(hipMemsetAsync(a->d_live, 0, (end - lo) * 4, c->stream));
        return 0;
      },
      [&](u64 lo, u64, u64 n_inst) -> int {
        const int rcc = collect();                                 // (the slice before this one has finished as well)
        if (rcc) return rcc;
        const unsigned grid_a = scan_grid(n_inst, c->num_cus);
        HIPCHK(hipEventRecord(a->ev[2], c->stream));
        hipLaunchKernelGGL(apply_kernel, dim3(grid_a), dim3(256), 0, c->stream, M, (const u32*)a->d_prog, (int)a->prog.prog.names.size(), (const u64*)c->words[c->cur],
                           (const u64*)c->off[c->cur], (const u64*)nullptr, (const u64*)a->d_list, n_inst, a->d_sctl, (u64*)nullptr, (u64)0, a->d_rows);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(a->ev[3], c->stream));
        HIPCHK(hipEventRecord(a->ev[4], c->stream));
        hipLaunchKernelGGL(expand_kernel, dim3(grid_a), dim3(256), 0, c->stream, M, (const u64*)c->words[c->cur], (const u64*)c->off[c->cur], (const u64*)a->d_list,
                           (const u32*)a->d_rows, n_inst, a->k, c->level + 1, lo, c->table, c->tmask, c->words[nxt], nx_wcap, c->off[nxt], c->opt.frontier_states,
                           c->lvl_fp, c->ctl, a->d_actl, a->d_live);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(a->ev[5], c->stream));
        timed = true;
        launches += 2;
        return 0;
      });
  if (rc) return rc;
  const u64 slices = sp.listings, relisted = sp.relisted;
  launches += sp.listings;
  HIPCHK(hipMemcpyAsync(&c->h, c->ctl, sizeof(c->h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&ah, a->d_actl, sizeof(ah), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&sh, a->d_sctl, sizeof(sh), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  rc = collect();
  if (rc) return rc;
  c->expand_ms = list_ms + verdict_ms + expand_ms;
  if (scanned != c->n_valid) { c->failed = 1; return fail(VSRMC_E_HIP, "k_step_list: scanned " + std::to_string(scanned) + " records of " + std::to_string(c->n_valid)); }
  if (sh.n_internal) { c->failed = 1; return fail(VSRMC_E_HIP, "k_step_apply: " + std::to_string(sh.n_internal) + " listed instances are not enabled (guard_slot_pre and gen disagree)"); }
  c->h.deadlocks = scanned - ah.live_parents;
  if (!c->h.err && c->h.full) {                                    // the record buffers ran out: with a constraint attached vsrmc_checker_advance ends the run there
    c->h.err = ERR_FRONTIER_FULL;
    c->h.err_info = c->h.full_info << 16;
    c->full_recoverable = c->h.ties == 0;
    if (c->full_recoverable) { c->full_h = c->h; c->full_ms = c->expand_ms; c->full_t0 = c->t_level0; }
    // (with the opt-in for the levels beyond the buffers the host adopts the level: complete in the seen-set, every claim counted in n_new; its figures wait here)
    if (c->full_recoverable && a->deep_on) action_pass_figures(&a->pass, ah, scanned, c->h.generated, slices, relisted, launches, list_ms, verdict_ms, expand_ms);
  }
  if (c->h.err) return level_error(c, c->h, c->level + 1);
  c->nx_n = c->h.n_new;                                            // (dense: the index range is the number of states)
  c->nx_w = c->h.words_new;
  if (c->h.ties) {
    c->failed = 1;
    return fail(VSRMC_E_STATE, "two successors of one level share a VIEW fingerprint but differ in the aux variables (SURVEY F2); the single-pass scheme cannot arbitrate, "
                               "and an action constraint needs it");
  }
  vsrmc_action_constraint_info ai;
  std::memset(&ai, 0, sizeof(ai));
  ai.level = c->level + 1;
  ai.k = a->k;
  ai.parents = scanned;
  ai.pairs = c->h.generated;
  ai.blocked = ah.blocked;
  ai.permitted = c->h.generated - ah.blocked;
  for (int i = 0; i < 16; i++) ai.blocked_act[i] = ah.blocked_act[i];
  ai.blocked_violating = ah.blocked_violating;
  ai.blocked_viol_mask = ah.blocked_viol_mask;
  ai.blocked_min_fp = ah.blocked_min_pfp;
  ai.blocked_viol_min_fp = ah.blocked_viol_min_pfp;
  ai.n_new = c->h.n_written;
  ai.slices = slices; ai.relisted = relisted; ai.launches = launches;
  ai.list_ms = list_ms; ai.verdict_ms = verdict_ms; ai.expand_ms = expand_ms;
  if (a->levels.size() <= (size_t)ai.level) a->levels.resize((size_t)ai.level + 1);
  a->levels[(size_t)ai.level] = ai;
  a->newest = ai.level;
  if ((size_t)ai.level < a->deep_levels.size()) a->deep_levels[(size_t)ai.level].kind = 0;   // (probed by an earlier pass, stored now after a re-basing: this row is the level's, not both)
  return 0;
}

// One pass of the deep search through the gate, in the place of expand_pass (vsr_deep.hpp routes MODE_INSERT, MODE_NORMAL and MODE_PROBE here when
// vsrmc_checker_action_constrain_deep is on; MODE_REGEN keeps k_expand: DESIGN.md §9m): the `n` indices src_off[0 .. n) (holes included) through step_slices —
// k_step_list, k_step_apply (the verdict), k_step_expand in the pass's mode — with phase_expand_gated's slice policy, knobs and `live` words.
//   MODE_INSERT  nothing is written (GATE_INSERT): the control block comes back with n_new, fp_xor, fp_sum, max_bag as k_expand's MODE_INSERT leaves them
//   MODE_NORMAL  the level a descent inserts (GATE_STORED, the stored level's code) into dst: dense, so the index range c->h.n_new is the number of states
//   MODE_PROBE   nothing is inserted (GATE_PROBE): the violating candidates are in c->pending, c->h.n_pending of them
// The control blocks are read back once, when the last slice has been launched.  Leaves c->h as expand_pass does (deadlocks: parents scanned minus live
// ones), adds the kernels' time to c->expand_ms, the launches beyond the first to c->extra_launches, and the ActionCtl figures in a->pass for the caller to
// file under the level (action_deep_file).  p_off: the first index's place in its level, for the error message only.
int expand_pass_gated(vsrmc_checker* c, const u64* src_words, const u64* src_off, u64 n, u64 p_off, int level, int mode, u64 bag, const PassDst* dst) {
  vsrmc_action_constraint* a = c->action_constraint;
  const Model& M = c->model.M;
  if (!a || (mode != MODE_INSERT && mode != MODE_NORMAL && mode != MODE_PROBE) || (mode == MODE_NORMAL && !dst)) return fail(VSRMC_E_ARG, "expand_pass_gated: not a pass the gate runs");
  std::memset(&c->h, 0, sizeof(c->h));
  c->h.viol_fp = ~(u64)0;
  c->extra_launches = 0;
  ActionCtl ah;
  std::memset(&ah, 0, sizeof(ah));
  ah.blocked_min_pfp = ah.blocked_viol_min_pfp = ~(u64)0;
  action_pass_figures(&a->pass, ah, 0, 0, 0, 0, 0, 0, 0, 0);
  if (n == 0) return 0;
  StepCtl sh = fresh_ctl<StepCtl>();
  HIPCHK(hipMemcpyAsync(c->ctl, &c->h, sizeof(c->h), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(a->d_actl, &ah, sizeof(ah), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(a->d_sctl, &sh, sizeof(sh), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));                         // (the sources are pageable host memory on this frame)
  auto* const apply_kernel = KERNEL_OF(k_step_apply, M);
  auto* const expand_kernel = mode == MODE_NORMAL ? KERNEL_OF(k_step_expand, M) : mode == MODE_INSERT ? GATED_KERNEL_OF(M, GATE_INSERT) : GATED_KERNEL_OF(M, GATE_PROBE);
  // where the kernel writes: the scratch buffer's records (a margin of one record, as on a stored level), or — nothing written — the pending list
  u64* const out_words = mode == MODE_NORMAL ? dst->words : c->pending;
  const u64 out_cap = mode == MODE_NORMAL ? (dst->words_cap > 256 ? dst->words_cap - 256 : 0) : c->opt.pending_entries;
  u64* const out_off = mode == MODE_NORMAL ? dst->off : nullptr;
  u64* const out_fp = mode == MODE_NORMAL ? dst->fp : nullptr;
  const u64 out_n = mode == MODE_NORMAL ? dst->cap : 0;
  const int bg = (int)std::min<u64>(bag, (u64)M.max_bag);
  bool fixed_slice = false;
  const u64 slice = slice_initial(a->list_cap, ord_count(M, bg), "VSRMC_ACTION_SLICE", &fixed_slice);
  SlicePolicy sp(0, n, a->list_cap, slice, !fixed_slice, a->live_cap);
  double list_ms = 0, verdict_ms = 0, expand_ms = 0;
  u64 scanned = 0, launches = 0;
  bool timed = false;
  auto collect = [&]() -> int {
    if (!timed) return 0;
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, a->ev[2], a->ev[3]));
    verdict_ms += (double)ms;
    HIPCHK(hipEventElapsedTime(&ms, a->ev[4], a->ev[5]));
    expand_ms += (double)ms;
    timed = false;
    return 0;
  };
  const StepListing listing{src_words, src_off, c->stream, c->num_cus, a->d_list, a->d_sctl, a->ev[0], a->ev[1], &list_ms};
  int rc = step_slices(
      M, listing, sp, "action constraint", &scanned,
      [&](u64 lo, u64 end) -> int {
        HIPCHK(hipMemsetAsync(a->d_live, 0, (end - lo) * 4, c->stream));
        return 0;
      },
      [&](u64 lo, u64, u64 n_inst) -> int {
        const int rcc = collect();
        if (rcc) return rcc;
        const unsigned grid_a = scan_grid(n_inst, c->num_cus);
        HIPCHK(hipEventRecord(a->ev[2], c->stream));
        hipLaunchKernelGGL(apply_kernel, dim3(grid_a), dim3(256), 0, c->stream, M, (const u32*)a->d_prog, (int)a->prog.prog.names.size(), src_words, src_off,
                           (const u64*)nullptr, (const u64*)a->d_list, n_inst, a->d_sctl, (u64*)nullptr, (u64)0, a->d_rows);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(a->ev[3], c->stream));
        HIPCHK(hipEventRecord(a->ev[4], c->stream));
        hipLaunchKernelGGL(expand_kernel, dim3(grid_a), dim3(256), 0, c->stream, M, src_words, src_off, (const u64*)a->d_list, (const u32*)a->d_rows, n_inst, a->k, level, lo,
                           c->table, c->tmask, out_words, out_cap, out_off, out_n, out_fp, c->ctl, a->d_actl, a->d_live);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(a->ev[5], c->stream));
        timed = true;
        launches += 2;
        return 0;
      });
  if (rc) return rc;
  launches += sp.listings;
  HIPCHK(hipMemcpyAsync(&c->h, c->ctl, sizeof(c->h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&ah, a->d_actl, sizeof(ah), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&sh, a->d_sctl, sizeof(sh), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  rc = collect();
  if (rc) return rc;
  c->expand_ms += list_ms + verdict_ms + expand_ms;
  c->extra_launches = launches ? launches - 1 : 0;
  if (sh.n_internal) { c->failed = 1; return fail(VSRMC_E_HIP, "k_step_apply: " + std::to_string(sh.n_internal) + " listed instances are not enabled (guard_slot_pre and gen disagree)"); }
  c->h.deadlocks = scanned - ah.live_parents;
  if (c->h.err) c->h.err_info += p_off << 16;
  if (!c->h.err && !c->h.full && c->h.ties) {
    c->failed = 1;
    return fail(VSRMC_E_STATE, "two successors of one level share a VIEW fingerprint but differ in the aux variables (SURVEY F2); the single-pass scheme cannot arbitrate, "
                               "and an action constraint needs it");
  }
  action_pass_figures(&a->pass, ah, scanned, c->h.generated, sp.listings, sp.relisted, launches, list_ms, verdict_ms, expand_ms);
  return pass_verdict(c, level);                                   // (a full scratch buffer is an error here, as in expand_pass: the caller sized the slice)
}

// The behaviour along the fingerprints a walk through the seen-set gave (fps[0] = Init's), taking PERMITTED steps only: k_replay takes the smallest ordinal
// whose successor has the next fingerprint, permitted or not, so with an action constraint attached the path is rebuilt here instead — every state of it
// through the expand batch (successor fingerprints) and the step batch (verdicts), the smallest permitted ordinal that leads to the next fingerprint taken.
// Such an ordinal exists: the parent pointer of a stored state was written by a permitted transition.  Cost: per state of the path two batch calls of one
// record (vsrmc_expand_batch, vsrmc_step_batch), each with its own device allocations, copies and launches — a report's path, tens of states, not a hot path.
int action_constraint_trace(vsrmc_checker* c, const std::vector<u64>& fps, u64* words, u64 cap_words, u64* off, int32_t* actions, u64 cap_states, u64* n_states) {
  const vsrmc_action_constraint* a = c->action_constraint;
  const Model& M = c->model.M;
  const u64 level = fps.size();
  if (cap_states < level + 1) return fail(VSRMC_E_ARG, "state buffers too small");
  std::vector<u64> cur;
  init_record_wire(M, cur);
#ifdef VSRMC_TEST_HOOKS
  if (g_test_replay_start) cur.assign(g_test_replay_start, g_test_replay_start + M.h0 + hdr_nmsg(g_test_replay_start[0]));   // (a seeded search: as replay_path)
#endif
  u64 pos = 0;
  for (u64 t = 0; t < level; t++) {
    if (t > 0) {
      const u64 poff[2] = {0, (u64)cur.size()};
      const u64 cap = (u64)ord_count(M, hdr_nmsg(cur[0])) + 1, capw = cap * 256;
      std::vector<u64> ow(capw), om(cap * 8), rows(cap * 5);
      u64 n_out = 0, w_out = 0, n_rows = 0;
      int rc = vsrmc_expand_batch(&c->model, c->opt.device, cur.data(), poff, 1, ow.data(), capw, om.data(), cap, &n_out, &w_out);
      if (rc) return rc;
      rc = vsrmc_step_batch(&c->model, c->opt.device, &a->prog, cur.data(), poff, 1, rows.data(), cap, &n_rows);
      if (rc) return rc;
      u64 at = n_out;
      for (u64 k = 0; k < n_out && at == n_out; k++) {             // (both batches are in ordinal order)
        if (om[8 * k + 6] || om[8 * k + 3] != fps[t]) continue;
        for (u64 q = 0; q < n_rows; q++)
          if (rows[5 * q + 1] == om[8 * k + 1] && !rows[5 * q + 4] && ((rows[5 * q + 3] >> a->k) & 1)) { at = k; break; }
      }
      if (at == n_out) return fail(VSRMC_E_STATE, "action constraint: a state of the path has no permitted step to the next fingerprint");
      const u64 wo = om[8 * at + 7], len = (u64)M.h0 + (u64)hdr_nmsg(ow[wo]);
      cur.assign(&ow[wo], &ow[wo] + len);
      actions[t] = (int32_t)om[8 * at + 2];
    } else {
      actions[0] = 0;
    }
    if (pos + cur.size() > cap_words) return fail(VSRMC_E_ARG, "word buffer too small");
    off[t] = pos;
    std::copy(cur.begin(), cur.end(), words + pos);
    pos += cur.size();
  }
  off[level] = pos;
  *n_states = level;
  return 0;
}

}  // namespace

extern "C" {

int32_t vsrmc_checker_action_constrain_attach(vsrmc_checker* c, const vsrmc_where* w, int32_t name_index) {
  if (!c) return fail(VSRMC_E_ARG, "NULL argument");
  if (c->opt.world > 1) return fail(VSRMC_E_STATE, "action constraint: sharded checkers (world > 1) are not constrained");
  if (c->opt.exact_ties) return fail(VSRMC_E_STATE, "action constraint: exact_ties = 1 (the two-kernel scheme claims the seen-set before a successor is materialised; the gate needs the single-pass scheme)");
  if (!w) {                                                        // detach, at any level: the search starts over unconstrained
    if (!c->action_constraint) return 0;
    HIPCHK(hipSetDevice(c->opt.device));
    action_constraint_free(c);
    return checker_seed(c);
  }
  if (c->level != 1 || c->total_generated != 0 || c->failed || c->deep || c->deep_regen_done)
    return fail(VSRMC_E_STATE, "action constraint: attached at level 1 only, to a fresh checker or after vsrmc_checker_reset (every transition of the search is subject to it)");
  if (deep_constrain_on(c)) return fail(VSRMC_E_STATE, "action constraint: the state constraint is applied beyond the record buffers (vsrmc_checker_constrain_deep): the transitions there are not judged, an action constraint needs stored levels");
  if (c->deep_attach) return fail(VSRMC_E_STATE, "action constraint: predicates are attached for the levels beyond the record buffers (vsrmc_checker_deep_attach): those levels are not constrained");
  if (c->deep_term) return fail(VSRMC_E_STATE, "action constraint: the terminal attachment (vsrmc_checker_deep_terminal_attach) is for the levels beyond the record buffers: those levels are not constrained");
  if (!w->prog.step) return fail(VSRMC_E_ARG, "action constraint: a state program (vsrmc_where_compile) judges a state; an action constraint is a step predicate (vsrmc_step_predicates_compile: vsrmc_where_desc.step)");
  if (!where_fits(w, c->model.M, c->model.symmetry)) return fail(VSRMC_E_ARG, "action constraint: compiled for another model");
  if (name_index < 0 || (size_t)name_index >= w->prog.names.size()) return fail(VSRMC_E_ARG, "action constraint: the program exports no predicate of that index");
  if (constraint_reads_aux(w->prog))
    return fail(VSRMC_E_ARG, "action constraint: the program reads aux_svc or aux_client_acked (primed or not), which are outside VIEW: of the copies of one state the one that "
                             "arrived first would decide which transitions are taken");
  if (c->action_constraint) return fail(VSRMC_E_STATE, "action constraint: one is attached already (NULL detaches it)");
  HIPCHK(hipSetDevice(c->opt.device));
  vsrmc_action_constraint* a = new vsrmc_action_constraint();
  a->prog = *w;
  a->k = name_index;
  a->list_cap = ACTION_LIST_CAP;
  // TEST KNOB (documented in include/vsrmc.h): a shorter instance list, so that slices of a small level overflow it and are listed again in halves
  if (const char* e = std::getenv("VSRMC_ACTION_LIST_CAP")) a->list_cap = std::max<u64>(64, std::min<u64>(ACTION_LIST_CAP, std::strtoull(e, nullptr, 10)));
  a->live_cap = std::max<u64>(64, std::min<u64>(a->list_cap, c->opt.frontier_states));
  c->action_constraint = a;
  (void)a->mem.upload(&a->d_prog, w->prog.ops.data(), w->prog.ops.size(), WHERE_MAX_OPS);
  (void)a->mem.alloc(&a->d_list, a->list_cap * 8);
  (void)a->mem.alloc(&a->d_rows, a->list_cap * 4);
  (void)a->mem.alloc(&a->d_live, a->live_cap * 4);
  (void)a->mem.alloc(&a->d_sctl, sizeof(StepCtl));
  hipError_t e = a->mem.alloc(&a->d_actl, sizeof(ActionCtl));
  for (hipEvent_t& ev : a->ev)
    if (e == hipSuccess) e = hipEventCreate(&ev);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    action_constraint_free(c);
    return fail(VSRMC_E_HIP, std::string("action constraint: ") + hipGetErrorString(e));
  }
  return checker_seed(c);                                          // (a fresh search: the state constraint, if one is attached, evaluates Init again)
}

int32_t vsrmc_checker_action_constraint_info(vsrmc_checker* c, int32_t level, vsrmc_action_constraint_info* out) {
  if (!c || !out) return fail(VSRMC_E_ARG, "NULL argument");
  std::memset(out, 0, sizeof(*out));
  const vsrmc_action_constraint* a = c->action_constraint;
  if (!a) return fail(VSRMC_E_STATE, "no action constraint attached (vsrmc_checker_action_constrain_attach)");
  if (level == 0) level = a->newest;                               // the level the last step led into
  if (level < 2 || (size_t)level >= a->levels.size() || a->levels[(size_t)level].level != level) return fail(VSRMC_E_ARG, "action constraint: no step has led into that level");
  *out = a->levels[(size_t)level];
  return 0;
}

int32_t vsrmc_checker_action_constrain_deep(vsrmc_checker* c, int32_t on) {
  if (!c) return fail(VSRMC_E_ARG, "NULL argument");
  vsrmc_action_constraint* a = c->action_constraint;
  if (!a) return fail(VSRMC_E_STATE, "action_constrain_deep: no action constraint attached (vsrmc_checker_action_constrain_attach)");
  if (c->level != 1 || c->total_generated != 0 || c->failed || c->deep || c->deep_regen_done)
    return fail(VSRMC_E_STATE, "action_constrain_deep: at level 1 only, right after the action constraint was attached or after vsrmc_checker_reset");
  if (!on) { a->deep_on = false; return 0; }
  if (c->constraint)
    return fail(VSRMC_E_STATE, deep_constrain_on(c) ? "action_constrain_deep: the state constraint is applied beyond the record buffers (vsrmc_checker_constrain_deep): the two together beyond the buffers are not built yet"
                                                    : "action_constrain_deep: a state constraint is attached (vsrmc_checker_constrain_attach): the record-less pass beyond the record buffers cannot judge states, "
                                                      "so the two together are not taken there");
  if (c->deep_attach) return fail(VSRMC_E_STATE, "action_constrain_deep: predicates are attached for the levels beyond the record buffers (vsrmc_checker_deep_attach): their scans do not know the gate");
  if (c->deep_term) return fail(VSRMC_E_STATE, "action_constrain_deep: the terminal attachment (vsrmc_checker_deep_terminal_attach) scans passes that do not know the gate");
  if (c->opt.world > 1) return fail(VSRMC_E_STATE, "action_constrain_deep: sharded checkers (world > 1) are not constrained");
  if (c->opt.exact_ties) return fail(VSRMC_E_STATE, "action_constrain_deep: levels beyond the record buffers need a single-pass checker (exact_ties is set)");
  a->deep_levels.clear();
  a->deep_epochs.clear();
  a->deep_on = true;
  return 0;
}

int32_t vsrmc_checker_action_constraint_deep_info(vsrmc_checker* c, int32_t level, vsrmc_action_constraint_deep_info* out) {
  if (!c || !out) return fail(VSRMC_E_ARG, "NULL argument");
  std::memset(out, 0, sizeof(*out));
  const vsrmc_action_constraint* a = c->action_constraint;
  if (!a || !a->deep_on) return fail(VSRMC_E_STATE, "the action constraint is not applied beyond the record buffers (vsrmc_checker_action_constrain_deep)");
  if (level < 2 || (size_t)level >= a->deep_levels.size() || a->deep_levels[(size_t)level].kind == 0)
    return fail(VSRMC_E_ARG, "action constraint: not a level a gated pass beyond the record buffers led into");
  *out = a->deep_levels[(size_t)level];
  return 0;
}

// the seen-set's load as the table itself shows it: the slots that hold a fingerprint, counted on the host from a copy (a figure for tests and reports, not for a
// hot path: the whole table crosses the bus)
int32_t vsrmc_checker_seen_set_load(vsrmc_checker* c, uint64_t* occupied, uint64_t* slots) {
  if (!c || !occupied || !slots) return fail(VSRMC_E_ARG, "NULL argument");
  *occupied = 0;
  *slots = c->tmask + 1;
  HIPCHK(hipSetDevice(c->opt.device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const u64 window = (u64)1 << 20;
  std::vector<Slot> buf((size_t)std::min<u64>(window, *slots));
  for (u64 first = 0; first < *slots; first += window) {
    const u64 n = std::min<u64>(window, *slots - first);
    HIPCHK(hipMemcpy(buf.data(), c->table + first, n * sizeof(Slot), hipMemcpyDeviceToHost));
    for (u64 i = 0; i < n; i++) *occupied += buf[i].fp != 0;
  }
  return 0;
}

}  // extern "C"
