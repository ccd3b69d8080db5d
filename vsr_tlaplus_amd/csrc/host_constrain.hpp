// host_constrain.hpp — state constraints: the host side of k_constrain (vsr_constrain.hpp) — attaching one exported predicate of a compiled
// state program to a checker, the filter step_local runs on every level it has just committed, the per-level figures, the list of the newest level's
// pruned states (included by vsrmc.hip: one translation unit, the sections share its anonymous-namespace helpers).
#pragma once

// what the opt-in for the levels beyond the record buffers adds to an attachment (vsrmc_checker_constrain_deep; host_deep_constrain.hpp)
struct DeepConstrainLevel {            // one level that was (or still is to be) filtered in a scratch buffer
  int kind = 0;                        // 1: first filtered as a regenerated level, 2: as the inserted level of a descent
  bool list_overflowed = false;
  u64 slices = 0;                      // scratch slices of the descent that recorded its figures
  u64 launches = 0, regen_records = 0, regen_pruned = 0;   // over every descent since: k_constrain_slice launches; records regenerated, and the pruned ones among them
};
struct DeepConstrainState {
  bool on = false;
  ConstrainCtl* d_blocks = nullptr;    // one control block per level (index = level), on the device for the whole descent
  u64* d_list2 = nullptr;              // a second pruned list: a descent records at most two levels (one regenerated for the first time, the inserted one)
  int filtered_through = 0;            // the deepest level beyond the record buffers whose figures are recorded
  int first = 0, last = 0;             // the levels of the descent in flight (0: none)
  int list_level[2] = {0, 0};          // which level appends to d_list / d_list2 in the descent in flight
  std::vector<DeepConstrainLevel> levels;   // [level]
  std::vector<u64> count;              // [level]: launches of the descent in flight
  int other_level = 0;                 // the last recording descent's OTHER level (the regenerated one when it recorded two): its pruned list, ascending
  std::vector<u64> other_fps;
  u64 other_total = 0;
  void restart() { filtered_through = first = last = 0; list_level[0] = list_level[1] = 0; levels.clear(); count.clear(); other_level = 0; other_fps.clear(); other_total = 0; }
};

struct vsrmc_constraint {
  vsrmc_where prog;                    // a copy: the caller may destroy its own
  int k = 0;                           // the exported predicate that is the constraint
  DevMem mem;                          // owns the device buffers: allocated once per attachment, freed with it
  u32* d_prog = nullptr;               // the program (uploaded once) ..
  ConstrainCtl* d_ctl = nullptr;       // .. the control block of one launch ..
  u64* d_list = nullptr;               // .. and the pruned fingerprints of one level
  u64 list_cap = 0;
  std::vector<vsrmc_constraint_info> levels;   // [level]: the figures of every level filtered since the search started (level 0 unused)
  std::vector<u64> pruned_fps;         // the newest filtered level's pruned states, ascending (the first list_cap that arrived): copied from d_list and sorted when asked for
  u64 pruned_held = 0;                 // entries of d_list that hold them
  bool pruned_fetched = true;
  double write_ratio = 1.0;            // (kept + pruned) / kept of the newest filtered level: what next_level_fits scales its in-model prediction by
  u64 pruned_total = 0;
  int pruned_level = 0;
  int beyond = 0;                      // 1: the last filtered level had no in-model state — it is level c->level + 1 in the seen-set, the search is exhausted
  DeepConstrainState deep;             // off unless vsrmc_checker_constrain_deep turned it on
};

namespace {

// does the program read aux_svc or aux_client_acked (header bits 8..19, outside VIEW: vsr_model.hpp)?  The op codes show it.
bool constraint_reads_aux(const WhereProgram& p) {
  for (const u32 op : p.ops) {
    if ((op >> 24) != (u32)W_LDBITS) continue;
    const u32 arg = op & 0xFFFFFFu, word = arg & 0xFF, shift = (arg >> 8) & 63, width = (arg >> 14) & 63;
    if (word == 0 && shift + width > 8 && shift < 20) return true;
  }
  return false;
}

void constraint_free(vsrmc_checker* c) {
  vsrmc_constraint* a = c->constraint;
  if (!a) return;
  delete a;
  c->constraint = nullptr;
}

int constraint_beyond(const vsrmc_checker* c) { return c->constraint ? c->constraint->beyond : 0; }
double constraint_write_ratio(const vsrmc_checker* c) { return c->constraint ? c->constraint->write_ratio : 1.0; }

// The filter: k_constrain over the newest stored level (index range c->n_frontier of buffer c->cur), before anything else reads it.  Afterwards the
// checker's figures of the level are the in-model ones; info (may be NULL: Init) is rewritten to match.  `generated`, the per-action counts and the
// violation fields stay k_expand's.
int constrain_level(vsrmc_checker* c, vsrmc_level_info* info) {
  vsrmc_constraint* a = c->constraint;
  if (!a || c->n_frontier == 0) return 0;
  const Model& M = c->model.M;
  HIPCHK(hipSetDevice(c->opt.device));
  ConstrainCtl init;
  std::memset(&init, 0, sizeof(init));
  init.pruned_min_fp = ~(u64)0;
  for (int p = 0; p < WHERE_MAX_EXPORTS; p++) init.p_min_fp[p] = ~(u64)0;
  HIPCHK(hipMemcpyAsync(a->d_ctl, &init, sizeof(init), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));                         // (the source is pageable host memory on this frame)
  const u64 n = c->n_frontier;
  u64 cap = a->list_cap;
  // TEST KNOBS (documented in include/vsrmc.h): a shorter list, so that a test reaches the overflow path on a small space; fewer blocks, so that a small
  // level drives the grid-stride loop through several trips
  if (const char* e = std::getenv("VSRMC_WHERE_LIST_CAP")) cap = std::min<u64>(cap, std::max<u64>(1, std::strtoull(e, nullptr, 10)));
  u64 grid64 = scan_grid(n, c->num_cus);
  if (const char* e = std::getenv("VSRMC_CONSTRAIN_GRID")) grid64 = std::max<u64>(1, std::min<u64>(grid64, std::strtoull(e, nullptr, 10)));
  HIPCHK(hipEventRecord(c->ev[2], c->stream));
  hipLaunchKernelGGL(KERNEL_OF(k_constrain, M), dim3((unsigned)grid64), dim3(256), 0, c->stream, M, (const u32*)a->d_prog, (int)a->prog.prog.names.size(), a->k,
                     (const u64*)c->words[c->cur], c->off[c->cur], c->lvl_fp, n, a->d_ctl, a->d_list, cap);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev[3], c->stream));
  ConstrainCtl h;
  HIPCHK(hipMemcpyAsync(&h, a->d_ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
  if (h.kept + h.pruned != c->n_valid || h.n_list != h.pruned) {
    c->failed = 1;
    return fail(VSRMC_E_HIP, "k_constrain: looked at " + std::to_string(h.kept + h.pruned) + " records of " + std::to_string(c->n_valid));
  }
  const int level = c->level;
  vsrmc_constraint_info ci;
  std::memset(&ci, 0, sizeof(ci));
  ci.level = level;
  ci.k = a->k;
  ci.n_states = c->n_valid;
  ci.kept = h.kept; ci.pruned = h.pruned;
  ci.kept_xor = h.kept_xor; ci.kept_sum = h.kept_sum; ci.kept_max_bag = h.kept_max_bag; ci.kept_words = h.kept_words;
  ci.pruned_min_fp = h.pruned_min_fp;
  for (int p = 0; p < WHERE_MAX_EXPORTS; p++) { ci.pruned_count[p] = h.p_count[p]; ci.pruned_min_fp_k[p] = h.p_min_fp[p]; }
  ci.kernel_ms = (double)ms;
  if (a->levels.size() <= (size_t)level) a->levels.resize((size_t)level + 1);
  a->levels[(size_t)level] = ci;
  a->pruned_held = std::min<u64>(h.n_list, cap);                   // (the list stays on the device until somebody asks: vsrmc_checker_constraint_pruned)
  a->pruned_fetched = false;
  a->pruned_fps.clear();
  a->pruned_total = h.n_list;
  a->write_ratio = h.kept ? (double)(h.kept + h.pruned) / (double)h.kept : 1.0;
  c->table_pruned += h.pruned;
  a->pruned_level = level;
  // the level's bookkeeping: the in-model figures (cur_max_bag stays k_expand's: an upper bound is all the next launch's LDS slots need)
  c->distinct -= h.pruned;
  c->n_valid = h.kept;
  c->hist_new[1] = h.kept;
  c->cur_rec_w = h.kept_words;
  a->beyond = 0;
  if (h.kept == 0) {                                               // nothing of the level is in the model: the search is exhausted, as after a step that found no new state —
    if (level > 1) { c->cur ^= 1; c->level -= 1; a->beyond = 1; }  // the newest level with a state is the one before (its records are spent), the seen-set keeps the pruned one
    c->n_frontier = 0;
    // (hist_new[0], cur_w, cur_max_bag and g_last keep the abandoned level's values: with an empty frontier no launch and no prediction reads them again, and
    // checker_seed sets every one of them when the search starts over)
  }
  if (info) {
    info->n_new = h.kept;
    info->record_words = h.kept_words;
    info->distinct = c->distinct;
    info->level = c->level;
  }
  return 0;
}

// a search that starts over (checker_seed): the attachment stays, its results go, Init is evaluated again
int constraint_restart(vsrmc_checker* c) {
  vsrmc_constraint* a = c->constraint;
  if (!a) return 0;
  a->levels.clear();
  a->pruned_fps.clear();
  a->pruned_total = 0;
  a->pruned_held = 0;
  a->pruned_fetched = true;
  a->write_ratio = 1.0;
  a->pruned_level = 0;
  a->beyond = 0;
  a->deep.restart();
  return constrain_level(c, nullptr);
}

#ifdef VSRMC_TEST_HOOKS
// TEST HOOK (host_test_seed.hpp): level 1 of a seeded search is the caller's records, subject to no constraint — what constraint_restart has just made of Init
// (its level-1 figures, a pruned Init's seen-set slot in table_pruned, its count in hist_new) goes, the attachment stays
void constraint_forget_init(vsrmc_checker* c) {
  c->table_pruned = 0;
  c->hist_new[1] = 0;
  vsrmc_constraint* a = c->constraint;
  if (!a) return;
  a->levels.clear();
  a->pruned_fps.clear();
  a->pruned_total = 0;
  a->pruned_held = 0;
  a->pruned_fetched = true;
  a->write_ratio = 1.0;
  a->pruned_level = 0;
  a->beyond = 0;
  a->deep.restart();
}
#endif

}  // namespace

extern "C" {

int32_t vsrmc_checker_constrain_attach(vsrmc_checker* c, const vsrmc_where* w, int32_t name_index) {
  if (!c) return fail(VSRMC_E_ARG, "NULL argument");
  if (c->opt.world > 1) return fail(VSRMC_E_STATE, "constraint: sharded checkers (world > 1) are not constrained");
  if (c->level != 1 || c->total_generated != 0 || c->failed || c->deep || c->deep_regen_done)
    return fail(VSRMC_E_STATE, "constraint: attached at level 1 only, to a fresh checker or after vsrmc_checker_reset (Init is subject to it)");
  if (c->deep_attach) return fail(VSRMC_E_STATE, "constraint: predicates are attached for the levels beyond the record buffers (vsrmc_checker_deep_attach): those levels are not constrained");
  if (c->deep_term) return fail(VSRMC_E_STATE, "constraint: the terminal attachment (vsrmc_checker_deep_terminal_attach) is for the levels beyond the record buffers: those levels are not constrained");
  if (!w) {                                                        // detach: the search starts over unconstrained
    if (!c->constraint) return 0;
    HIPCHK(hipSetDevice(c->opt.device));
    constraint_free(c);
    return checker_seed(c);
  }
  if (action_deep_on(c)) return fail(VSRMC_E_STATE, "constraint: the action constraint is applied beyond the record buffers (vsrmc_checker_action_constrain_deep): the record-less pass there cannot judge states, "
                                                    "so a state constraint is not taken beside it");
  if (w->prog.step) return fail(VSRMC_E_ARG, "constraint: a step program (vsrmc_step_compile) runs over pairs; a constraint is a state predicate");
  if (!where_fits(w, c->model.M, c->model.symmetry)) return fail(VSRMC_E_ARG, "constraint: compiled for another model");
  if (name_index < 0 || (size_t)name_index >= w->prog.names.size()) return fail(VSRMC_E_ARG, "constraint: the program exports no predicate of that index");
  if (constraint_reads_aux(w->prog))
    return fail(VSRMC_E_ARG, "constraint: the program reads aux_svc or aux_client_acked, which are outside VIEW: of the copies of one state the one that arrived first would "
                             "decide its membership");
  if (c->constraint) return fail(VSRMC_E_STATE, "constraint: one is attached already (NULL detaches it)");
  HIPCHK(hipSetDevice(c->opt.device));
  vsrmc_constraint* a = new vsrmc_constraint();
  a->prog = *w;
  a->k = name_index;
  a->list_cap = std::max<u64>(1, std::min<u64>(c->opt.frontier_states, (u64)1 << 20));   // fingerprints kept per level; the counters and minima do not come from the list
  c->constraint = a;
  (void)a->mem.upload(&a->d_prog, w->prog.ops.data(), w->prog.ops.size(), WHERE_MAX_OPS);
  (void)a->mem.alloc(&a->d_ctl, sizeof(ConstrainCtl));
  const hipError_t e = a->mem.alloc(&a->d_list, a->list_cap * 8);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    constraint_free(c);
    return fail(VSRMC_E_HIP, std::string("constraint: ") + hipGetErrorString(e));
  }
  const int rc = constraint_restart(c);                            // Init, at once
  if (rc) constraint_free(c);
  return rc;
}

int32_t vsrmc_checker_constraint_info(vsrmc_checker* c, int32_t level, vsrmc_constraint_info* out) {
  if (!c || !out) return fail(VSRMC_E_ARG, "NULL argument");
  std::memset(out, 0, sizeof(*out));
  const vsrmc_constraint* a = c->constraint;
  if (!a) return fail(VSRMC_E_STATE, "no constraint attached (vsrmc_checker_constrain_attach)");
  if (level == 0) level = a->pruned_level;                         // the newest filtered level
  if (level < 1 || (size_t)level >= a->levels.size() || a->levels[(size_t)level].level != level) return fail(VSRMC_E_ARG, "constraint: no such level has been filtered");
  *out = a->levels[(size_t)level];
  return 0;
}

int32_t vsrmc_checker_constraint_pruned(vsrmc_checker* c, uint64_t* fps, uint64_t cap, uint64_t* n) {
  if (!c || !n) return fail(VSRMC_E_ARG, "NULL argument");
  *n = 0;
  vsrmc_constraint* a = c->constraint;
  if (!a) return fail(VSRMC_E_STATE, "no constraint attached (vsrmc_checker_constrain_attach)");
  *n = a->pruned_total;
  if (!a->pruned_fetched) {                                        // the first call after the level was filtered: the list leaves the device now
    HIPCHK(hipSetDevice(c->opt.device));
    a->pruned_fps.resize(a->pruned_held);
    if (a->pruned_held) HIPCHK(hipMemcpy(a->pruned_fps.data(), a->d_list, a->pruned_held * 8, hipMemcpyDeviceToHost));
    std::sort(a->pruned_fps.begin(), a->pruned_fps.end());
    a->pruned_fetched = true;
  }
  const u64 held = a->pruned_fps.size();
  if (fps) {
    if (cap < held) return fail(VSRMC_E_ARG, "buffer too small");
    std::copy(a->pruned_fps.begin(), a->pruned_fps.end(), fps);
  }
  if (a->pruned_total > held)
    return fail(VSRMC_E_REP, "constraint: level " + std::to_string(a->pruned_level) + " has " + std::to_string(a->pruned_total) + " pruned states, the list holds the " +
                                 std::to_string(held) + " that arrived first (counts and minima are exact)");
  return 0;
}

}  // extern "C"
