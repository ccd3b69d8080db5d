// host_deep_constrain.hpp — the state constraint on the levels beyond the record buffers: the host side of k_constrain_slice (vsr_deep_constrain.hpp;
// DESIGN.md §9l) — the opt-in, the three places a descent of the deep search (vsr_deep.hpp) calls while it is on, the per-level deep figures (included by
// vsrmc.hip: one translation unit, the sections share its anonymous-namespace helpers).
//
// A descent resets the control blocks of its levels once (deep_constrain_begin), launches the filter on every scratch slice before anything reads it
// (deep_constrain_slice: no copy and no synchronisation for a regenerated slice; the inserted sub-slice's block is copied back, where the host waited for
// k_level_checksum before), and reads the blocks once when it is over (deep_constrain_end): a level filtered for the first time gets its
// vsrmc_constraint_info there, a level filtered before must have come back with the very figures it was recorded with.
#pragma once

namespace {

bool deep_constrain_on(const vsrmc_checker* c) { return c->constraint && c->constraint->deep.on; }

ConstrainCtl deep_constrain_fresh() {
  ConstrainCtl init;
  std::memset(&init, 0, sizeof(init));
  init.pruned_min_fp = ~(u64)0;
  for (int p = 0; p < WHERE_MAX_EXPORTS; p++) init.p_min_fp[p] = ~(u64)0;
  return init;
}

// the deepest level whose states have all been judged: every stored level is (constrain_level), and the deep levels a descent has recorded
int deep_constrain_filtered_through(const vsrmc_checker* c) { return std::max(c->level, c->constraint->deep.filtered_through); }

// before a descent over the levels first .. last (last = the inserted level, or the newest regenerated one of a re-basing descent)
int deep_constrain_begin(vsrmc_checker* c, int first, int last) {
  DeepConstrainState& D = c->constraint->deep;
  D.first = D.last = 0;
  if (first > last) return 0;
  if (last >= 512) return fail(VSRMC_E_REP, "more than 510 BFS levels");
  if (D.levels.size() <= (size_t)last) D.levels.resize((size_t)last + 1);
  D.count.assign((size_t)last + 1, 0);
  const int ft = deep_constrain_filtered_through(c);
  int n_rec = 0;
  D.list_level[0] = D.list_level[1] = 0;
  for (int lv = last; lv >= first; lv--)                            // the newest level takes the attachment's own list, as a stored level does
    if (lv > ft) {
      if (n_rec == 2) return fail(VSRMC_E_STATE, "constraint: more than two unfiltered levels beyond the record buffers");
      D.list_level[n_rec++] = lv;
    }
  std::vector<ConstrainCtl> init((size_t)(last - first + 1), deep_constrain_fresh());
  HIPCHK(hipMemcpyAsync(D.d_blocks + first, init.data(), init.size() * sizeof(ConstrainCtl), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));                         // (the source is pageable host memory on this frame)
  D.first = first;
  D.last = last;
  return 0;
}

// one scratch slice of `level` (index range `part` of B, holes included), right after k_expand wrote it.  inserted != nullptr: the sub-slice of the
// inserted level — the level's block so far comes back (the host waits here, as it did for the checksum this replaces)
int deep_constrain_slice(vsrmc_checker* c, const PassDst& B, u64 part, int level, ConstrainCtl* inserted) {
  vsrmc_constraint* a = c->constraint;
  DeepConstrainState& D = a->deep;
  if (level < D.first || level > D.last) return fail(VSRMC_E_STATE, "constraint: a scratch slice of a level the descent did not announce");
  if (!part) return 0;
  const Model& M = c->model.M;
  u64* list = nullptr;
  u64 cap = 0;
  if (level == D.list_level[0]) { list = a->d_list; cap = a->list_cap; }
  else if (level == D.list_level[1]) { list = D.d_list2; cap = a->list_cap; }
  // TEST KNOBS (include/vsrmc.h): the ones of constrain_level
  if (cap) if (const char* e = std::getenv("VSRMC_WHERE_LIST_CAP")) cap = std::min<u64>(cap, std::max<u64>(1, std::strtoull(e, nullptr, 10)));
  u64 grid64 = scan_grid(part, c->num_cus);
  if (const char* e = std::getenv("VSRMC_CONSTRAIN_GRID")) grid64 = std::max<u64>(1, std::min<u64>(grid64, std::strtoull(e, nullptr, 10)));
  hipLaunchKernelGGL(KERNEL_OF(k_constrain_slice, M), dim3((unsigned)grid64), dim3(256), 0, c->stream, M, (const u32*)a->d_prog, (int)a->prog.prog.names.size(), a->k,
                     (const u64*)B.words, B.off, B.fp, part, D.d_blocks + level, list, cap);
  HIPCHK(hipGetLastError());
  D.count[(size_t)level]++;
  if (inserted) {
    HIPCHK(hipMemcpyAsync(inserted, D.d_blocks + level, sizeof(ConstrainCtl), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return 0;
}

// the descent is over (rc: how).  base = the stored level it started from; last_regen = the deepest regenerated level.  Records the figures of the levels
// filtered for the first time, corrects the bookkeeping of a regenerated one among them (a level that reached the seen-set before a record of it could be
// judged: deep_first_pass, adopt_overflowed_level), checks the others.
int deep_constrain_end(vsrmc_checker* c, int rc, int base, int last_regen) {
  vsrmc_constraint* a = c->constraint;
  DeepConstrainState& D = a->deep;
  const int first = D.first, last = D.last;
  D.first = D.last = 0;
  if (rc || !first) return rc;
  std::vector<ConstrainCtl> h((size_t)(last - first + 1));
  HIPCHK(hipMemcpy(h.data(), D.d_blocks + first, h.size() * sizeof(ConstrainCtl), hipMemcpyDeviceToHost));
  const int ft = deep_constrain_filtered_through(c);
  u64 cap = a->list_cap;
  if (const char* e = std::getenv("VSRMC_WHERE_LIST_CAP")) cap = std::min<u64>(cap, std::max<u64>(1, std::strtoull(e, nullptr, 10)));
  bool newest_set = false;
  for (int lv = last; lv >= first; lv--) {
    const ConstrainCtl& b = h[(size_t)(lv - first)];
    DeepConstrainLevel& L = D.levels[(size_t)lv];
    const bool regenerated = lv <= last_regen;
    DeepLevelRec* dl = (regenerated && (size_t)(lv - base - 1) < c->deep_lv.size()) ? &c->deep_lv[(size_t)(lv - base - 1)] : nullptr;
    L.launches += D.count[(size_t)lv];
    if (regenerated) { L.regen_records += b.kept + b.pruned; L.regen_pruned += b.pruned; }
    if (lv <= ft) {                                                // recorded by an earlier descent: the same states came back and got the same verdicts
      if (dl && (b.kept != dl->n_new || b.kept + b.pruned != dl->n_local)) {
        c->failed = 1;
        return fail(VSRMC_E_STATE, "constraint: level " + std::to_string(lv) + " was recorded with " + std::to_string((unsigned long long)dl->n_new) + " in-model states of " +
                                       std::to_string((unsigned long long)dl->n_local) + ", this descent regenerated " + std::to_string((unsigned long long)b.kept) + " of " +
                                       std::to_string((unsigned long long)(b.kept + b.pruned)));
      }
      continue;
    }
    if (!regenerated && b.kept + b.pruned == 0) continue;            // the descent found nothing to insert: there is no such level
    const bool listed = lv == D.list_level[0] || lv == D.list_level[1];
    if (dl && b.kept + b.pruned != dl->n_local) {
      c->failed = 1;
      return fail(VSRMC_E_STATE, "constraint: level " + std::to_string(lv) + " has " + std::to_string((unsigned long long)dl->n_local) + " states in the seen-set, the descent regenerated " +
                                     std::to_string((unsigned long long)(b.kept + b.pruned)));
    }
    if (!listed || b.n_list != b.pruned) { c->failed = 1; return fail(VSRMC_E_HIP, "k_constrain_slice: the pruned list of level " + std::to_string(lv) + " does not match its count"); }
    vsrmc_constraint_info ci;
    std::memset(&ci, 0, sizeof(ci));
    ci.level = lv;
    ci.k = a->k;
    ci.n_states = b.kept + b.pruned;
    ci.kept = b.kept; ci.pruned = b.pruned;
    ci.kept_xor = b.kept_xor; ci.kept_sum = b.kept_sum; ci.kept_max_bag = b.kept_max_bag; ci.kept_words = b.kept_words;
    ci.pruned_min_fp = b.pruned_min_fp;
    for (int p = 0; p < WHERE_MAX_EXPORTS; p++) { ci.pruned_count[p] = b.p_count[p]; ci.pruned_min_fp_k[p] = b.p_min_fp[p]; }
    if (a->levels.size() <= (size_t)lv) a->levels.resize((size_t)lv + 1);
    a->levels[(size_t)lv] = ci;
    L.kind = regenerated ? 1 : 2;
    L.slices = D.count[(size_t)lv];
    L.list_overflowed = b.n_list > cap;
    c->table_pruned += b.pruned;
    if (dl) {                                                      // its unfiltered figures went into the bookkeeping when it was inserted
      dl->n_new = b.kept;                                          // (n_local stays: what a descent regenerates, kept + pruned)
      c->deep_distinct -= b.pruned;
    }
    // the pruned list leaves the device now: the next descent appends to the same buffers
    std::vector<u64> fps((size_t)std::min<u64>(b.n_list, cap));
    if (!fps.empty()) HIPCHK(hipMemcpy(fps.data(), lv == D.list_level[0] ? a->d_list : D.d_list2, fps.size() * 8, hipMemcpyDeviceToHost));
    std::sort(fps.begin(), fps.end());
    if (!newest_set) {                                             // the newest recorded level: what vsrmc_checker_constraint_pruned and level 0 of _constraint_info name
      newest_set = true;
      a->pruned_fps.swap(fps);
      a->pruned_held = a->pruned_fps.size();
      a->pruned_total = b.n_list;
      a->pruned_fetched = true;
      a->pruned_level = lv;
      D.other_level = 0; D.other_fps.clear(); D.other_total = 0;
    } else {
      D.other_level = lv;
      D.other_fps.swap(fps);
      D.other_total = b.n_list;
    }
    D.filtered_through = std::max(D.filtered_through, lv);
  }
  return 0;
}

// after a descent: a newest seen-set-only level of which nothing is in the model is no level — the search is exhausted at the one below (the seen-set keeps
// the pruned one: traceable by fingerprint, like the stored path's `beyond`)
void deep_constrain_drop_empty(vsrmc_checker* c) {
  vsrmc_constraint* a = c->constraint;
  if (c->deep && !c->deep_lv.empty() && c->deep_lv.back().n_new == 0 && c->level + c->deep <= a->deep.filtered_through) {
    c->deep_lv.pop_back();
    c->deep -= 1;
  }
  a->beyond = a->deep.filtered_through > c->level + c->deep ? 1 : 0;   // (the inserted level of a descent that kept nothing of it was never counted in c->deep)
}

u64 deep_constrain_pruned_of(const vsrmc_checker* c, int level) {
  const vsrmc_constraint* a = c->constraint;
  return (size_t)level < a->levels.size() && a->levels[(size_t)level].level == level ? a->levels[(size_t)level].pruned : 0;
}

}  // namespace

extern "C" {

int32_t vsrmc_checker_constrain_deep(vsrmc_checker* c, int32_t on) {
  if (!c) return fail(VSRMC_E_ARG, "NULL argument");
  vsrmc_constraint* a = c->constraint;
  if (!a) return fail(VSRMC_E_STATE, "constrain_deep: no constraint attached (vsrmc_checker_constrain_attach)");
  if (c->level != 1 || c->total_generated != 0 || c->failed || c->deep || c->deep_regen_done)
    return fail(VSRMC_E_STATE, "constrain_deep: at level 1 only, right after the constraint was attached or after vsrmc_checker_reset");
  if (!on) { a->deep.on = false; return 0; }
  if (c->action_constraint) return fail(VSRMC_E_STATE, "constrain_deep: an action constraint is attached: beyond the record buffers only a state constraint is applied, the transitions there are not judged");
  if (c->opt.world > 1) return fail(VSRMC_E_STATE, "constrain_deep: sharded checkers (world > 1) are not constrained");
  if (c->opt.exact_ties) return fail(VSRMC_E_STATE, "constrain_deep: levels beyond the record buffers need a single-pass checker (exact_ties is set)");
  HIPCHK(hipSetDevice(c->opt.device));
  DeepConstrainState& D = a->deep;
  if (!D.d_blocks) {
    if (a->mem.alloc(&D.d_blocks, 512 * sizeof(ConstrainCtl)) != hipSuccess || a->mem.alloc(&D.d_list2, a->list_cap * 8) != hipSuccess) {
      const hipError_t e = a->mem.err;
      (void)hipGetLastError();
      a->mem.err = hipSuccess;
      D.d_blocks = nullptr;                                        // (what was allocated stays with the attachment and is freed with it)
      return fail(VSRMC_E_HIP, std::string("constrain_deep: ") + hipGetErrorString(e));
    }
  }
  D.restart();
  D.on = true;
  return 0;
}

int32_t vsrmc_checker_constraint_deep_info(vsrmc_checker* c, int32_t level, vsrmc_constraint_deep_info* out) {
  if (!c || !out) return fail(VSRMC_E_ARG, "NULL argument");
  std::memset(out, 0, sizeof(*out));
  const vsrmc_constraint* a = c->constraint;
  if (!a || !a->deep.on) return fail(VSRMC_E_STATE, "the constraint is not applied beyond the record buffers (vsrmc_checker_constrain_deep)");
  const DeepConstrainState& D = a->deep;
  out->level = level;
  if ((size_t)level < D.levels.size() && D.levels[(size_t)level].kind) {
    const DeepConstrainLevel& L = D.levels[(size_t)level];
    out->kind = L.kind;
    out->filtered = 1;
    out->list_overflowed = L.list_overflowed ? 1 : 0;
    out->slices = L.slices;
    out->launches = L.launches;
    out->regen_records = L.regen_records;
    out->regen_pruned = L.regen_pruned;
    return 0;
  }
  if (level > c->level && level <= c->level + c->deep && level > deep_constrain_filtered_through(c)) {   // in the seen-set, not judged yet: the next descent regenerates and filters it
    out->kind = 1;
    return 0;
  }
  return fail(VSRMC_E_ARG, "constraint: not a level that was filtered beyond the record buffers");
}

int32_t vsrmc_checker_constraint_pruned_level(vsrmc_checker* c, int32_t level, uint64_t* fps, uint64_t cap, uint64_t* n) {
  if (!c || !n) return fail(VSRMC_E_ARG, "NULL argument");
  *n = 0;
  vsrmc_constraint* a = c->constraint;
  if (!a) return fail(VSRMC_E_STATE, "no constraint attached (vsrmc_checker_constrain_attach)");
  if (level == 0 || level == a->pruned_level) return vsrmc_checker_constraint_pruned(c, fps, cap, n);
  if (!a->deep.on || level != a->deep.other_level) return fail(VSRMC_E_ARG, "constraint: the pruned list of that level is not kept (the levels the last filtering descent recorded, or the newest stored level)");
  *n = a->deep.other_total;
  const u64 held = a->deep.other_fps.size();
  if (fps) {
    if (cap < held) return fail(VSRMC_E_ARG, "buffer too small");
    std::copy(a->deep.other_fps.begin(), a->deep.other_fps.end(), fps);
  }
  if (a->deep.other_total > held)
    return fail(VSRMC_E_REP, "constraint: level " + std::to_string(level) + " has " + std::to_string(a->deep.other_total) + " pruned states, the list holds the " + std::to_string(held) +
                                 " that arrived first (counts and minima are exact)");
  return 0;
}

}  // extern "C"
