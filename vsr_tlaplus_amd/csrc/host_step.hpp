// host_step.hpp — step predicates: the host side of k_step_list / k_step_apply (vsr_step.hpp) — compiling a text with primes (vsr_where_parse.hpp;
// vsrmc_step_predicates_compile for any model, vsrmc_step_compile for VSR.tla alone), picking the model's instantiation, a
// caller's batch, the scan of the checker's newest stored level over slices (a consumer of step_slices, host_step_slices.hpp), the hit pairs the last
// scan left (included by vsrmc.hip: one translation unit, the sections share its anonymous-namespace helpers).
#pragma once

namespace {

enum : u64 { STEP_LIST_CAP = (u64)1 << 22, STEP_HIT_CAP = (u64)1 << 20 };

struct StepRun {
  StepCtl h;                           // counters over every slice (h.scanned = parents of the accepted slices)
  double list_ms = 0, apply_ms = 0;    // HIP-event time of the two kernels, summed over the slices
  u64 slices = 0, retried = 0;         // launches of the pair of kernels; slices run again with half the parents after the list overflowed
  std::vector<u64> hits;               // 4 words per kept hit pair
  std::vector<u64> row_entry;          // want_rows: every list entry (parent index | ordinal << 40) ...
  std::vector<u32> row_val;            // ... and action | bits << 8 | err << 16 beside it
};

struct StepBufs {
  DevMem mem;
  u64 *list = nullptr, *hits = nullptr;
  StepCtl* ctl = nullptr;
  u32 *prog = nullptr, *rows = nullptr;
  // a constrained checker's scan: the constraint's program, its verdicts, its counters (not reported), the permitted entries of the list and their number
  u32 *gate_prog = nullptr, *gate_rows = nullptr;
  StepCtl* gate_ctl = nullptr;
  u64 *kept = nullptr, *n_kept = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~StepBufs() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// parents per slice: the list cannot overflow when every ordinal of every parent of a slice is enabled (bag_bound = the largest bag a record can have);
// TEST KNOB (documented in include/vsrmc.h): VSRMC_STEP_SLICE, parents per slice
u64 step_slice_default(const Model& M, int bag_bound, u64 list_cap) { return slice_initial(list_cap, ord_count(M, bag_bound), "VSRMC_STEP_SLICE"); }

// the records refs[lo, hi) through both kernels, slice by slice (step_slices, host_step_slices.hpp: a slice that offered more than the list holds is listed
// again in two halves, nothing of it having been applied).
// `gate` (a checker with an action constraint attached): exported predicate gate_k of that step program says which transitions the model
// takes.  Every slice's list then goes through k_step_apply with the GATE's program first and through k_step_keep, and `w` runs over the permitted
// instances only: counts, minima, hits and rows are those of the constrained model.  apply_ms then holds all three launches of a slice.
int step_run(const Model& M, const vsrmc_where* w, int num_cus, hipStream_t stream, const u64* d_words, const u64* d_refs, const u64* d_fps, u64 lo, u64 hi,
             u64 slice, u64 list_cap, u64 hit_cap, bool want_rows, StepRun* out, const vsrmc_where* gate = nullptr, int gate_k = 0) {
  StepBufs b;
  hit_cap = d_fps ? std::max<u64>(1, hit_cap) : 1;
  HIPCHK(b.mem.alloc(&b.list, list_cap * 8));
  HIPCHK(b.mem.alloc(&b.hits, hit_cap * 32));
  HIPCHK(b.mem.alloc(&b.ctl, sizeof(StepCtl)));
  HIPCHK(b.mem.alloc(&b.prog, WHERE_MAX_OPS * sizeof(u32)));
  if (want_rows) HIPCHK(b.mem.alloc(&b.rows, list_cap * 4));
  if (gate) {
    HIPCHK(b.mem.alloc(&b.gate_prog, WHERE_MAX_OPS * sizeof(u32)));
    HIPCHK(b.mem.alloc(&b.gate_rows, list_cap * 4));
    HIPCHK(b.mem.alloc(&b.gate_ctl, sizeof(StepCtl)));
    HIPCHK(b.mem.alloc(&b.kept, list_cap * 8));
    HIPCHK(b.mem.alloc(&b.n_kept, 8));
    HIPCHK(hipMemsetAsync(b.gate_ctl, 0, sizeof(StepCtl), stream));
    HIPCHK(hipMemcpyAsync(b.gate_prog, gate->prog.ops.data(), gate->prog.ops.size() * sizeof(u32), hipMemcpyHostToDevice, stream));
  }
  for (hipEvent_t& e : b.ev) HIPCHK(hipEventCreate(&e));
  const StepCtl init = fresh_ctl<StepCtl>();
  HIPCHK(hipMemcpyAsync(b.ctl, &init, sizeof(init), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(b.prog, w->prog.ops.data(), w->prog.ops.size() * sizeof(u32), hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));
  auto* const apply_kernel = KERNEL_OF(k_step_apply, M);            // (where_fits: the program is this model's)
  u64 scanned = 0;
  SlicePolicy sp(lo, hi, list_cap, slice);
  const StepListing listing{d_words, d_refs, stream, num_cus, b.list, b.ctl, b.ev[0], b.ev[1], &out->list_ms};
  int rc = step_slices(M, listing, sp, "step scan", &scanned, nullptr, [&](u64, u64, u64 n_inst) -> int {
    const unsigned grid_a = scan_grid(n_inst, num_cus);
    HIPCHK(hipEventRecord(b.ev[2], stream));
    const u64* d_list = b.list;
    if (gate) {                                                    // the constraint's verdicts, then the entries it permits (n_inst <= list_cap = the room of kept[])
      HIPCHK(hipMemsetAsync(b.n_kept, 0, 8, stream));
      hipLaunchKernelGGL(apply_kernel, dim3(grid_a), dim3(256), 0, stream, M, (const u32*)b.gate_prog, (int)gate->prog.names.size(), d_words, d_refs, (const u64*)nullptr,
                         (const u64*)b.list, n_inst, b.gate_ctl, (u64*)nullptr, (u64)0, b.gate_rows);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(k_step_keep, dim3(grid_a), dim3(256), 0, stream, (const u64*)b.list, (const u32*)b.gate_rows, n_inst, gate_k, b.kept, b.n_kept);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(&n_inst, b.n_kept, 8, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      d_list = b.kept;
    }
    if (n_inst) {
      hipLaunchKernelGGL(apply_kernel, dim3(grid_a), dim3(256), 0, stream, M, (const u32*)b.prog, (int)w->prog.names.size(), d_words, d_refs, d_fps, d_list, n_inst,
                         b.ctl, d_fps ? b.hits : nullptr, hit_cap, b.rows);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(b.ev[3], stream));
    HIPCHK(hipStreamSynchronize(stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, b.ev[2], b.ev[3]));
    out->apply_ms += (double)ms;
    if (want_rows && n_inst) {
      const size_t at = out->row_entry.size();
      out->row_entry.resize(at + n_inst);
      out->row_val.resize(at + n_inst);
      HIPCHK(hipMemcpy(out->row_entry.data() + at, d_list, n_inst * 8, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(out->row_val.data() + at, b.rows, n_inst * 4, hipMemcpyDeviceToHost));
    }
    return 0;
  });
  out->slices += sp.listings;
  out->retried += sp.relisted;
  if (rc) return rc;
  HIPCHK(hipMemcpy(&out->h, b.ctl, sizeof(StepCtl), hipMemcpyDeviceToHost));
  out->h.scanned = scanned;
  if (gate) {
    StepCtl gh;
    HIPCHK(hipMemcpy(&gh, b.gate_ctl, sizeof(StepCtl), hipMemcpyDeviceToHost));
    out->h.n_internal += gh.n_internal;
  }
  if (out->h.n_internal) return fail(VSRMC_E_HIP, "k_step_apply: " + std::to_string(out->h.n_internal) + " listed instances are not enabled (guard_slot_pre and gen disagree)");
  const u64 kept = d_fps ? std::min<u64>(out->h.n_hits, hit_cap) : 0;
  out->hits.resize(kept * 4);
  if (kept) HIPCHK(hipMemcpy(out->hits.data(), b.hits, kept * 32, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" {

int32_t vsrmc_step_compile(const vsrmc_model* m, const char* text, vsrmc_where** out) {
  if (!m || !text || !out) return fail(VSRMC_E_ARG, "NULL argument");
  *out = nullptr;
  if (m->M.model_id != 0) return fail(VSRMC_E_ARG, "step predicates: VSR.tla only");
  return compile_predicates(m, text, true, out);
}

// the model-generic entry: VSR.tla -> what vsrmc_step_compile gives, op for op; the analysis models -> the step language over their own variable table
int32_t vsrmc_step_predicates_compile(const vsrmc_model* m, const char* text, vsrmc_where** out) {
  if (!m || !text || !out) return fail(VSRMC_E_ARG, "NULL argument");
  if (m->M.model_id == 0) return vsrmc_step_compile(m, text, out);
  return compile_predicates(m, text, true, out);
}

int32_t vsrmc_step_batch(const vsrmc_model* m, int32_t device, const vsrmc_where* w, const uint64_t* words, const uint64_t* off, uint64_t n, uint64_t* rows,
                         uint64_t cap_rows, uint64_t* n_rows) {
  if (!m || !w || !words || !off || !n_rows) return fail(VSRMC_E_ARG, "NULL argument");
  *n_rows = 0;
  if (!w->prog.step) return fail(VSRMC_E_ARG, "step predicates: the program was compiled by vsrmc_where_compile (vsrmc_step_compile / vsrmc_step_predicates_compile compile a step program)");
  if (!where_fits(w, m->M, m->symmetry)) return fail(VSRMC_E_ARG, "step predicates: compiled for another model");
  int rc = check_device(device);
  if (rc) return rc;
  if (n == 0) return 0;
  const Model& M = m->M;
  DevMem mem;
  u64 *d_words = nullptr, *d_refs = nullptr;
  int bag = 0;
  rc = stage_batch(M, words, off, n, beyond_max_bag, mem, &d_words, &d_refs, &bag);
  if (rc) return rc;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  const u64 list_cap = std::min<u64>(STEP_LIST_CAP, std::max<u64>(64, n * (u64)ord_count(M, bag)));
  StepRun run;
  rc = step_run(M, w, prop.multiProcessorCount, nullptr, d_words, d_refs, nullptr, 0, n, step_slice_default(M, bag, list_cap), list_cap, 0, true, &run);
  if (rc) return rc;
  if (run.h.scanned != n) return fail(VSRMC_E_HIP, "k_step_list: the scan did not cover the batch");
  const u64 total = run.row_entry.size();
  *n_rows = total;
  if (!rows) return 0;                                            // size query
  if (cap_rows < total) return fail(VSRMC_E_ARG, "row buffer too small");
  const std::vector<u64> order = sorted_order(total, [&](u64 a, u64 b) {        // (parent, ordinal): the order of vsrmc_expand_batch
    const u64 ea = run.row_entry[a], eb = run.row_entry[b];
    if (origin_pidx(ea) != origin_pidx(eb)) return origin_pidx(ea) < origin_pidx(eb);
    return origin_ord(ea) < origin_ord(eb);
  });
  for (u64 k = 0; k < total; k++) {
    const u64 e = run.row_entry[order[k]];
    const u32 v = run.row_val[order[k]];
    rows[5 * k] = origin_pidx(e);
    rows[5 * k + 1] = (u64)origin_ord(e);
    rows[5 * k + 2] = v & 0xFF;
    rows[5 * k + 3] = (v >> 8) & 0xFF;
    rows[5 * k + 4] = (v >> 16) & 0xFF;
  }
  return 0;
}

int32_t vsrmc_checker_step_scan(vsrmc_checker* c, const vsrmc_where* w, vsrmc_step_info* out) {
  if (!c || !w || !out) return fail(VSRMC_E_ARG, "NULL argument");
  std::memset(out, 0, sizeof(*out));
  out->level = c->level;
  for (int k = 0; k < WHERE_MAX_EXPORTS; k++) { out->min_fp[k] = out->min_index[k] = ~(u64)0; out->min_ordinal[k] = ~(uint32_t)0; out->min_action[k] = -1; }
  if (!w->prog.step) return fail(VSRMC_E_ARG, "step predicates: the program was compiled by vsrmc_where_compile (vsrmc_step_compile / vsrmc_step_predicates_compile compile a step program)");
  if (!where_fits(w, c->model.M, c->model.symmetry)) return fail(VSRMC_E_ARG, "step predicates: compiled for another model");
  if (c->opt.world > 1) return fail(VSRMC_E_STATE, "step scan: sharded checkers are not scanned");
  if (c->deep || c->deep_regen_done || c->full_recoverable)
    return fail(VSRMC_E_STATE, "step scan: the deepest complete level exists in the seen-set only (vsrmc_checker_deepen): it has no records to scan; it is not examined");
  if (c->failed) return fail(VSRMC_E_STATE, "step scan: the search has stopped with an error");
  c->step_fps.clear();
  c->step_ords.clear();
  c->step_bits.clear();
  c->step_total = 0;
  c->step_level = c->level;
  if (c->n_frontier == 0) return 0;
  HIPCHK(hipSetDevice(c->opt.device));
  const Model& M = c->model.M;
  u64 hit_cap = STEP_HIT_CAP;
  // TEST KNOB (documented in include/vsrmc.h): a smaller hit list, so that a test can reach the overflow path on a small space
  if (const char* e = std::getenv("VSRMC_STEP_LIST_CAP")) hit_cap = std::min<u64>(hit_cap, std::max<u64>(1, std::strtoull(e, nullptr, 10)));
  // the largest bag among the level's records where the checker knows it, else the capacity (a wrong bound costs a slice run again, never a result)
  const int bag = (c->bag_known && c->cur_max_bag) ? (int)std::min<u64>(c->cur_max_bag, (u64)M.max_bag) : M.max_bag;
  const u64 list_cap = std::min<u64>(STEP_LIST_CAP, std::max<u64>(64, c->n_frontier * (u64)ord_count(M, bag)));
  hit_cap = std::min<u64>(hit_cap, std::max<u64>(1, c->n_frontier * (u64)ord_count(M, M.max_bag)));   // (no level has more pairs than that)
  // with an action constraint attached the scan is one of the constrained model: the transitions the constraint blocks are not judged, counted or listed
  int gate_k = 0;
  const vsrmc_where* gate = action_constraint_program(c, &gate_k);
  StepRun run;
  int rc = step_run(M, w, c->num_cus, c->stream, c->words[c->cur], c->off[c->cur], c->lvl_fp, 0, c->n_frontier, step_slice_default(M, bag, list_cap), list_cap,
                    hit_cap, false, &run, gate, gate_k);
  if (rc) return rc;
  const StepCtl& h = run.h;
  if (h.scanned != c->n_valid) return fail(VSRMC_E_HIP, "k_step_list: scanned " + std::to_string(h.scanned) + " records of " + std::to_string(c->n_valid));
  out->n_states = h.scanned;
  out->n_pairs = h.n_pairs;
  out->n_err = h.n_err;
  out->list_ms = run.list_ms;
  out->apply_ms = run.apply_ms;
  out->kernel_ms = run.list_ms + run.apply_ms;
  out->slices = run.slices;
  for (int k = 0; k < WHERE_MAX_EXPORTS; k++) { out->count[k] = h.count[k]; out->min_fp[k] = h.min_fp[k]; }
  const u64 kept = run.hits.size() / 4;
  const std::vector<u64> order = sorted_order(kept, [&](u64 a, u64 b) {
    if (run.hits[4 * a] != run.hits[4 * b]) return run.hits[4 * a] < run.hits[4 * b];
    return run.hits[4 * a + 2] < run.hits[4 * b + 2];
  });
  c->step_fps.resize(kept);
  c->step_ords.resize(kept);
  c->step_bits.resize(kept);
  for (u64 k = 0; k < kept; k++) {
    c->step_fps[k] = run.hits[4 * order[k]];
    c->step_ords[k] = (uint32_t)run.hits[4 * order[k] + 2];
    c->step_bits[k] = (uint8_t)run.hits[4 * order[k] + 3];
  }
  c->step_total = h.n_hits;
  // the witness of predicate k: the parent with the smallest fingerprint, and of its instances the smallest ordinal with bit k — that one record through
  // the kernels again (the hit list may have overflowed, and it does not hold the action)
  for (int p = 0; p < WHERE_MAX_EXPORTS; p++) {
    if (!h.count[p]) continue;
    bool done = false;
    for (int q = 0; q < p && !done; q++)
      if (h.count[q] && h.min_fp[q] == h.min_fp[p]) { out->min_index[p] = out->min_index[q]; done = true; }
    if (!done && (rc = find_fp_newest(c, h.min_fp[p], &out->min_index[p]))) return rc;
    if (out->min_index[p] == ~(u64)0) return fail(VSRMC_E_HIP, "step scan: the parent of a witness is not in the level");
    StepRun one;
    const u64 cap1 = (u64)std::max(64, ord_count(M, M.max_bag));
    rc = step_run(M, w, c->num_cus, c->stream, c->words[c->cur], c->off[c->cur], nullptr, out->min_index[p], out->min_index[p] + 1, 1, cap1, 0, true, &one, gate, gate_k);
    if (rc) return rc;
    for (size_t k = 0; k < one.row_entry.size(); k++) {
      const u32 v = one.row_val[k];
      const uint32_t ord = (uint32_t)origin_ord(one.row_entry[k]);
      if (((v >> (8 + p)) & 1) && ord < out->min_ordinal[p]) { out->min_ordinal[p] = ord; out->min_action[p] = (int32_t)(v & 0xFF); }
    }
    if (out->min_action[p] < 0) return fail(VSRMC_E_HIP, "step scan: the witness pair was not found again");
  }
  return 0;
}

int32_t vsrmc_checker_step_successor(vsrmc_checker* c, uint64_t index, uint32_t ordinal, const uint64_t* parent, uint64_t parent_words, uint64_t* words,
                                     uint64_t cap_words, uint64_t* n_words, int32_t* action) {
  if (!c || !words || !n_words) return fail(VSRMC_E_ARG, "NULL argument");
  *n_words = 0;
  if (c->step_level < 0 || c->step_level != c->level || c->deep || c->deep_regen_done)
    return fail(VSRMC_E_STATE, "step successor: the level of the last step scan is no longer the newest stored level");
  if (index >= c->n_frontier) return fail(VSRMC_E_ARG, "index outside the level");
  HIPCHK(hipSetDevice(c->opt.device));
  const Model& M = c->model.M;
  u64 ref = 0;
  HIPCHK(hipMemcpy(&ref, c->off[c->cur] + index, 8, hipMemcpyDeviceToHost));
  if (ref == 0) return fail(VSRMC_E_ARG, "index is a withdrawn index of the level");
  std::vector<u64> dev(ref & 0xFF), wire(512);
  HIPCHK(hipMemcpy(dev.data(), c->words[c->cur] + (ref >> 8), dev.size() * 8, hipMemcpyDefault));
  device_to_wire(M, dev.data(), wire.data());
  const u64 off[2] = {0, (u64)M.h0 + (u64)hdr_nmsg(dev[0])};
  const u64 cap = (u64)ord_count(M, hdr_nmsg(dev[0])) + 1, capw = cap * 256;
  std::vector<u64> ow(capw), om(cap * 8);
  u64 n_out = 0, w_out = 0;
  int rc = vsrmc_expand_batch(&c->model, c->opt.device, wire.data(), off, 1, ow.data(), capw, om.data(), cap, &n_out, &w_out);
  if (rc) return rc;
  u64 at = n_out;
  for (u64 k = 0; k < n_out && at == n_out; k++)
    if (om[8 * k + 1] == ordinal) at = k;
  if (at == n_out) return fail(VSRMC_E_ARG, "the ordinal is not enabled in that record");
  if (om[8 * at + 6]) return fail(VSRMC_E_ARG, "the instance raises an evaluation error: it has no successor");
  if (parent) {
    // the same step out of the caller's record of that state (a trace's last record: under SYMMETRY it may be another member of the state's orbit, with
    // another bag order): the successor with the same action and the same fingerprint
    const u64 want_act = om[8 * at + 2], want_fp = om[8 * at + 3];
    if (parent_words != (u64)M.h0 + (u64)hdr_nmsg(parent[0])) return fail(VSRMC_E_ARG, "record length does not match its header");
    const u64 poff[2] = {0, parent_words};
    const u64 cap2 = (u64)ord_count(M, hdr_nmsg(parent[0])) + 1;
    ow.assign(cap2 * 256, 0);
    om.assign(cap2 * 8, 0);
    rc = vsrmc_expand_batch(&c->model, c->opt.device, parent, poff, 1, ow.data(), cap2 * 256, om.data(), cap2, &n_out, &w_out);
    if (rc) return rc;
    at = n_out;
    for (u64 k = 0; k < n_out && at == n_out; k++)
      if (!om[8 * k + 6] && om[8 * k + 2] == want_act && om[8 * k + 3] == want_fp) at = k;
    if (at == n_out) return fail(VSRMC_E_ARG, "the record given is not the state the pair starts from");
  }
  const u64 wo = om[8 * at + 7], len = (u64)M.h0 + (u64)hdr_nmsg(ow[wo]);
  if (len > cap_words) return fail(VSRMC_E_ARG, "buffer too small");
  std::copy(&ow[wo], &ow[wo] + len, words);
  *n_words = len;
  if (action) *action = (int32_t)om[8 * at + 2];
  return 0;
}

int32_t vsrmc_checker_step_pairs(vsrmc_checker* c, uint64_t* fps, uint32_t* ordinals, uint8_t* bits, uint64_t cap, uint64_t* n) {
  if (!c || !n) return fail(VSRMC_E_ARG, "NULL argument");
  *n = 0;
  if (c->step_level < 0) return fail(VSRMC_E_STATE, "no step scan yet (vsrmc_checker_step_scan)");
  *n = c->step_total;
  const u64 kept = c->step_fps.size();
  if (fps) {
    if (cap < kept) return fail(VSRMC_E_ARG, "buffer too small");
    std::copy(c->step_fps.begin(), c->step_fps.end(), fps);
    if (ordinals) std::copy(c->step_ords.begin(), c->step_ords.end(), ordinals);
    if (bits) std::copy(c->step_bits.begin(), c->step_bits.end(), bits);
  }
  if (c->step_total > kept)
    return fail(VSRMC_E_REP, "step pairs: level " + std::to_string(c->step_level) + " has " + std::to_string(c->step_total) + ", the list holds the " + std::to_string(kept) +
                                 " that arrived first (counters and minima of the scan are exact)");
  return 0;
}

}  // extern "C"
