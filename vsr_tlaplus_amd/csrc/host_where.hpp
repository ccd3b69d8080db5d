// host_where.hpp — state predicates: the host side of k_where (vsr_where.hpp) — compiling a text (vsr_where_parse.hpp; vsrmc_predicates_compile for any model,
// vsrmc_where_compile for VSR.tla alone; both through compile_predicates, host_scan_common.hpp, where vsrmc_where lives), a caller's batch, the scan of
// the checker's newest stored level, the list the last scan left (included by vsrmc.hip: one translation unit, the sections share its
// anonymous-namespace helpers).
#pragma once

namespace {

bool where_fits(const vsrmc_where* w, const Model& M, int symmetry) {
  return w->model_id == M.model_id && w->R == M.R && w->C == M.C && w->n == M.n && w->L == M.L && w->symmetry == symmetry;
}

// one launch over n refs; the program is uploaded and the WhereCtl at d_ctl initialised here (d_prog: room for WHERE_MAX_OPS ops); e0 / e1, when given,
// are recorded around the kernel alone
int launch_where(const Model& M, const vsrmc_where* w, int num_cus, hipStream_t stream, u32* d_prog, const u64* d_words, const u64* d_refs, const u64* d_fps, u64 n,
                 uint8_t* d_flags, WhereCtl* d_ctl, u64* d_list, u64 list_cap, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
  const WhereCtl init = fresh_ctl<WhereCtl>();
  HIPCHK(hipMemcpyAsync(d_ctl, &init, sizeof(init), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_prog, w->prog.ops.data(), w->prog.ops.size() * sizeof(u32), hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));                            // (both sources are pageable host memory that the caller may free)
  if (e0) HIPCHK(hipEventRecord(e0, stream));
  hipLaunchKernelGGL(KERNEL_OF(k_where, M), dim3(scan_grid(n, num_cus)), dim3(256), 0, stream, M, (const u32*)d_prog, (int)w->prog.names.size(), d_words, d_refs, d_fps, n, d_flags, d_ctl, d_list,
                     list_cap);
  HIPCHK(hipGetLastError());
  if (e1) HIPCHK(hipEventRecord(e1, stream));
  return 0;
}

}  // namespace

extern "C" {

int32_t vsrmc_where_compile(const vsrmc_model* m, const char* text, vsrmc_where** out) {
  if (!m || !text || !out) return fail(VSRMC_E_ARG, "NULL argument");
  *out = nullptr;
  if (m->M.model_id != 0) return fail(VSRMC_E_ARG, "state predicates: VSR.tla only");
  return compile_predicates(m, text, false, out);
}

// the model-generic entry: VSR.tla -> what vsrmc_where_compile gives, op for op; the analysis models -> their own variable table (vsr_where_parse.hpp)
int32_t vsrmc_predicates_compile(const vsrmc_model* m, const char* text, vsrmc_where** out) {
  if (!m || !text || !out) return fail(VSRMC_E_ARG, "NULL argument");
  if (m->M.model_id == 0) return vsrmc_where_compile(m, text, out);
  return compile_predicates(m, text, false, out);
}

void vsrmc_where_destroy(vsrmc_where* w) { delete w; }

int32_t vsrmc_where_describe(const vsrmc_where* w, vsrmc_where_desc* out) {
  if (!w || !out) return fail(VSRMC_E_ARG, "NULL argument");
  std::memset(out, 0, sizeof(*out));
  out->n_names = (int32_t)w->prog.names.size();
  out->n_ops = (int32_t)w->prog.ops.size();
  out->depth = w->prog.depth;
  out->msg_loops = w->prog.msg_loops;
  out->n_bodies = w->prog.n_bodies;
  out->step = w->prog.step ? 1 : 0;
  for (size_t k = 0; k < w->prog.names.size(); k++) std::snprintf(out->names[k], sizeof(out->names[k]), "%s", w->prog.names[k].c_str());
  return 0;
}

int32_t vsrmc_where_batch(const vsrmc_model* m, int32_t device, const vsrmc_where* w, const uint64_t* words, const uint64_t* off, uint64_t n, uint8_t* flags) {
  if (!m || !w || !words || !off || !flags) return fail(VSRMC_E_ARG, "NULL argument");
  if (w->prog.step) return fail(VSRMC_E_ARG, "state predicates: a step program (vsrmc_step_compile) runs over pairs: vsrmc_step_batch");
  if (!where_fits(w, m->M, m->symmetry)) return fail(VSRMC_E_ARG, "state predicates: compiled for another model");
  int rc = check_device(device);
  if (rc) return rc;
  if (n == 0) return 0;
  const Model& M = m->M;
  DevMem mem;
  u64 *d_words = nullptr, *d_refs = nullptr;
  uint8_t* d_flags = nullptr;
  WhereCtl* d_ctl = nullptr;
  u32* d_prog = nullptr;
  rc = stage_batch(M, words, off, n, longer_than_255, mem, &d_words, &d_refs);
  if (rc) return rc;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  HIPCHK(mem.alloc(&d_flags, n));
  HIPCHK(mem.alloc(&d_ctl, sizeof(WhereCtl)));
  HIPCHK(mem.alloc(&d_prog, WHERE_MAX_OPS * sizeof(u32)));
  HIPCHK(hipMemset(d_flags, 0, n));
  rc = launch_where(M, w, prop.multiProcessorCount, nullptr, d_prog, d_words, d_refs, nullptr, n, d_flags, d_ctl, nullptr, 0);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize());
  WhereCtl h;
  HIPCHK(hipMemcpy(&h, d_ctl, sizeof(h), hipMemcpyDeviceToHost));
  if (h.scanned != n) return fail(VSRMC_E_HIP, "k_where: the scan did not cover the batch");
  HIPCHK(hipMemcpy(flags, d_flags, n, hipMemcpyDeviceToHost));
  return 0;
}

int32_t vsrmc_checker_where_scan(vsrmc_checker* c, const vsrmc_where* w, vsrmc_where_info* out) {
  if (!c || !w || !out) return fail(VSRMC_E_ARG, "NULL argument");
  std::memset(out, 0, sizeof(*out));
  out->level = c->level;
  for (int k = 0; k < WHERE_MAX_EXPORTS; k++) out->min_fp[k] = out->min_index[k] = ~(u64)0;
  if (w->prog.step) return fail(VSRMC_E_ARG, "state predicates: a step program (vsrmc_step_compile) runs over pairs: vsrmc_checker_step_scan");
  if (!where_fits(w, c->model.M, c->model.symmetry)) return fail(VSRMC_E_ARG, "state predicates: compiled for another model");
  if (c->opt.world > 1) return fail(VSRMC_E_STATE, "where scan: sharded checkers are not scanned");
  if (c->deep || c->deep_regen_done || c->full_recoverable)
    return fail(VSRMC_E_STATE, "where scan: the deepest complete level exists in the seen-set only (vsrmc_checker_deepen): it has no records to scan; it is not examined");
  if (c->failed) return fail(VSRMC_E_STATE, "where scan: the search has stopped with an error");
  c->where_fps.clear();
  c->where_bits.clear();
  c->where_total = 0;
  c->where_level = c->level;
  if (c->n_frontier == 0) return 0;
  HIPCHK(hipSetDevice(c->opt.device));
  const Model& M = c->model.M;
  u64 cap = std::min<u64>(c->n_frontier, (u64)1 << 20);          // list entries kept (24 B each); the counters and minima do not come from the list
  // TEST KNOB (documented in include/vsrmc.h): a smaller list, so that a test can reach the overflow path on a small space
  if (const char* e = std::getenv("VSRMC_WHERE_LIST_CAP")) cap = std::min<u64>(cap, std::max<u64>(1, std::strtoull(e, nullptr, 10)));
  DevMem mem;
  u64* d_list = nullptr;
  WhereCtl* d_ctl = nullptr;
  u32* d_prog = nullptr;
  HIPCHK(mem.alloc(&d_list, cap * 24));
  HIPCHK(mem.alloc(&d_ctl, sizeof(WhereCtl)));
  HIPCHK(mem.alloc(&d_prog, WHERE_MAX_OPS * sizeof(u32)));
  int rc = launch_where(M, w, c->num_cus, c->stream, d_prog, c->words[c->cur], c->off[c->cur], c->lvl_fp, c->n_frontier, nullptr, d_ctl, d_list, cap, c->ev[0], c->ev[1]);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
  WhereCtl h;
  HIPCHK(hipMemcpy(&h, d_ctl, sizeof(h), hipMemcpyDeviceToHost));
  if (h.scanned != c->n_valid) return fail(VSRMC_E_HIP, "k_where: scanned " + std::to_string(h.scanned) + " records of " + std::to_string(c->n_valid));
  out->n_states = h.scanned;
  out->kernel_ms = (double)ms;
  for (int k = 0; k < WHERE_MAX_EXPORTS; k++) { out->count[k] = h.count[k]; out->min_fp[k] = h.min_fp[k]; }
  const u64 kept = std::min<u64>(h.n_list, cap);
  std::vector<u64> raw(kept * 3);
  if (kept) HIPCHK(hipMemcpy(raw.data(), d_list, kept * 24, hipMemcpyDeviceToHost));
  const std::vector<u64> order = sorted_order(kept, [&](u64 a, u64 b) { return raw[3 * a] < raw[3 * b]; });
  c->where_fps.resize(kept);
  c->where_bits.resize(kept);
  for (u64 k = 0; k < kept; k++) {
    const u64 fp = raw[3 * order[k]];
    c->where_fps[k] = fp;
    c->where_bits[k] = (uint8_t)raw[3 * order[k] + 2];
    for (int p = 0; p < WHERE_MAX_EXPORTS; p++)
      if (fp == h.min_fp[p]) out->min_index[p] = raw[3 * order[k] + 1];
  }
  c->where_total = h.n_list;
  // a list that overflowed may not hold the minima: their indices come from the level's fingerprint array then
  for (int p = 0; p < WHERE_MAX_EXPORTS; p++)
    if (h.count[p] && out->min_index[p] == ~(u64)0 && (rc = find_fp_newest(c, h.min_fp[p], &out->min_index[p]))) return rc;
  return 0;
}

int32_t vsrmc_checker_where_states(vsrmc_checker* c, uint64_t* fps, uint8_t* bits, uint64_t cap, uint64_t* n) {
  if (!c || !n) return fail(VSRMC_E_ARG, "NULL argument");
  *n = 0;
  if (c->where_level < 0) return fail(VSRMC_E_STATE, "no where scan yet (vsrmc_checker_where_scan)");
  *n = c->where_total;
  const u64 kept = c->where_fps.size();
  if (fps) {
    if (cap < kept) return fail(VSRMC_E_ARG, "buffer too small");
    std::copy(c->where_fps.begin(), c->where_fps.end(), fps);
    if (bits) std::copy(c->where_bits.begin(), c->where_bits.end(), bits);
  }
  if (c->where_total > kept)
    return fail(VSRMC_E_REP, "where states: level " + std::to_string(c->where_level) + " has " + std::to_string(c->where_total) + ", the list holds the " +
                                 std::to_string(kept) + " that arrived first (counters and minima of the scan are exact)");
  return 0;
}

}  // extern "C"
