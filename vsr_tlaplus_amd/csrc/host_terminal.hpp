// host_terminal.hpp — terminal states (TLC's deadlock check with a counter-example): the host side of k_terminal (vsr_terminal.hpp) — a caller's batch,
// the scan of the checker's newest stored level, the list the last scan left (included by vsrmc.hip: one translation unit, the sections share its
// anonymous-namespace helpers).
#pragma once

namespace {

// one launch over n refs; the TermCtl at d_ctl is initialised here
int launch_terminal(const Model& M, int num_cus, hipStream_t stream, const u64* d_words, const u64* d_refs, const u64* d_fps, u64 n, uint8_t* d_flags,
                    TermCtl* d_ctl, u64* d_list, u64 list_cap) {
  TermCtl init;
  std::memset(&init, 0, sizeof(init));
  init.min_fp = init.min_fp_unsettled = ~(u64)0;
  HIPCHK(hipMemcpyAsync(d_ctl, &init, sizeof(init), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(KERNEL_OF(k_terminal, M), dim3(scan_grid(n, num_cus)), dim3(256), 0, stream, M, d_words, d_refs, d_fps, n, d_flags, d_ctl, d_list, list_cap);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int32_t vsrmc_terminal_batch(const vsrmc_model* m, int32_t device, const uint64_t* words, const uint64_t* off, uint64_t n, uint8_t* flags) {
  if (!m || !words || !off || !flags) return fail(VSRMC_E_ARG, "NULL argument");
  int rc = check_device(device);
  if (rc) return rc;
  if (n == 0) return 0;
  const Model& M = m->M;
  DevMem mem;
  u64 *d_words = nullptr, *d_refs = nullptr;
  uint8_t* d_flags = nullptr;
  TermCtl* d_ctl = nullptr;
  rc = stage_batch(M, words, off, n, longer_than_255, mem, &d_words, &d_refs);
  if (rc) return rc;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  HIPCHK(mem.alloc(&d_flags, n));
  HIPCHK(mem.alloc(&d_ctl, sizeof(TermCtl)));
  HIPCHK(hipMemset(d_flags, 0, n));
  rc = launch_terminal(M, prop.multiProcessorCount, nullptr, d_words, d_refs, nullptr, n, d_flags, d_ctl, nullptr, 0);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize());
  TermCtl h;
  HIPCHK(hipMemcpy(&h, d_ctl, sizeof(h), hipMemcpyDeviceToHost));
  if (h.scanned != n) return fail(VSRMC_E_HIP, "k_terminal: the scan did not cover the batch");
  HIPCHK(hipMemcpy(flags, d_flags, n, hipMemcpyDeviceToHost));
  return 0;
}

int32_t vsrmc_checker_terminal_scan(vsrmc_checker* c, vsrmc_terminal_info* out) {
  if (!c || !out) return fail(VSRMC_E_ARG, "NULL argument");
  std::memset(out, 0, sizeof(*out));
  out->level = c->level;
  out->min_fp = out->min_index = out->min_fp_unsettled = out->min_index_unsettled = ~(u64)0;
  if (c->opt.world > 1) return fail(VSRMC_E_STATE, "terminal scan: sharded checkers are not scanned (their terminal states stay counted: vsrmc_level_info.deadlocks)");
  if (c->deep || c->deep_regen_done || c->full_recoverable)
    return fail(VSRMC_E_STATE, "terminal scan: the deepest complete level exists in the seen-set only (vsrmc_checker_deepen): it has no records to scan; its terminal states stay counted");
  if (c->failed) return fail(VSRMC_E_STATE, "terminal scan: the search has stopped with an error");
  c->term_fps.clear();
  c->term_flags.clear();
  c->term_total = 0;
  c->term_level = c->level;
  if (c->n_frontier == 0) return 0;
  HIPCHK(hipSetDevice(c->opt.device));
  const Model& M = c->model.M;
  u64 cap = std::min<u64>(c->n_frontier, (u64)1 << 20);          // list entries kept (24 B each); the counters and minima do not come from the list
  // TEST KNOB (documented in include/vsrmc.h): a smaller list, so that a test can reach the overflow path on a small space
  if (const char* e = std::getenv("VSRMC_TERMINAL_LIST_CAP")) cap = std::min<u64>(cap, std::max<u64>(1, std::strtoull(e, nullptr, 10)));
  DevMem mem;
  u64* d_list = nullptr;
  TermCtl* d_ctl = nullptr;
  HIPCHK(mem.alloc(&d_list, cap * 24));
  HIPCHK(mem.alloc(&d_ctl, sizeof(TermCtl)));
  HIPCHK(hipEventRecord(c->ev[0], c->stream));
  int rc = launch_terminal(M, c->num_cus, c->stream, c->words[c->cur], c->off[c->cur], c->lvl_fp, c->n_frontier, nullptr, d_ctl, d_list, cap);
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev[1], c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
  TermCtl h;
  HIPCHK(hipMemcpy(&h, d_ctl, sizeof(h), hipMemcpyDeviceToHost));
  if (h.scanned != c->n_valid) return fail(VSRMC_E_HIP, "k_terminal: scanned " + std::to_string(h.scanned) + " records of " + std::to_string(c->n_valid));
  out->n_states = h.scanned;
  out->n_terminal = h.terminal;
  out->n_unsettled = h.unsettled;
  out->min_fp = h.min_fp;
  out->min_fp_unsettled = h.min_fp_unsettled;
  out->kernel_ms = (double)ms;
  const u64 kept = std::min<u64>(h.n_list, cap);
  std::vector<u64> raw(kept * 3);
  if (kept) HIPCHK(hipMemcpy(raw.data(), d_list, kept * 24, hipMemcpyDeviceToHost));
  const std::vector<u64> order = sorted_order(kept, [&](u64 a, u64 b) { return raw[3 * a] < raw[3 * b]; });
  c->term_fps.resize(kept);
  c->term_flags.resize(kept);
  for (u64 k = 0; k < kept; k++) {
    c->term_fps[k] = raw[3 * order[k]];
    c->term_flags[k] = (uint8_t)raw[3 * order[k] + 2];
    if (raw[3 * order[k]] == h.min_fp) out->min_index = raw[3 * order[k] + 1];
    if (raw[3 * order[k]] == h.min_fp_unsettled) out->min_index_unsettled = raw[3 * order[k] + 1];
  }
  c->term_total = h.n_list;
  // a list that overflowed may not hold the minima: their indices come from the level's fingerprint array then
  if (h.terminal && out->min_index == ~(u64)0 && (rc = find_fp_newest(c, h.min_fp, &out->min_index))) return rc;
  if (h.unsettled && out->min_index_unsettled == ~(u64)0 && (rc = find_fp_newest(c, h.min_fp_unsettled, &out->min_index_unsettled))) return rc;
  return 0;
}

int32_t vsrmc_checker_terminal_states(vsrmc_checker* c, uint64_t* fps, uint8_t* flags, uint64_t cap, uint64_t* n) {
  if (!c || !n) return fail(VSRMC_E_ARG, "NULL argument");
  *n = 0;
  if (c->term_level < 0) return fail(VSRMC_E_STATE, "no terminal scan yet (vsrmc_checker_terminal_scan)");
  *n = c->term_total;
  const u64 kept = c->term_fps.size();
  if (fps) {
    if (cap < kept) return fail(VSRMC_E_ARG, "buffer too small");
    std::copy(c->term_fps.begin(), c->term_fps.end(), fps);
    if (flags) std::copy(c->term_flags.begin(), c->term_flags.end(), flags);
  }
  if (c->term_total > kept)
    return fail(VSRMC_E_REP, "terminal states: level " + std::to_string(c->term_level) + " has " + std::to_string(c->term_total) + ", the list holds the " +
                                 std::to_string(kept) + " that arrived first (counters and minima of the scan are exact)");
  return 0;
}

}  // extern "C"
