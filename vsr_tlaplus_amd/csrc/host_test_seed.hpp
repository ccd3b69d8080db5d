// host_test_seed.hpp — TEST HOOK, compiled only with -DVSRMC_TEST_HOOKS (vsr_tlaplus_amd/libvsrmc_hooks.so; the product library does not export it):
// start a search from a caller's set of records instead of Init (included by vsrmc.hip after host_checkpoint.hpp).
//
// Why: the actions deep in the view-change and state-transfer protocol are out of reach of a BFS from Init at four and five replicas (10^8 - 10^10
// states before the first ReceiveSV), so no level total ever exercised k_expand's R = 4 / R = 5 instantiations on them.  tests/deep_harvest.py
// steers the CPU oracle to such states; this entry point makes them level 1 of a checker — checker_seed and k_seed generalised from one record
// to n — and the test then runs the ordinary vsrmc_checker_step / _probe / _deepen / _terminal_scan / _select over that level.  Nothing of k_expand
// changes: the hook only prepares the level it then runs on.
#pragma once
#ifdef VSRMC_TEST_HOOKS

namespace {
void constraint_forget_init(vsrmc_checker* c);                  // (host_constrain.hpp)
// one claim per record at level 1 (k_seed for many records): the records are in device layout with their view hashes filled in
__global__ void k_seed_many(Model M, const u64* words, const u64* refs, u64 n, Slot* table, u64 tmask, u64* lvl_fp, u32* err) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64* rec = words + (refs[i] >> 8);
  u64 fp;
  u32 ak;
  canonical_fp(M, rec[0], rec + M.h0, &fp, &ak);
  bool found_old = false, full = false;
  u32 np = 0;
  table_claim(table, tmask, fp, meta_make(1, ak, 0), 1, &found_old, CntReg{&np}, &full);
  if (full) atomicExch(err, (u32)ERR_TABLE_FULL);
  else if (found_old) atomicExch(err, (u32)ERR_INTERNAL);       // a second record of the same fingerprint: the host refuses those before the launch
  lvl_fp[i] = fp;
}
}  // namespace

extern "C" {

// Make the n wire records words[off[i] .. off[i + 1]) level 1 of the search: empty seen-set, one claim per record (level 1, its canonical auxkey, no
// parent), refs, level fingerprints, frontier counters.  Refuses, without launching anything, a record whose length is not the layout's
// (VSRMC_E_ARG) or whose bag is larger than the layout allows (VSRMC_E_REP), two records of one fingerprint (VSRMC_E_ARG) and more records or words
// than the checker's buffers hold (VSRMC_E_ARG).  vsrmc_checker_reset goes back to Init.
// A state constraint and an action constraint stay attached (attach first, then seed: both attach calls put Init back) and their results start over.  The
// seeds are level 1 AS GIVEN, subject to neither constraint: no seed is pruned, and what checker_seed's filter made of Init is forgotten with Init.
int32_t vsrmc_test_checker_seed_records(vsrmc_checker* c, const uint64_t* words, const uint64_t* off, uint64_t n) {
  if (!c || !words || !off || n == 0) return fail(VSRMC_E_ARG, "NULL argument / no record");
  if (c->opt.world != 1) return fail(VSRMC_E_STATE, "seeding is for unsharded checkers");
  const Model& M = c->model.M;
  if (n > c->opt.frontier_states) return fail(VSRMC_E_ARG, "more records than the index arrays hold (frontier_states)");
  if (n > (c->tmask + 1) / 2) return fail(VSRMC_E_ARG, "more records than half the seen-set's slots");
  u64 total = 0, max_bag = 0;
  for (u64 i = 0; i < n; i++) {
    if (off[i + 1] <= off[i] || off[i + 1] - off[i] < (u64)M.h0) return fail(VSRMC_E_ARG, "record " + std::to_string(i) + ": shorter than the fixed part of the layout");
    const u64 nmsg = (u64)hdr_nmsg(words[off[i]]);
    if (nmsg > (u64)M.max_bag) return fail(VSRMC_E_REP, "record " + std::to_string(i) + ": bag larger than the layout allows (max_bag)");
    if (off[i + 1] - off[i] != (u64)M.h0 + nmsg) return fail(VSRMC_E_ARG, "record " + std::to_string(i) + ": length differs from fixed words + bag entries of its header");
    total += (u64)M.fixed + nmsg;
    max_bag = std::max(max_bag, nmsg);
  }
  if (total > c->words_cap(0) || (total << 8) >> 8 != total) return fail(VSRMC_E_ARG, "more record words than the record buffer holds (frontier_words)");
  std::vector<u64> dev(total), refs(n), fps(n);
  u64 pos = 0;
  for (u64 i = 0; i < n; i++) {
    const int len = wire_to_device(M, words + off[i], &dev[pos]);
    u64 H[6];
    hash_full_host(M, (const u64*)&dev[pos], H);
    for (int k = 0; k < M.np; k++) dev[pos + M.h0 + k] = H[k];
    u32 ak = 0;
    canonical_fp(M, dev[pos], &dev[pos + M.h0], &fps[i], &ak);
    refs[i] = (pos << 8) | (u64)len;
    pos += (u64)len;
  }
  {
    std::vector<u64> sorted_fps(fps);
    std::sort(sorted_fps.begin(), sorted_fps.end());
    if (std::adjacent_find(sorted_fps.begin(), sorted_fps.end()) != sorted_fps.end()) return fail(VSRMC_E_ARG, "two records of one fingerprint");
  }
  int rc = checker_seed(c);                                      // every counter and mode of a fresh search; Init is taken out again below
  if (rc) return rc;
  u32* d_err = nullptr;
  HIPCHK(hipMalloc((void**)&d_err, 4));
  struct FreeErr { u32* p; ~FreeErr() { (void)hipFree(p); } } free_err{d_err};
  HIPCHK(hipMemsetAsync(d_err, 0, 4, c->stream));
  hipLaunchKernelGGL(k_table_init, dim3(4096), dim3(256), 0, c->stream, c->table, c->tmask + 1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(c->ctl, 0, sizeof(LevelCtl), c->stream));
  HIPCHK(hipMemcpyAsync(c->words[0], dev.data(), total * 8, hipMemcpyDefault, c->stream));
  HIPCHK(hipMemcpyAsync(c->off[0], refs.data(), n * 8, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_seed_many, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, M, (const u64*)c->words[0], (const u64*)c->off[0], n, c->table, c->tmask,
                     c->lvl_fp, d_err);
  HIPCHK(hipGetLastError());
  u32 err = 0;
  HIPCHK(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (err) {
    c->failed = 1;
    return fail(VSRMC_E_REP, "seeding failed on the device (error " + std::to_string(err) + ")");
  }
  c->cur = 0;
  c->level = 1;
  c->n_frontier = c->n_valid = n;
  c->cur_w = c->cur_rec_w = total;
  c->distinct = n;
  c->total_generated = 0;
  c->cur_max_bag = max_bag;
  c->bag_known = true;
  constraint_forget_init(c);                                     // (Init's level-1 figures, table_pruned and hist_new of a pruned or kept Init: not this level's)
  // traces of a seeded search start at a seed, not at Init (host_checkpoint.hpp: replay_path): the records are kept, addressed by fingerprint
  c->test_seed_index.resize(n);
  for (u64 i = 0; i < n; i++) c->test_seed_index[i] = {fps[i], i};
  std::sort(c->test_seed_index.begin(), c->test_seed_index.end());
  c->test_seed_words.assign(words, words + off[n]);
  c->test_seed_off.assign(off, off + n + 1);
  return 0;
}

// How often a list of overflowed tiles was launched again (redo_overflowed_tiles) and the other k_expand launches beyond a pass's first one: the
// checker's running counter.  A stored step adds to it and never resets it: a test reads it before and after the step.
int32_t vsrmc_test_checker_extra_launches(vsrmc_checker* c, uint64_t* out) {
  if (!c || !out) return fail(VSRMC_E_ARG, "null argument");
  *out = c->extra_launches;
  return 0;
}

}  // extern "C"
#endif
