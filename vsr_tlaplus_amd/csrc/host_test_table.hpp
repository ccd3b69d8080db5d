// host_test_table.hpp — TEST HOOKS, compiled only with -DVSRMC_TEST_HOOKS (vsr_tlaplus_amd/libvsrmc_hooks.so; the product library does not export them):
// the seen-set kernels, the winner set and k_partition driven one launch at a time with a caller's keys (included by vsrmc.hip after host_test_seed.hpp).
//
// Why: a search only ever hands the seen-set uniform fingerprints at a load below 0.85, so probe runs that start at slots 0..3 of a line, that cross the
// end of the table or are hundreds of slots long, several candidates of one fingerprint in one launch, and the kernels behind growth, checkpoints, descents
// and trace walks are met by luck and reported as "a count differs at level 17".  tests/seen_set_model.py restates what the table must hold;
// tests/seen_set_worker.py builds keys that hit those edges and compares the raw slots with it.  The table hooks work on the seen-set of an ordinary
// vsrmc_checker and launch the PRODUCT kernels and host routines unchanged (k_claim_batch + k_verdict, k_claim_batch_fused, table_grow, table_lookup,
// walk_trace, k_table_export / _import window by window as vsrmc_checker_save / _load do); the winner-set hooks work on a stand-alone set.  Two kernels are
// hook-only, because the device functions they call have no kernel of their own in the product: k_test_wset_take (wset_take, called inside k_expand) and
// k_test_probe_lookup (probe_lookup, called inside k_expand and k_probe_resolve) — one lane per entry, like k_seed_many.
#pragma once
#ifdef VSRMC_TEST_HOOKS

namespace {
__global__ void k_test_wset_take(const WSet* w, const u64* __restrict__ fps, u64 n, int level, u32 epoch, uint8_t* out) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = wset_take(w, fps[i], level, epoch) ? 1 : 0;
}
__global__ void k_test_probe_lookup(const Slot* table, u64 tmask, const u64* __restrict__ fps, u64 n, uint8_t* found, u64* metas) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u64 m = META_EMPTY;
  u32 np = 0;
  found[i] = probe_lookup(table, tmask, fps[i], &m, CntReg{&np}) ? 1 : 0;
  metas[i] = m;
}

// device buffers of one hook call: freed on every way out
struct TestBufs {
  std::vector<void*> p;
  ~TestBufs() { for (void* q : p) (void)hipFree(q); }
  template <typename T>
  hipError_t get(T** out, size_t bytes) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes ? bytes : 8);
    if (e == hipSuccess) p.push_back(q);
    *out = (T*)q;
    return e;
  }
};
unsigned test_grid(u64 n) { return (unsigned)((n + 255) / 256); }
}  // namespace

// the stand-alone winner set of the vsrmc_test_wset_* hooks: the three words the kernels are handed, a control block for k_apply_verdict / k_count_verdict
struct vsrmc_test_wset {
  int device = 0;
  hipStream_t stream = nullptr;
  WSet h = {nullptr, nullptr, 0};
  WSet* d = nullptr;
  LevelCtl* ctl = nullptr;
};

namespace {
void test_wset_free(WSet* h, WSet** d) {
  if (h->fp) (void)hipFree(h->fp);
  if (h->epoch) (void)hipFree(h->epoch);
  if (*d) (void)hipFree(*d);
  h->fp = nullptr; h->epoch = nullptr; h->mask = 0; *d = nullptr;
}
int test_wset_alloc(hipStream_t stream, int log2, WSet* h, WSet** d) {
  const u64 slots = (u64)1 << log2;
  h->fp = nullptr; h->epoch = nullptr; h->mask = slots - 1; *d = nullptr;
  hipError_t e = hipMalloc((void**)&h->fp, slots * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&h->epoch, slots * 4);
  if (e == hipSuccess) e = hipMalloc((void**)d, sizeof(WSet));
  if (e == hipSuccess) e = hipMemsetAsync(h->fp, 0, slots * 8, stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->epoch, 0, slots * 4, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(*d, h, sizeof(WSet), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) {
    test_wset_free(h, d);
    return fail(VSRMC_E_HIP, std::string("winner set: ") + hipGetErrorString(e));
  }
  return 0;
}
}  // namespace

extern "C" {

// ---- the seen-set of a checker -----------------------------------------------------------------------------------------------------------------------
// k_table_init: an empty table (Init, which vsrmc_checker_create seeded, is gone too)
int32_t vsrmc_test_table_clear(vsrmc_checker* c) {
  if (!c) return fail(VSRMC_E_ARG, "NULL argument");
  HIPCHK(hipSetDevice(c->opt.device));
  hipLaunchKernelGGL(k_table_init, dim3(4096), dim3(256), 0, c->stream, c->table, c->tmask + 1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// One launch of the owner's side of a sharded level over n (fingerprint, key) pairs: scheme 0 = k_claim_batch, then k_verdict; scheme 1 = k_claim_batch_fused.
// verdict[n] = the verdict bytes; ctl_out[3] = err, ties, probes of the control block (an ERR_TABLE_FULL is reported there, not as a failure of the call).
int32_t vsrmc_test_table_claim(vsrmc_checker* c, const uint64_t* entries, uint64_t n, int32_t level, int32_t scheme, uint8_t* verdict, uint64_t* ctl_out) {
  if (!c || !entries || !verdict || !ctl_out || n == 0) return fail(VSRMC_E_ARG, "NULL argument / empty batch");
  if (level < 1 || level > 510 || (scheme != 0 && scheme != 1)) return fail(VSRMC_E_ARG, "bad level / scheme");
  if (scheme == 0)
    for (u64 i = 0; i < n; i++)
      if (entries[2 * i] == 0) return fail(VSRMC_E_ARG, "fingerprint 0 in a batch of the two-kernel scheme (only the single-pass scheme pads its chunks)");
  HIPCHK(hipSetDevice(c->opt.device));
  TestBufs b;
  u64 *d_ent = nullptr, *d_rslot = nullptr;
  uint8_t* d_ver = nullptr;
  HIPCHK(b.get(&d_ent, 16 * n));
  HIPCHK(b.get(&d_rslot, 8 * n));
  HIPCHK(b.get(&d_ver, n));
  HIPCHK(hipMemcpyAsync(d_ent, entries, 16 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(d_ver, 0xEE, n, c->stream));           // every byte must be written by the kernels
  HIPCHK(hipMemsetAsync(c->ctl, 0, sizeof(LevelCtl), c->stream));
  if (scheme == 0) {
    hipLaunchKernelGGL(k_claim_batch, dim3(test_grid(n)), dim3(256), 0, c->stream, c->table, c->tmask, (const u64*)d_ent, (u64)n, (int)level, d_rslot, c->ctl);
    hipLaunchKernelGGL(k_verdict, dim3(test_grid(n)), dim3(256), 0, c->stream, c->table, (const u64*)d_ent, (const u64*)d_rslot, (u64)n, d_ver);
  } else {
    hipLaunchKernelGGL(k_claim_batch_fused, dim3(test_grid(n)), dim3(256), 0, c->stream, c->table, c->tmask, (const u64*)d_ent, (u64)n, (int)level, d_ver, c->ctl);
  }
  HIPCHK(hipGetLastError());
  LevelCtl h;
  HIPCHK(hipMemcpyAsync(&h, c->ctl, sizeof(LevelCtl), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(verdict, d_ver, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  ctl_out[0] = h.err; ctl_out[1] = h.ties; ctl_out[2] = h.probes;
  return 0;
}

// the raw slot array: slots[2 * i] = fingerprint, slots[2 * i + 1] = meta word of slot i; *n_slots = slots of the table
int32_t vsrmc_test_table_dump(vsrmc_checker* c, uint64_t* slots, uint64_t cap_slots, uint64_t* n_slots) {
  if (!c || !n_slots) return fail(VSRMC_E_ARG, "NULL argument");
  *n_slots = c->tmask + 1;
  if (!slots) return 0;
  if (cap_slots < c->tmask + 1) return fail(VSRMC_E_ARG, "buffer too small");
  HIPCHK(hipSetDevice(c->opt.device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(slots, c->table, (c->tmask + 1) * sizeof(Slot), hipMemcpyDeviceToHost));
  return 0;
}

// table_grow (host_search.hpp): the table re-hashed into twice the slots
int32_t vsrmc_test_table_grow(vsrmc_checker* c) {
  if (!c) return fail(VSRMC_E_ARG, "NULL argument");
  const int g = table_grow(c);
  if (g == 1) return fail(VSRMC_E_STATE, "the seen-set cannot grow");
  return g;
}

int32_t vsrmc_test_table_untake(vsrmc_checker* c, int32_t min_level) {
  if (!c) return fail(VSRMC_E_ARG, "NULL argument");
  HIPCHK(hipSetDevice(c->opt.device));
  hipLaunchKernelGGL(k_table_untake, dim3(4096), dim3(256), 0, c->stream, c->table, c->tmask + 1, (int)min_level);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// out[3] = xor, sum, count of the fingerprints of one level, read from the table
int32_t vsrmc_test_table_level_checksum(vsrmc_checker* c, int32_t level, uint64_t* out) {
  if (!c || !out) return fail(VSRMC_E_ARG, "NULL argument");
  HIPCHK(hipSetDevice(c->opt.device));
  TestBufs b;
  u64* d = nullptr;
  HIPCHK(b.get(&d, 24));
  HIPCHK(hipMemsetAsync(d, 0, 24, c->stream));
  hipLaunchKernelGGL(k_table_level_checksum, dim3(4096), dim3(256), 0, c->stream, (const Slot*)c->table, c->tmask + 1, (int)level, d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, d, 24, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// table_lookup (host_checker.hpp, k_table_lookup): *found = matching states
int32_t vsrmc_test_table_lookup(vsrmc_checker* c, uint64_t key, int32_t level, int32_t by_low_bits, int32_t* found, uint64_t* fp, uint64_t* meta) {
  if (!c || !found || !fp || !meta) return fail(VSRMC_E_ARG, "NULL argument");
  HIPCHK(hipSetDevice(c->opt.device));
  int f = 0;
  u64 a = 0, m = 0;
  const int rc = table_lookup(c, key, level, by_low_bits, &f, &a, &m);
  *found = f; *fp = a; *meta = m;
  return rc;
}

// k_trace_walk, raw: raw[0 .. level) = the fingerprints it wrote, raw[level] = its status word; then walk_trace (host_checker.hpp) over the same table:
// *walk_rc = what it returns, fps[0 .. level) = the path it hands its callers when that is 0
int32_t vsrmc_test_table_walk(vsrmc_checker* c, uint64_t fp, int32_t level, uint64_t* raw, uint64_t* fps, int32_t* walk_rc) {
  if (!c || !raw || !fps || !walk_rc || level < 1 || level > 510) return fail(VSRMC_E_ARG, "NULL argument / no such level");
  HIPCHK(hipSetDevice(c->opt.device));
  TestBufs b;
  u64* d = nullptr;
  HIPCHK(b.get(&d, ((u64)level + 1) * 8));
  HIPCHK(hipMemsetAsync(d, 0, ((u64)level + 1) * 8, c->stream));
  hipLaunchKernelGGL(k_trace_walk, dim3(1), dim3(64), 0, c->stream, (const Slot*)c->table, c->tmask, (u64)fp, (int)level, d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(raw, d, ((u64)level + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  std::vector<u64> path;
  *walk_rc = walk_trace(c, fp, level, &path);
  for (int i = 0; i < level; i++) fps[i] = (*walk_rc == 0 && (size_t)i < path.size()) ? path[(size_t)i] : 0;
  return 0;
}

// probe_lookup, one lane per fingerprint: found[i], metas[i] (META_EMPTY where absent)
int32_t vsrmc_test_table_probe_lookup(vsrmc_checker* c, const uint64_t* fps, uint64_t n, uint8_t* found, uint64_t* metas) {
  if (!c || !fps || !found || !metas || n == 0) return fail(VSRMC_E_ARG, "NULL argument / empty batch");
  HIPCHK(hipSetDevice(c->opt.device));
  TestBufs b;
  u64 *d_fps = nullptr, *d_m = nullptr;
  uint8_t* d_f = nullptr;
  HIPCHK(b.get(&d_fps, 8 * n));
  HIPCHK(b.get(&d_m, 8 * n));
  HIPCHK(b.get(&d_f, n));
  HIPCHK(hipMemcpyAsync(d_fps, fps, 8 * n, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_test_probe_lookup, dim3(test_grid(n)), dim3(256), 0, c->stream, (const Slot*)c->table, c->tmask, (const u64*)d_fps, (u64)n, d_f, d_m);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(found, d_f, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(metas, d_m, 8 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// The seen-set through a checkpoint's two kernels: k_table_export over windows of `window` slots, as vsrmc_checker_save walks the table, the occupied slots
// collected on the host; then k_table_import into a fresh table of 2^new_log2 slots in pieces of `window` entries, as vsrmc_checker_load reads them back.
// The fresh table replaces the checker's.  *n_exported = the sum of the export counters.
int32_t vsrmc_test_table_export_import(vsrmc_checker* c, uint64_t window, int32_t new_log2, uint64_t* n_exported) {
  if (!c || !n_exported || window == 0) return fail(VSRMC_E_ARG, "NULL argument / empty window");
  if (new_log2 < 8 || new_log2 > 24) return fail(VSRMC_E_ARG, "new table: 2^8 .. 2^24 slots");
  HIPCHK(hipSetDevice(c->opt.device));
  const u64 slots = c->tmask + 1, win = std::min<u64>(slots, window);
  TestBufs b;
  Slot* d_out = nullptr;
  u64* d_cnt = nullptr;
  u32* d_err = nullptr;
  HIPCHK(b.get(&d_out, win * sizeof(Slot)));
  HIPCHK(b.get(&d_cnt, 8));
  HIPCHK(b.get(&d_err, 4));
  std::vector<Slot> held;
  for (u64 first = 0; first < slots; first += win) {
    const u64 n = std::min<u64>(win, slots - first);            // (the table's sizes are powers of two, a caller's window need not be)
    u64 cnt = 0;
    HIPCHK(hipMemsetAsync(d_cnt, 0, 8, c->stream));
    hipLaunchKernelGGL(k_table_export, dim3(test_grid(n)), dim3(256), 0, c->stream, (const Slot*)c->table, first, n, d_out, win, d_cnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (cnt > n) return fail(VSRMC_E_STATE, "k_table_export counted more slots than its window has");
    const size_t at = held.size();
    held.resize(at + (size_t)cnt);
    if (cnt) HIPCHK(hipMemcpy(held.data() + at, d_out, cnt * sizeof(Slot), hipMemcpyDeviceToHost));
  }
  *n_exported = (u64)held.size();
  const u64 new_slots = (u64)1 << new_log2;
  if (held.size() > new_slots) return fail(VSRMC_E_ARG, "more entries than the new table has slots");
  Slot* nt = nullptr;
  HIPCHK(hipMalloc((void**)&nt, new_slots * sizeof(Slot)));
  struct FreeTable { Slot* p; ~FreeTable() { if (p) (void)hipFree(p); } } guard{nt};
  hipLaunchKernelGGL(k_table_init, dim3(4096), dim3(256), 0, c->stream, nt, new_slots);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(d_err, 0, 4, c->stream));
  for (u64 done = 0; done < (u64)held.size(); done += win) {
    const u64 k = std::min<u64>(win, (u64)held.size() - done);
    HIPCHK(hipMemcpyAsync(d_out, held.data() + done, k * sizeof(Slot), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_table_import, dim3(test_grid(k)), dim3(256), 0, c->stream, nt, new_slots - 1, (const Slot*)d_out, k, d_err);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  u32 terr = 0;
  HIPCHK(hipMemcpy(&terr, d_err, 4, hipMemcpyDeviceToHost));
  if (terr) return fail(VSRMC_E_REP, "k_table_import raised error " + std::to_string(terr));
  guard.p = c->table;                                           // the old table is the one to free now
  c->table = nt;
  c->tmask = new_slots - 1;
  c->opt.table_log2 = new_log2;
  return 0;
}

// ---- k_partition over a caller's refs and fingerprints (both rewritten in place) ------------------------------------------------------------------------
int32_t vsrmc_test_table_partition(int32_t device, uint64_t* off, uint64_t* lvl_fp, uint64_t n, int32_t rank, int32_t world, uint64_t* n_kept) {
  if (!off || !lvl_fp || !n_kept || n == 0) return fail(VSRMC_E_ARG, "NULL argument / nothing to partition");
  if (world < 1 || world > 8 || rank < 0 || rank >= world) return fail(VSRMC_E_ARG, "bad rank / world");
  int rc = check_device(device);
  if (rc) return rc;
  TestBufs b;
  u64 *d_off = nullptr, *d_fp = nullptr, *d_cnt = nullptr;
  HIPCHK(b.get(&d_off, 8 * n));
  HIPCHK(b.get(&d_fp, 8 * n));
  HIPCHK(b.get(&d_cnt, 8));
  HIPCHK(hipMemcpy(d_off, off, 8 * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_fp, lvl_fp, 8 * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(d_cnt, 0, 8));
  hipLaunchKernelGGL(k_partition, dim3(test_grid(n)), dim3(256), 0, 0, d_off, d_fp, (u64)n, (int)rank, (int)world, d_cnt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(off, d_off, 8 * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(lvl_fp, d_fp, 8 * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(n_kept, d_cnt, 8, hipMemcpyDeviceToHost));
  return 0;
}

// ---- a stand-alone winner set --------------------------------------------------------------------------------------------------------------------------
int32_t vsrmc_test_wset_create(int32_t device, int32_t log2_slots, vsrmc_test_wset** out) {
  if (!out || log2_slots < 4 || log2_slots > 24) return fail(VSRMC_E_ARG, "NULL argument / 2^4 .. 2^24 slots");
  int rc = check_device(device);
  if (rc) return rc;
  vsrmc_test_wset* w = new vsrmc_test_wset();
  w->device = device;
  hipError_t e = hipStreamCreate(&w->stream);
  if (e == hipSuccess) e = hipMalloc((void**)&w->ctl, sizeof(LevelCtl));
  if (e != hipSuccess) {
    if (w->stream) (void)hipStreamDestroy(w->stream);
    delete w;
    return fail(VSRMC_E_HIP, std::string("winner set: ") + hipGetErrorString(e));
  }
  rc = test_wset_alloc(w->stream, log2_slots, &w->h, &w->d);
  if (rc) {
    (void)hipFree(w->ctl);
    (void)hipStreamDestroy(w->stream);
    delete w;
    return rc;
  }
  *out = w;
  return 0;
}

void vsrmc_test_wset_destroy(vsrmc_test_wset* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  (void)hipStreamSynchronize(w->stream);
  test_wset_free(&w->h, &w->d);
  if (w->ctl) (void)hipFree(w->ctl);
  (void)hipStreamDestroy(w->stream);
  delete w;
}

// fp[i], epoch[i] = the two words of slot i
int32_t vsrmc_test_wset_dump(vsrmc_test_wset* w, uint64_t* fp, uint32_t* epoch, uint64_t cap_slots, uint64_t* n_slots) {
  if (!w || !n_slots) return fail(VSRMC_E_ARG, "NULL argument");
  *n_slots = w->h.mask + 1;
  if (!fp || !epoch) return 0;
  if (cap_slots < w->h.mask + 1) return fail(VSRMC_E_ARG, "buffer too small");
  HIPCHK(hipSetDevice(w->device));
  HIPCHK(hipStreamSynchronize(w->stream));
  HIPCHK(hipMemcpy(fp, w->h.fp, (w->h.mask + 1) * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(epoch, w->h.epoch, (w->h.mask + 1) * 4, hipMemcpyDeviceToHost));
  return 0;
}

// k_wset_rehash into twice the slots, as wset_grow (host_checker.hpp) launches it
int32_t vsrmc_test_wset_grow(vsrmc_test_wset* w) {
  if (!w) return fail(VSRMC_E_ARG, "NULL argument");
  if (w->h.mask + 1 >= ((u64)1 << 24)) return fail(VSRMC_E_ARG, "2^24 slots at the most");
  HIPCHK(hipSetDevice(w->device));
  const u64 old_slots = w->h.mask + 1;
  int log2 = 0;
  while (((u64)1 << log2) < old_slots * 2) log2++;
  WSet nh;
  WSet* nd = nullptr;
  int rc = test_wset_alloc(w->stream, log2, &nh, &nd);
  if (rc) return rc;
  TestBufs b;
  u32* d_err = nullptr;
  hipError_t e = b.get(&d_err, 4);
  if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, 4, w->stream);
  u32 err = 0;
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_wset_rehash, dim3(4096), dim3(256), 0, w->stream, (const u64*)w->h.fp, (const u32*)w->h.epoch, old_slots, nh.fp, nh.epoch, nh.mask, d_err);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, w->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(w->stream);
  if (e != hipSuccess || err) {
    test_wset_free(&nh, &nd);
    return e != hipSuccess ? fail(VSRMC_E_HIP, std::string("k_wset_rehash: ") + hipGetErrorString(e)) : fail(VSRMC_E_REP, "k_wset_rehash raised error " + std::to_string(err));
  }
  test_wset_free(&w->h, &w->d);
  w->h = nh;
  w->d = nd;
  return 0;
}

// k_wset_export over windows of `window` slots (vsrmc_checker_save), then k_wset_import into a fresh set of 2^new_log2 slots (vsrmc_checker_load), which
// replaces this one.  *n_exported = the sum of the export counters.
int32_t vsrmc_test_wset_export_import(vsrmc_test_wset* w, uint64_t window, int32_t new_log2, uint64_t* n_exported) {
  if (!w || !n_exported || window == 0) return fail(VSRMC_E_ARG, "NULL argument / empty window");
  if (new_log2 < 4 || new_log2 > 24) return fail(VSRMC_E_ARG, "new set: 2^4 .. 2^24 slots");
  HIPCHK(hipSetDevice(w->device));
  const u64 slots = w->h.mask + 1, win = std::min<u64>(slots, window);
  TestBufs b;
  Slot* d_out = nullptr;
  u64* d_cnt = nullptr;
  u32* d_err = nullptr;
  HIPCHK(b.get(&d_out, win * sizeof(Slot)));
  HIPCHK(b.get(&d_cnt, 8));
  HIPCHK(b.get(&d_err, 4));
  std::vector<Slot> held;
  for (u64 first = 0; first < slots; first += win) {
    const u64 n = std::min<u64>(win, slots - first);
    u64 cnt = 0;
    HIPCHK(hipMemsetAsync(d_cnt, 0, 8, w->stream));
    hipLaunchKernelGGL(k_wset_export, dim3(test_grid(n)), dim3(256), 0, w->stream, (const u64*)w->h.fp, (const u32*)w->h.epoch, first, n, d_out, win, d_cnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    if (cnt > n) return fail(VSRMC_E_STATE, "k_wset_export counted more slots than its window has");
    const size_t at = held.size();
    held.resize(at + (size_t)cnt);
    if (cnt) HIPCHK(hipMemcpy(held.data() + at, d_out, cnt * sizeof(Slot), hipMemcpyDeviceToHost));
  }
  *n_exported = (u64)held.size();
  if (held.size() > ((u64)1 << new_log2)) return fail(VSRMC_E_ARG, "more entries than the new set has slots");
  WSet nh;
  WSet* nd = nullptr;
  int rc = test_wset_alloc(w->stream, new_log2, &nh, &nd);
  if (rc) return rc;
  hipError_t e = hipMemsetAsync(d_err, 0, 4, w->stream);
  for (u64 done = 0; done < (u64)held.size() && e == hipSuccess; done += win) {
    const u64 k = std::min<u64>(win, (u64)held.size() - done);
    e = hipMemcpyAsync(d_out, held.data() + done, k * sizeof(Slot), hipMemcpyHostToDevice, w->stream);
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(k_wset_import, dim3(test_grid(k)), dim3(256), 0, w->stream, (const WSet*)nd, (const Slot*)d_out, k, d_err);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(w->stream);
  }
  u32 terr = 0;
  if (e == hipSuccess) e = hipMemcpy(&terr, d_err, 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess || terr) {
    test_wset_free(&nh, &nd);
    return e != hipSuccess ? fail(VSRMC_E_HIP, std::string("k_wset_import: ") + hipGetErrorString(e)) : fail(VSRMC_E_REP, "k_wset_import raised error " + std::to_string(terr));
  }
  test_wset_free(&w->h, &w->d);
  w->h = nh;
  w->d = nd;
  return 0;
}

// The generator's side of a sharded level over n candidates with a caller's verdict bytes: mode 0 = k_apply_verdict (cand_idx: state index | violated-invariant
// mask << 56; nx_off / lvl_fp: n_idx entries, rewritten in place — the losers' are withdrawn), mode 1 = k_count_verdict (cand_idx: bag size | mask << 56;
// pending: pending_cap (fingerprint, key) pairs).  w == NULL runs the kernels without a winner set.
// out[8] = err, viol_fp, viol_mask, n_new, fp_xor, fp_sum, max_bag, n_pending of the control block.
int32_t vsrmc_test_wset_insert(vsrmc_test_wset* w, int32_t device, int32_t mode, const uint64_t* entries, const uint64_t* cand_idx, const uint8_t* verdict, uint64_t n,
                               int32_t level, uint64_t* nx_off, uint64_t* lvl_fp, uint64_t n_idx, uint64_t* pending, uint64_t pending_cap, uint64_t* out) {
  if (!entries || !cand_idx || !verdict || !out || n == 0) return fail(VSRMC_E_ARG, "NULL argument / empty batch");
  if (level < 1 || level > 510 || (mode != 0 && mode != 1)) return fail(VSRMC_E_ARG, "bad level / mode");
  if (mode == 0) {
    if (!nx_off || !lvl_fp || n_idx == 0) return fail(VSRMC_E_ARG, "k_apply_verdict needs the index arrays");
    for (u64 i = 0; i < n; i++)                                 // the kernel writes nx_off[index] / lvl_fp[index] of every loser
      if (entries[2 * i] != 0 && cand_index(cand_idx[i]) >= n_idx) return fail(VSRMC_E_ARG, "candidate " + std::to_string(i) + ": state index beyond the index arrays");
  } else if (pending_cap && !pending) {
    return fail(VSRMC_E_ARG, "k_count_verdict needs the pending list");
  }
  const int dev = w ? w->device : device;
  int rc = check_device(dev);
  if (rc) return rc;
  hipStream_t st = w ? w->stream : (hipStream_t) nullptr;
  TestBufs b;
  u64 *d_ent = nullptr, *d_ci = nullptr, *d_off = nullptr, *d_fp = nullptr, *d_pend = nullptr;
  uint8_t* d_ver = nullptr;
  LevelCtl* ctl = w ? w->ctl : nullptr;
  HIPCHK(b.get(&d_ent, 16 * n));
  HIPCHK(b.get(&d_ci, 8 * n));
  HIPCHK(b.get(&d_ver, n));
  if (!ctl) HIPCHK(b.get(&ctl, sizeof(LevelCtl)));
  LevelCtl h;
  std::memset(&h, 0, sizeof(h));
  h.viol_fp = ~(u64)0;
  HIPCHK(hipMemcpyAsync(ctl, &h, sizeof(h), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_ent, entries, 16 * n, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_ci, cand_idx, 8 * n, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_ver, verdict, n, hipMemcpyHostToDevice, st));
  if (mode == 0) {
    HIPCHK(b.get(&d_off, 8 * n_idx));
    HIPCHK(b.get(&d_fp, 8 * n_idx));
    HIPCHK(hipMemcpyAsync(d_off, nx_off, 8 * n_idx, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_fp, lvl_fp, 8 * n_idx, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_apply_verdict, dim3(test_grid(n)), dim3(256), 0, st, (const u64*)d_ent, (const u64*)d_ci, (const uint8_t*)d_ver, (u64)n, d_off, d_fp, ctl,
                       (const WSet*)(w ? w->d : nullptr), (int)level);
  } else {
    HIPCHK(b.get(&d_pend, 16 * pending_cap));
    HIPCHK(hipMemsetAsync(d_pend, 0, pending_cap ? 16 * pending_cap : 8, st));
    hipLaunchKernelGGL(k_count_verdict, dim3(test_grid(n)), dim3(256), 0, st, (const u64*)d_ent, (const u64*)d_ci, (const uint8_t*)d_ver, (u64)n, d_pend, (u64)pending_cap, ctl,
                       (const WSet*)(w ? w->d : nullptr), (int)level);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (mode == 0) {
    HIPCHK(hipMemcpy(nx_off, d_off, 8 * n_idx, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(lvl_fp, d_fp, 8 * n_idx, hipMemcpyDeviceToHost));
  } else if (pending_cap) {
    HIPCHK(hipMemcpy(pending, d_pend, 16 * pending_cap, hipMemcpyDeviceToHost));
  }
  out[0] = h.err; out[1] = h.viol_fp; out[2] = h.viol_mask; out[3] = h.n_new; out[4] = h.fp_xor; out[5] = h.fp_sum; out[6] = h.max_bag; out[7] = h.n_pending;
  return 0;
}

// wset_take, one lane per fingerprint (k_test_wset_take): out[i] = this lane was the first of descent `epoch` to ask for a level-`level` state of the set
int32_t vsrmc_test_wset_take(vsrmc_test_wset* w, const uint64_t* fps, uint64_t n, int32_t level, uint32_t epoch, uint8_t* out) {
  if (!w || !fps || !out || n == 0) return fail(VSRMC_E_ARG, "NULL argument / empty batch");
  if (level < 1 || level > 510) return fail(VSRMC_E_ARG, "bad level");
  HIPCHK(hipSetDevice(w->device));
  TestBufs b;
  u64* d_fps = nullptr;
  uint8_t* d_out = nullptr;
  HIPCHK(b.get(&d_fps, 8 * n));
  HIPCHK(b.get(&d_out, n));
  HIPCHK(hipMemcpyAsync(d_fps, fps, 8 * n, hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipMemsetAsync(d_out, 0xEE, n, w->stream));
  hipLaunchKernelGGL(k_test_wset_take, dim3(test_grid(n)), dim3(256), 0, w->stream, (const WSet*)w->d, (const u64*)d_fps, (u64)n, (int)level, (u32)epoch, d_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, d_out, n, hipMemcpyDeviceToHost, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  return 0;
}

}  // extern "C"
#endif
