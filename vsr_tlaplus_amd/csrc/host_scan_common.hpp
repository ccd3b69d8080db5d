// host_scan_common.hpp — what the host sides of the predicate scans share (host_batch / host_terminal / host_where / host_constrain / host_step /
// host_action_constrain / host_deep_where): the kernel instantiation of a model, the grid of a scan, fresh control blocks, the owner of device
// allocations, a wire batch staged as a level has its records, the body of the compile entry points (included by vsrmc.hip: one translation unit, the
// sections share its anonymous-namespace helpers).
#pragma once

// the instantiation of kernel template K for model M (the kernels have different signatures: a macro over the name)
#define KERNEL_OF(K, M) ((M).model_id == 1 ? K<1> : (M).model_id == 2 ? K<2> : K<0>)

struct vsrmc_where {
  WhereProgram prog;
  int R, C, n, L, symmetry;            // the model it was compiled for: the unfolding depends on these
  int model_id = 0;                    // and the layout the loads address (vsrmc_predicates_compile; the two older entries compile for VSR.tla only)
};

namespace {

// blocks of 256 lanes for a grid-stride scan over n items
unsigned scan_grid(u64 n, int num_cus) { return (unsigned)std::max<u64>(1, std::min<u64>((n + 255) / 256, (u64)num_cus * 8)); }

// the indices 0 .. n-1 in the order `less` gives them (a downloaded list is published sorted, its entries staying where they are)
template <class Less>
std::vector<u64> sorted_order(u64 n, Less less) {
  std::vector<u64> order(n);
  for (u64 k = 0; k < n; k++) order[k] = k;
  std::sort(order.begin(), order.end(), less);
  return order;
}

// a control block before its first launch: counters 0, minima "none" (WhereCtl and StepCtl)
template <class Ctl>
Ctl fresh_ctl() {
  Ctl h;
  std::memset(&h, 0, sizeof(h));
  for (int k = 0; k < WHERE_MAX_EXPORTS; k++) h.min_fp[k] = ~(u64)0;
  return h;
}

// Device allocations of one scope, or of one handle as its member: freed when it ends.  alloc() after a failure does nothing and returns that failure, so
// that a run of them is checked once (err) or one by one (HIPCHK).
struct DevMem {
  std::vector<void*> held;
  hipError_t err = hipSuccess;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  ~DevMem() { for (void* p : held) (void)hipFree(p); }
  template <class T>
  hipError_t alloc(T** p, size_t bytes) {
    *p = nullptr;
    if (err == hipSuccess && (err = hipMalloc((void**)p, bytes)) == hipSuccess) held.push_back(*p);
    return err;
  }
  template <class T>
  hipError_t upload(T** p, const T* src, size_t count, size_t room = 0) {   // alloc of max(count, room) elements + copy of count
    if (alloc(p, std::max(count, room) * sizeof(T)) == hipSuccess && count) err = hipMemcpy(*p, src, count * sizeof(T), hipMemcpyHostToDevice);
    return err;
  }
};

// n wire records as device-layout records (the H words stay 0: guards and predicates never read them) behind a ref array, as a level has them, on the
// device.  too_long is the caller's own refusal of a record (longer_than_255 / beyond_max_bag below): its text, or nullptr for a record that passes.
int stage_batch(const Model& M, const u64* words, const u64* off, u64 n, const char* (*too_long)(const Model&, int), DevMem& mem, u64** d_words, u64** d_refs,
                int* max_bag = nullptr) {
  std::vector<u64> dev, refs(n), tmp(512);
  dev.reserve((size_t)(off[n] + n * (u64)(M.fixed - M.h0)));
  int bag = 0;
  for (u64 i = 0; i < n; i++) {
    const u64* r = words + off[i];
    const int nmsg = hdr_nmsg(r[0]);
    if ((u64)(M.h0 + nmsg) != off[i + 1] - off[i]) return fail(VSRMC_E_ARG, "record length does not match its header");
    if (const char* why = too_long(M, nmsg)) return fail(VSRMC_E_REP, why);
    bag = std::max(bag, nmsg);
    const int len = wire_to_device(M, r, tmp.data());
    refs[i] = ((u64)dev.size() << 8) | (u64)len;
    dev.insert(dev.end(), tmp.begin(), tmp.begin() + len);
  }
  if (max_bag) *max_bag = bag;
  HIPCHK(mem.upload(d_words, (const u64*)dev.data(), dev.size()));
  HIPCHK(mem.upload(d_refs, (const u64*)refs.data(), refs.size()));
  return 0;
}
const char* longer_than_255(const Model& M, int nmsg) { return M.fixed + nmsg > 255 ? "record longer than 255 words" : nullptr; }
const char* beyond_max_bag(const Model& M, int nmsg) { return nmsg > M.max_bag ? "record bag larger than max_bag" : nullptr; }

// the four compile entry points: a state (step = false) or step program for model m
int compile_predicates(const vsrmc_model* m, const char* text, bool step, vsrmc_where** out) {
  *out = nullptr;
  vsrmc_where* w = new vsrmc_where();
  std::string err;
  const int rc = where_compile(m->M, m->symmetry != 0, m->value_names, text, &w->prog, &err, step);
  if (rc) {
    delete w;
    return fail(rc == 2 ? VSRMC_E_REP : VSRMC_E_ARG, err);
  }
  w->R = m->M.R; w->C = m->M.C; w->n = m->M.n; w->L = m->M.L; w->symmetry = m->symmetry; w->model_id = m->M.model_id;
  *out = w;
  return 0;
}

}  // namespace
