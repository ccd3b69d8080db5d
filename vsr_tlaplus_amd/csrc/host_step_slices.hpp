// host_step_slices.hpp — the one loop that lists the transitions out of a range of parents with k_step_list (vsr_step.hpp), slice by slice, and hands every
// slice's instance list to its consumer: step_run (host_step.hpp), phase_expand_gated (host_action_constrain.hpp) and deep_where_slice
// (host_deep_where.hpp) are its callers.  The sizes of the slices and the overflow protocol are SlicePolicy's (host_slice_policy.hpp, plain C++); the
// launches, the read-back and the failure are here (included by vsrmc.hip: one translation unit, the sections share its anonymous-namespace helpers).
#pragma once
#include <functional>

#include "host_slice_policy.hpp"

namespace {

// what k_step_list reads and writes.  ev0 / ev1, when given, are recorded around the kernel alone and their time is added to *list_ms.
struct StepListing {
  const u64 *words, *refs;
  hipStream_t stream;
  int num_cus;
  u64* list;                           // list_cap = the policy's
  StepCtl* ctl;                        // n_list and scanned (its first 16 bytes) are each launch's; the rest is the consumer's
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double* list_ms = nullptr;
};

// Parents [sp.pos, sp.hi) through k_step_list.  Per slice: before(lo, end), if given, ahead of the launch; the launch; n_list and scanned copied back, ONE
// synchronisation of the stream; then either the slice is void (more instances than the list holds: listed again in halves, nothing consumed; a single
// parent that overflows fails as "<who>: one record has ...") or its parents are added to *scanned and consume(lo, end, n_instances) runs — for a slice with
// an instance; what consume leaves running on the stream is waited for by the next slice's synchronisation, or by the caller after the last.
// sp.listings and sp.relisted count the launches, also when the loop fails.  (Not a template over the two callables: the kernels' order in the code object
// follows the order of instantiation, and tools/kernel_resources.sh lists them in that order.)
int step_slices(const Model& M, const StepListing& s, SlicePolicy& sp, const char* who, u64* scanned, const std::function<int(u64, u64)>& before,
                const std::function<int(u64, u64, u64)>& consume) {
  auto* const list_kernel = KERNEL_OF(k_step_list, M);             // (where_fits: the caller's programs are this model's)
  while (sp.next()) {
    HIPCHK(hipMemsetAsync(s.ctl, 0, 16, s.stream));                // n_list, scanned: of this slice
    int rc = before ? before(sp.lo, sp.end) : 0;
    if (rc) return rc;
    if (s.ev0) HIPCHK(hipEventRecord(s.ev0, s.stream));
    hipLaunchKernelGGL(list_kernel, dim3(scan_grid(sp.end - sp.lo, s.num_cus)), dim3(256), 0, s.stream, M, s.words, s.refs, sp.lo, sp.end, s.list, sp.list_cap, s.ctl);
    HIPCHK(hipGetLastError());
    if (s.ev1) HIPCHK(hipEventRecord(s.ev1, s.stream));
    u64 head[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(head, s.ctl, 16, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    if (s.ev0) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, s.ev0, s.ev1));
      *s.list_ms += (double)ms;
    }
    switch (sp.judge(head[0])) {
      case SliceVerdict::Fail:
        return fail(VSRMC_E_REP, std::string(who) + ": one record has " + std::to_string(head[0]) + " enabled instances, the list holds " + std::to_string(sp.list_cap));
      case SliceVerdict::Relist:
        continue;
      case SliceVerdict::Accept:
        break;
    }
    *scanned += head[1];
    if (head[0] && (rc = consume(sp.lo, sp.end, head[0]))) return rc;
  }
  return 0;
}

}  // namespace
