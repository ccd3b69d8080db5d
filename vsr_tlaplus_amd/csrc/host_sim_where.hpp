// host_sim_where.hpp — simulation mode with the user's state and step predicates on every walk: the host side of k_simulate_where (vsr_sim_where.hpp;
// DESIGN.md §9f) beside vsrmc_simulate (host_batch.hpp), which it leaves alone (included by vsrmc.hip: one translation unit, the sections share its
// anonymous-namespace helpers).  Instantiations built: one per model (<0>, <1000>, <2000>: generic in the constants, as k_simulate's defaults) times the
// three ways a program can be present (state, step, both).  The per-configuration specialisations 312 / 313 / 512 of k_simulate are not built for it.
#pragma once

namespace {

typedef void (*SimWhereKernel)(Model, const u64*, int, u64*, int, u32*, u16*, u64*, u32, int, int, const u32*, int, const u32*, int, int, SimWhereCtl*);

template <int SPEC>
SimWhereKernel sim_where_kernel_of(bool has_state, bool has_step) {
  if (has_state && has_step) return k_simulate_where<SPEC, true, true>;
  return has_state ? k_simulate_where<SPEC, true, false> : k_simulate_where<SPEC, false, true>;
}

struct SimWhereBufs {
  u64 *init = nullptr, *words = nullptr, *rng = nullptr;
  u32 *depth = nullptr, *state_prog = nullptr, *step_prog = nullptr;
  u16* ords = nullptr;
  SimWhereCtl* ctl = nullptr;
  DevMem mem;
};

}  // namespace

extern "C" int32_t vsrmc_simulate_where(const vsrmc_model* m, int32_t device, const vsrmc_where* state_prog, const vsrmc_where* step_prog, int32_t stop,
                                        uint32_t n_walkers, int32_t max_depth, uint64_t seed, double max_seconds, uint64_t max_rounds,
                                        vsrmc_sim_where_result* out) {
  if (!m || !out) return fail(VSRMC_E_ARG, "NULL argument");
  std::memset(out, 0, sizeof(*out));
  // every refusal comes before the device is looked at
  if (!state_prog && !step_prog) return fail(VSRMC_E_ARG, "simulate where: neither a state program nor a step program was given (vsrmc_simulate walks without one)");
  if (state_prog && state_prog->prog.step)
    return fail(VSRMC_E_ARG, "simulate where: a step program (vsrmc_step_predicates_compile) was given as the state program");
  if (step_prog && !step_prog->prog.step)
    return fail(VSRMC_E_ARG, "simulate where: a state program (vsrmc_predicates_compile) was given as the step program");
  if ((state_prog && !where_fits(state_prog, m->M, m->symmetry)) || (step_prog && !where_fits(step_prog, m->M, m->symmetry)))
    return fail(VSRMC_E_ARG, "simulate where: compiled for another model");
  if (max_depth < 1 || max_depth > 512) return fail(VSRMC_E_ARG, "simulate where: max_depth outside 1..512");
  if (n_walkers == 0) return fail(VSRMC_E_ARG, "simulate where: no walkers");
  int rc = check_device(device);
  if (rc) return rc;
  Model M = m->M;
  M.max_bag = 255 - M.fixed;     // walkers live in HBM, not in LDS tiles: the bag may grow to what the 8-bit count can hold (as vsrmc_simulate)
  const int stride = M.fixed + M.max_bag;
  std::vector<u64> wire, dev(512);
  init_record_wire(M, wire);
  const int len = wire_to_device(M, wire.data(), dev.data());   // the H words stay 0: simulation never fingerprints
  SimWhereBufs b;
  HIPCHK(b.mem.alloc(&b.init, 512 * 8));
  HIPCHK(b.mem.alloc(&b.words, (u64)n_walkers * stride * 8));
  HIPCHK(b.mem.alloc(&b.rng, (u64)n_walkers * 8));
  HIPCHK(b.mem.alloc(&b.depth, (u64)n_walkers * 4));
  HIPCHK(b.mem.alloc(&b.ords, (u64)n_walkers * max_depth * 2));
  HIPCHK(b.mem.alloc(&b.ctl, sizeof(SimWhereCtl)));
  HIPCHK(b.mem.alloc(&b.state_prog, WHERE_MAX_OPS * sizeof(u32)));
  HIPCHK(b.mem.alloc(&b.step_prog, WHERE_MAX_OPS * sizeof(u32)));
  HIPCHK(hipMemcpy(b.init, dev.data(), len * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(b.depth, 0xFF, (u64)n_walkers * 4));
  HIPCHK(hipMemset(b.ctl, 0, sizeof(SimWhereCtl)));
  if (state_prog) HIPCHK(hipMemcpy(b.state_prog, state_prog->prog.ops.data(), state_prog->prog.ops.size() * sizeof(u32), hipMemcpyHostToDevice));
  if (step_prog) HIPCHK(hipMemcpy(b.step_prog, step_prog->prog.ops.data(), step_prog->prog.ops.size() * sizeof(u32), hipMemcpyHostToDevice));
  std::vector<u64> rng(n_walkers);
  u64 x = seed;
  for (u32 i = 0; i < n_walkers; i++) {   // vsrmc_simulate's splitmix64 stream: one non-zero xorshift state per walker
    x += 0x9E3779B97F4A7C15ULL;
    u64 z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    rng[i] = z ? z : 1;
  }
  HIPCHK(hipMemcpy(b.rng, rng.data(), (u64)n_walkers * 8, hipMemcpyHostToDevice));
  const bool hs = state_prog != nullptr, hp = step_prog != nullptr;
  const SimWhereKernel kernel = M.model_id == 1 ? sim_where_kernel_of<1000>(hs, hp) : M.model_id == 2 ? sim_where_kernel_of<2000>(hs, hp) : sim_where_kernel_of<0>(hs, hp);
  const int n_state = hs ? (int)state_prog->prog.names.size() : 0, n_step = hp ? (int)step_prog->prog.names.size() : 0;
  SimWhereCtl h;
  u64 rounds = 0;
  const double t0 = now_s();
  while (true) {
    hipLaunchKernelGGL(kernel, dim3((n_walkers + SIMW_BLOCK - 1) / SIMW_BLOCK), dim3(SIMW_BLOCK), 0, 0, M, (const u64*)b.init, len, b.words, stride, b.depth, b.ords,
                       b.rng, n_walkers, (int)max_depth, 64, (const u32*)b.state_prog, n_state, (const u32*)b.step_prog, n_step, stop ? 1 : 0, b.ctl);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(&h, b.ctl, sizeof(h), hipMemcpyDeviceToHost));
    rounds++;
    if (h.found) break;
    if (max_rounds ? rounds >= max_rounds : now_s() - t0 > max_seconds) break;   // bounded by rounds, the clock is not consulted
  }
  out->seconds = now_s() - t0;
  out->found = (int32_t)h.found;
  out->steps = h.steps;
  out->walks = h.walks;
  out->rounds = rounds;
  out->n_states = h.n_states;
  out->n_pairs = h.n_pairs;
  for (int k = 0; k < WHERE_MAX_EXPORTS; k++) { out->count_state[k] = h.count_state[k]; out->count_step[k] = h.count_step[k]; }
  if (h.found) {
    out->viol_mask = (int32_t)(h.viol_mask & 0x7FFFFFFFu);
    out->viol_steps = (int32_t)h.viol_depth;
    for (u32 k = 0; k < h.viol_depth && k < 512; k++) out->ords[k] = h.ords[k];
  }
  return 0;
}
