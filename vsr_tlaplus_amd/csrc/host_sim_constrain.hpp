// host_sim_constrain.hpp — random walks under a state constraint and / or an action constraint: the host side of k_simulate_constrained
// (vsr_sim_constrain.hpp) beside vsrmc_simulate (host_batch.hpp) and vsrmc_simulate_where (host_sim_where.hpp), which it leaves alone
// (included by vsrmc.hip: one translation unit, the sections share its anonymous-namespace helpers).  Instantiations built: one per model (<0>, <1000>,
// <2000>) times the three ways a program can be present (state, step, both), as k_simulate_where's.
#pragma once

static_assert(VSRMC_SIM_ERR_TRIED_WIDTH == ERR_SIM_TRIED_WIDTH, "include/vsrmc.h names the kernel's error code");

namespace {

typedef void (*SimConKernel)(Model, const u64*, int, u64*, int, u32*, u16*, u64*, u64*, u32, int, int, const u32*, int, int, const u32*, int, int, u32, int, SimConCtl*);

template <int SPEC>
SimConKernel sim_con_kernel_of(bool has_state, bool has_step) {
  if (has_state && has_step) return k_simulate_constrained<SPEC, true, true>;
  return has_state ? k_simulate_constrained<SPEC, true, false> : k_simulate_constrained<SPEC, false, true>;
}

struct HostWhereStack {               // the operand stack of where_run called on the host: one record, no lanes
  int s[WHERE_MAX_DEPTH];
  int& operator[](int slot) { return s[slot]; }
};

// the exported bits of a state program on one device-layout record, evaluated here
template <int MODEL>
u32 where_bits_on_host(const WhereProgram& p, const Model& M, const u64* rec) {
  HostWhereStack S;
  const int nmsg = hdr_nmsg(rec[0]);
  return where_run<HostWhereStack, const u64*, WhereNoPair, MODEL>(p.ops.data(), M.fixed, rec, true, nmsg, nmsg, S);
}

struct SimConBufs {
  u64 *init = nullptr, *words = nullptr, *rng = nullptr, *tried = nullptr;
  u32 *depth = nullptr, *state_prog = nullptr, *step_prog = nullptr;
  u16* ords = nullptr;
  SimConCtl* ctl = nullptr;
  DevMem mem;
};

}  // namespace

extern "C" int32_t vsrmc_simulate_constrained(const vsrmc_model* m, int32_t device, const vsrmc_where* state_prog, int32_t state_constraint,
                                              const vsrmc_where* step_prog, int32_t step_constraint, uint32_t pruned_stop_mask, int32_t stop, uint32_t n_walkers,
                                              int32_t max_depth, uint64_t seed, double max_seconds, uint64_t max_rounds, vsrmc_sim_constrained_result* out) {
  if (!m || !out) return fail(VSRMC_E_ARG, "NULL argument");
  std::memset(out, 0, sizeof(*out));
  // every refusal comes before the device is looked at
  if (state_prog && state_prog->prog.step)
    return fail(VSRMC_E_ARG, "simulate constrained: a step program (vsrmc_step_predicates_compile) was given as the state program");
  if (step_prog && !step_prog->prog.step)
    return fail(VSRMC_E_ARG, "simulate constrained: a state program (vsrmc_predicates_compile) was given as the step program");
  if ((state_prog && !where_fits(state_prog, m->M, m->symmetry)) || (step_prog && !where_fits(step_prog, m->M, m->symmetry)))
    return fail(VSRMC_E_ARG, "simulate constrained: compiled for another model");
  if (state_constraint < -1 || (state_constraint >= 0 && (!state_prog || state_constraint >= (int)state_prog->prog.names.size())))
    return fail(VSRMC_E_ARG, "simulate constrained: the state program exports no predicate of index state_constraint");
  if (step_constraint < -1 || (step_constraint >= 0 && (!step_prog || step_constraint >= (int)step_prog->prog.names.size())))
    return fail(VSRMC_E_ARG, "simulate constrained: the step program exports no predicate of index step_constraint");
  if (state_constraint < 0 && step_constraint < 0)
    return fail(VSRMC_E_ARG, "simulate constrained: neither a state constraint nor an action constraint was given (vsrmc_simulate_where walks without one)");
  if ((state_constraint >= 0 && constraint_reads_aux(state_prog->prog)) || (step_constraint >= 0 && constraint_reads_aux(step_prog->prog)))
    return fail(VSRMC_E_ARG, "simulate constrained: the program of a constraint reads aux_svc or aux_client_acked, which are outside VIEW: the walk's model would not be "
                             "the constrained search's");
  if (max_depth < 1 || max_depth > 512) return fail(VSRMC_E_ARG, "simulate constrained: max_depth outside 1..512");
  if (n_walkers == 0) return fail(VSRMC_E_ARG, "simulate constrained: no walkers");
  Model M = m->M;
  M.max_bag = 255 - M.fixed;     // walkers live in HBM, not in LDS tiles: the bag may grow to what the 8-bit count can hold (as vsrmc_simulate)
  const int stride = M.fixed + M.max_bag;
  std::vector<u64> wire, dev(512);
  init_record_wire(M, wire);
  const int len = wire_to_device(M, wire.data(), dev.data());   // the H words stay 0: simulation never fingerprints
  if (state_constraint >= 0) {   // Init is subject to the state constraint: out of the model, there is nothing to walk — evaluated here, no launch
    const u32 bits = M.model_id == 1   ? where_bits_on_host<1>(state_prog->prog, M, dev.data())
                     : M.model_id == 2 ? where_bits_on_host<2>(state_prog->prog, M, dev.data())
                                       : where_bits_on_host<0>(state_prog->prog, M, dev.data());
    if (!((bits >> state_constraint) & 1)) {
      out->init_pruned = 1;
      return 0;
    }
  }
  int rc = check_device(device);
  if (rc) return rc;
  SimConBufs b;
  HIPCHK(b.mem.alloc(&b.init, 512 * 8));
  HIPCHK(b.mem.alloc(&b.words, (u64)n_walkers * stride * 8));
  HIPCHK(b.mem.alloc(&b.rng, (u64)n_walkers * 8));
  HIPCHK(b.mem.alloc(&b.tried, (u64)n_walkers * SIM_TRIED_WORDS * 8));
  HIPCHK(b.mem.alloc(&b.depth, (u64)n_walkers * 4));
  HIPCHK(b.mem.alloc(&b.ords, (u64)n_walkers * max_depth * 2));
  HIPCHK(b.mem.alloc(&b.ctl, sizeof(SimConCtl)));
  HIPCHK(b.mem.alloc(&b.state_prog, WHERE_MAX_OPS * sizeof(u32)));
  HIPCHK(b.mem.alloc(&b.step_prog, WHERE_MAX_OPS * sizeof(u32)));
  HIPCHK(hipMemcpy(b.init, dev.data(), len * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(b.depth, 0xFF, (u64)n_walkers * 4));
  HIPCHK(hipMemset(b.tried, 0, (u64)n_walkers * SIM_TRIED_WORDS * 8));
  HIPCHK(hipMemset(b.ctl, 0, sizeof(SimConCtl)));
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
  const SimConKernel kernel = M.model_id == 1 ? sim_con_kernel_of<1000>(hs, hp) : M.model_id == 2 ? sim_con_kernel_of<2000>(hs, hp) : sim_con_kernel_of<0>(hs, hp);
  const int n_state = hs ? (int)state_prog->prog.names.size() : 0, n_step = hp ? (int)step_prog->prog.names.size() : 0;
  const u32 stop_mask = state_constraint >= 0 ? (pruned_stop_mask & ~(1u << state_constraint)) : 0u;   // the constraint export itself never stops a run
  SimConCtl h;
  u64 rounds = 0;
  const double t0 = now_s();
  while (true) {
    hipLaunchKernelGGL(kernel, dim3((n_walkers + SIMW_BLOCK - 1) / SIMW_BLOCK), dim3(SIMW_BLOCK), 0, 0, M, (const u64*)b.init, len, b.words, stride, b.depth, b.ords,
                       b.rng, b.tried, n_walkers, (int)max_depth, 64, (const u32*)b.state_prog, n_state, (int)state_constraint, (const u32*)b.step_prog, n_step,
                       (int)step_constraint, stop_mask, stop ? 1 : 0, b.ctl);
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
  out->blocked = h.blocked;
  out->pruned = h.pruned;
  out->stuck = h.stuck;
  for (int k = 0; k < WHERE_MAX_EXPORTS; k++) { out->count_state[k] = h.count_state[k]; out->count_step[k] = h.count_step[k]; }
  if (h.found) {
    out->viol_mask = (int32_t)(h.viol_mask & 0x7FFFFFFFu);
    out->viol_steps = (int32_t)h.viol_depth;
    for (u32 k = 0; k < h.viol_depth && k < 512; k++) out->ords[k] = h.ords[k];
  }
  return 0;
}
