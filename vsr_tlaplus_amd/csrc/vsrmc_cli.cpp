// vsrmc — command-line front end over the C ABI (include/vsrmc.h), keeping TLC's surface for this model:
//     vsrmc -config VSR.cfg VSR.tla [-deadlock] [-maxDepth N] [-device D] [-tableLog2 N] [-frontierGiB G] [-noTLA] [-json]
// ≙ `java -cp tla2tools.jar tlc2.TLC -config VSR.cfg VSR.tla -deadlock` (README:20 of the reference).  Output follows TLC's
// wording (progress lines, "Invariant ... is violated", "State k: <Action>" + the state in TLC value syntax, final counts).
// `-deadlock` (= do NOT check deadlock) is the default here because the spec has terminal states; pass
// -checkDeadlock to stop at the first state without successors like stock TLC would: the newest level is scanned for terminal states before it is
// expanded (vsrmc_checker_terminal_scan) and the behaviour into the one with the smallest fingerprint is printed.  -terminalReport scans every
// stored level without stopping.  -predicates FILE with -reach / -invariant / -whereReport evaluates the user's own state predicates (k_where) on every
// stored level, where -checkDeadlock scans.  -steps FILE with -stepReach / -stepInvariant / -stepReport does the same for step predicates (primed variables:
// csrc/vsr_step.hpp) over every transition out of every stored level.  With -simulate the same flags ask the same questions of random walks (csrc/vsr_sim_where.hpp).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include <unistd.h>

#include "../../include/vsrmc.h"

// invariant_mask bits (include/vsrmc.h): 0-1 in all three models, 2-3 in VSR.tla (NoLogDivergence only) and the analysis models, 4 only in VR_APP_STATE
static const char* const INVARIANT_NAMES[5] = {"AcknowledgedWriteNotLost", "AcknowledgedWritesExistOnMajority", "NoLogDivergence",
                                               "CommitNumberNeverHigherThanOpNumber", "NoAppStateDivergence"};

static void usage() {
  std::printf(
      "usage: vsrmc -config <file.cfg> <spec.tla> [options]\n"
      "  -config FILE      TLC configuration (grammar of VSR.cfg: CONSTANTS / INIT / NEXT / VIEW / SYMMETRY / INVARIANT)\n"
      "  -deadlock         do not check for deadlock (default)      -checkDeadlock   report the first terminal state\n"
      "                    (= CHECK_DEADLOCK TRUE in the cfg): every stored level is scanned before it is expanded; exit 11 with the behaviour\n"
      "                    that leads into the terminal state of the smallest fingerprint (-dumpTrace tla FILE writes it)\n"
      "  -terminalReport   scan every stored level for terminal states without stopping; one summary line at the end.  A terminal state in\n"
      "                    which AllReplicasMoveToSameView is false is printed with its behaviour (last line: Stuttering): a counter-example\n"
      "                    to ViewChangeCompletes.  Finding none is no verdict: behaviours that loop are not examined\n"
      "  -predicates FILE  state predicates in TLA+ syntax, for any loaded cfg (the language: csrc/vsr_where_parse.hpp; examples: tools/predicates_example.txt,\n"
      "                    tools/predicates_model2_example.txt, tools/predicates_model3_example.txt):\n"
      "                    one expression, or definitions Name == expr (at most 8 that are not LOCAL).  Used by:\n"
      "  -reach NAME[,NAME]      every stored level is scanned before it is expanded; the first level with a state that satisfies NAME ends the run:\n"
      "                    \"State satisfying NAME found at depth d\" and the behaviour into the one with the smallest fingerprint (a shortest one;\n"
      "                    -dumpTrace tla FILE writes it).  Exit 0 when found, 14 when the search ended without one\n"
      "  -invariant NAME[,NAME]  the same scan for ~NAME: a state in which NAME is false is reported like a violation of a built-in invariant (exit 12)\n"
      "  -whereReport      count the states that satisfy each exported predicate, level by level, without stopping; with -json a \"where\" object in\n"
      "                    the level lines.  Levels that are never stored (the Virtual / Probe lines) are not examined, and the report says how many\n"
      "  -steps FILE       step predicates (the same language plus primed variables, UNCHANGED and step_action, for any loaded cfg; examples: tools/steps_example.txt,\n"
      "                    tools/steps_model2_example.txt, tools/steps_model3_example.txt), evaluated\n"
      "                    on every transition out of every stored level (a file of its own: -predicates FILE goes through the state compiler).  Used by:\n"
      "  -stepInvariant NAME[,NAME]  a transition on which NAME is false ends the run: \"Error: Action property NAME is violated.\", the behaviour with\n"
      "                    that step at its end and the step's action name (exit 12; -dumpTrace tla FILE writes it, -json adds a line)\n"
      "  -stepReach NAME[,NAME]      the same scan for NAME itself: exit 0 when a transition satisfies it, 14 when the search ended without one\n"
      "  -stepReport       per level the pairs, the instances that raise an evaluation error and the pairs that satisfy each exported name, without\n"
      "                    stopping; with -json a \"steps\" object in the level lines.  Levels that are never stored are not examined, and the report says how many\n"
      "  -deepPredicates   with the flags above: the predicates are also evaluated on the levels beyond the record buffers (the Virtual / Probe lines) —\n"
      "                    every regenerated and inserted level and the transitions out of them, and the state predicates on the probed level too.  Report\n"
      "                    rows follow those lines; -reach / -invariant / -stepReach / -stepInvariant stop there with the messages and exit codes above.\n"
      "                    Per kind of program either the report or the query flags; not with -gpus N > 1, -simulate, -probe2At / -probe3At\n"
      "  -deepTerminal     with -checkDeadlock and / or -terminalReport (or CHECK_DEADLOCK TRUE in the cfg): terminal states are also looked for on the\n"
      "                    levels beyond the record buffers (the Virtual / Probe lines) — every regenerated and inserted level, and the probed level, whose\n"
      "                    states are written out chunk by chunk for the scan.  -checkDeadlock then stops there with the behaviour (exit 11); the report lists\n"
      "                    those levels.  Combines with -deepPredicates; not with -gpus N > 1, -simulate, -probe2At / -probe3At\n"
      "  -maxDepth N       stop after N BFS levels (Init = level 1)\n"
      "  -device D         HIP device ordinal (default 0)\n"
      "  -gpus N           N > 1: run the sharded checker on N GPUs of this node (re-executes as\n"
      "                    python3 -m torch.distributed.run ... -m vsr_tlaplus_amd.sharded_cli with the other arguments;\n"
      "                    -tableLog2 / -frontierGiB are then PER RANK; see that module for -replicateBelow, -backend, -exactTies,\n"
      "                    -checkpoint PREFIX / -recover PREFIX (one file per rank), -probeAt N)\n"
      "  -tableLog2 N      seen-set slots = 2^N x 16 B; -frontierGiB G: size of each of the two record buffers (-frontierBGiB G: the second one).\n"
      "                    Default for both: sized from the free memory of the device (the largest power of two of slots within 30 %% of it, the\n"
      "                    rest in two equal record buffers).  Levels are stored while the next one is predicted to fit; beyond that the search goes\n"
      "                    on through the seen-set alone (Virtual(L) / Probe(L+1) lines).  A seen-set that fills up is re-hashed into twice the\n"
      "                    slots while the device has the memory; when it cannot grow and is 85 %% full the run ends \"incomplete at depth N\" (exit 4).\n"
      "  -simulate         random walks instead of BFS (TLC -simulate): -depth N (default 100) -walkers N (131072) -seed S -maxSeconds T\n"
      "                    With -predicates FILE -reach / -invariant and / or -steps FILE -stepReach / -stepInvariant the same questions are asked of every\n"
      "                    state a walk stands on and every step it takes, at any depth (the BFS asks them of stored levels only): the first hit ends the\n"
      "                    run with its behaviour; exit codes as above (12 violated, 0 reached, 14 not met).  With -whereReport / -stepReport the exported\n"
      "                    predicates are counted over the walks instead, without stopping; -simRounds N: exactly N rounds of 64 steps per walker (the\n"
      "                    counts are then the same in every run with the same seed) instead of -maxSeconds\n"
      "  -walkConstraint NAME    with -simulate and -predicates FILE: the exported predicate NAME is a state constraint on the walks (TLC's simulator honours\n"
      "                    CONSTRAINT): a walker never moves into a state that fails it; Init is subject to it.  A walker draws among the enabled instances it\n"
      "                    has not been refused yet, so it leaves a state, or finds it terminal in the constrained model, within as many tries as the state\n"
      "                    has instances.  -invariant NAMES (and the built-in invariants) are checked on the refused successors as well, as -constraint does\n"
      "  -walkActionConstraint NAME  with -simulate and -steps FILE: the exported step predicate NAME is an action constraint on the walks (ACTION_CONSTRAINT):\n"
      "                    a transition that fails it is never taken.  Both combine with each other and with -reach, -invariant, -stepReach, -stepInvariant,\n"
      "                    -whereReport, -stepReport, -simRounds and -dumpTrace; with no query at all the built-in invariants are checked on the constrained\n"
      "                    walks.  A closing line gives the tries blocked, the tries pruned and the walks that ended stuck.  Not with -json\n"
      "  -validateTrace F  read a TLC trace (trace expression, or console \"State k:\" form) and check on the GPU that it is a\n"
      "                    behaviour of the model: Init, then one generated successor after the other; reports the invariants\n"
      "                    its last state violates\n"
      "  -hostFrontier     keep the two record buffers (-frontierGiB each) in pinned host memory, read / written over PCIe\n"
      "                    (state spaces whose frontier outgrows HBM; TLC's DiskStateQueue)\n"
      "  -hostFrontierMask M   the same per buffer: bit 0 = first buffer (levels 1, 3, ..), bit 1 = second (levels 2, 4, ..)\n"
      "  -probe2At N       when level N-1 is complete: level N as a VIRTUAL level (seen-set entries and invariants only) and level N+1\n"
      "                    as a PROBE level (nothing stored) — two levels beyond the last frontier that fits; the search ends there\n"
      "  -probe3At N       the same with TWO virtual levels (N, N+1) and level N+2 probed: three levels beyond the last stored one\n"
      "                    (level N-1 is expanded three times, level N twice; scratch buffers of a quarter of -frontierGiB)\n"
      "  -probeLast        when the next level does not fit the frontier buffers, still check its states' invariants without\n"
      "                    storing them (finds a violation one level beyond memory; the search ends there)\n"
      "  -coverage         print the successors generated per action of Next at the end (TLC's -coverage, totals only)\n"
      "  -dumpTrace tla FILE   write the counter-example as a TLA+ trace expression (TLC's -dumpTrace tla; the form of the reference's\n"
      "                    state_transfer_violation_trace.txt); -validateTrace reads it back\n"
      "  -dump FILE        write every distinct state in the text form of `tlc2.TLC -dump` (State k: + /\\ var = value conjuncts), level by\n"
      "                    level; for cross-checking small configurations against a real TLC run (refused beyond -dumpMax states, 1e6)\n"
      "  -checkpoint FILE  write a checkpoint between levels (stored ones and Virtual(L) ones alike), at most every -checkpointMinutes M\n"
      "                    (default 30; 0 = after every level)\n"
      "  -audit            second-hash audit (TLC: a rerun under another -fp N): when the search has ended, run it again to the same depth under\n"
      "                    another member of the fingerprint family and compare every level's new / generated / deadlock counts: a 64-bit\n"
      "                    collision that hid a state under one function would have to repeat under the other (exit 13 if they differ)\n"
      "  -recover FILE     continue the search a checkpoint stopped at (same constants; buffer sizes may differ)\n"
      "  -noTLA            do not read / hash-check the .tla file (only the cfg)\n"
      "  -constraint NAME  with -predicates FILE: the exported predicate NAME is a state constraint (TLC's CONSTRAINT): a state that fails it is generated,\n"
      "                    counted and checked against the invariants, but it is no distinct state and is not explored further; Init is subject to it.  Levels\n"
      "                    are stored only: when the next one does not fit the record buffers the run ends, incomplete (exit 4).  -invariant NAMES are checked\n"
      "                    on the states the constraint prunes as well.  Not with -gpus N > 1, -simulate, -deepPredicates, -probeLast, -probe2At, -probe3At,\n"
      "                    -checkpoint, -recover, -audit.  With -json the level lines carry \"kept\" and \"pruned\"\n"
      "  -deepConstraint   with -constraint NAME: the constraint is applied on the levels beyond the record buffers as well (every scratch slice of a descent is\n"
      "                    filtered before anything reads it), so the run goes on past them instead of ending with exit 4.  The Virtual lines then carry the\n"
      "                    in-model figures; a level that reached the seen-set before its records could be judged is marked so and gets a Filtered(L) line\n"
      "                    from the next pass; the closing line gives the kept and pruned totals.  -probeLast is allowed; not with -actionConstraint,\n"
      "                    -deepPredicates, -deepTerminal, -probe2At, -probe3At, -checkpoint, -recover, -audit, -gpus N > 1\n"
      "  -actionConstraint NAME  with -steps FILE: the exported step predicate NAME is an action constraint (TLC's ACTION_CONSTRAINT): a transition that\n"
      "                    fails it is generated and counted but not taken; its successor may still be reached through a permitted transition.  Init is not\n"
      "                    subject to it; every behaviour printed takes permitted steps only.  Combines with -constraint, -invariant, -reach, -stepInvariant,\n"
      "                    -stepReach, -checkDeadlock and -dumpTrace.  Levels are stored only, as with -constraint (exit 4 when the next one does not fit).\n"
      "                    Not with -gpus N > 1, -simulate, -deepPredicates, -probeLast, -probe2At, -probe3At, -checkpoint, -recover, -audit.  With -json the\n"
      "                    level lines carry \"permitted\" and \"blocked\"\n"
      "  -deepActionConstraint  with -actionConstraint NAME: the action constraint is applied on the levels beyond the record buffers as well (the record-less\n"
      "                    first pass, the level a descent inserts and the probed level take permitted transitions only), so the run goes on past them instead of\n"
      "                    ending with exit 4.  The Virtual and Probe lines then carry the transitions not taken, and the closing line's totals include those\n"
      "                    levels.  Not with -constraint, -deepPredicates, -deepTerminal, -probeLast, -probe2At, -probe3At, -checkpoint, -recover,\n"
      "                    -audit, -gpus N > 1\n"
      "  -json             one JSON object per level on stdout instead of TLC-style progress lines\n");
}

// -gpus N: hand the run to the multi-GPU front end (one process per GPU under torch.distributed.run)
static int exec_sharded(int argc, char** argv, int gpus_at) {
  std::string exe = argv[0];
  char real[4096];
  ssize_t n = readlink("/proc/self/exe", real, sizeof(real) - 1);
  if (n > 0) { real[n] = 0; exe = real; }
  std::string root = exe.substr(0, exe.find_last_of('/'));          // .../vsr-tlaplus_amd
  root = root.substr(0, root.find_last_of('/'));                    // repository root (holds the vsr_tlaplus_amd import shim)
  const char* old = getenv("PYTHONPATH");
  setenv("PYTHONPATH", old && *old ? (root + ":" + old).c_str() : root.c_str(), 1);
  const char* port = getenv("MASTER_PORT");
  std::vector<std::string> args = {"python3", "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", argv[gpus_at + 1],
                                   "--master-addr", "127.0.0.1", "--master-port", port ? port : "29500", "-m", "vsr_tlaplus_amd.sharded_cli"};
  for (int i = 1; i < argc; i++)
    if (i != gpus_at && i != gpus_at + 1) args.push_back(argv[i]);
  std::vector<char*> cargs;
  for (auto& a : args) cargs.push_back(const_cast<char*>(a.c_str()));
  cargs.push_back(nullptr);
  execvp("python3", cargs.data());
  std::perror("vsrmc: cannot start python3");
  return 1;
}

// -dumpTrace tla FILE: the counter-example as a TLA+ trace expression — the form of the reference's state_transfer_violation_trace.txt
// (a sequence of records, each with TLC's _TEAction field in front of the variables); source locations are not tracked by the
// lowering, so `location` says so for every step.  The product's reader (-validateTrace) takes the file back.
static bool write_trace_expression(const std::string& path, const vsrmc_model* m, const std::vector<uint64_t>& words,
                                   const std::vector<uint64_t>& off, const std::vector<int32_t>& acts, uint64_t n_states) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return false;
  std::fprintf(f, "<<\n");
  for (uint64_t t = 0; t < n_states; t++) {
    int64_t need = 0;
    vsrmc_model_format_state(m, &words[off[t]], nullptr, 0, &need);
    std::string buf((size_t)need, '\0');
    vsrmc_model_format_state(m, &words[off[t]], &buf[0], need, &need);
    while (!buf.empty() && buf.back() == '\0') buf.pop_back();
    const size_t first_nl = buf.find('\n');                     // "[\nvar |-> value,\n...\n]": splice the _TEAction field after the bracket
    std::fprintf(f, "[\n _TEAction |-> [\n   position |-> %llu,\n   name |-> \"%s\",\n   location |-> \"Unknown location\"\n ],\n%s%s\n",
                 (unsigned long long)(t + 1), vsrmc_action_name(acts[t]), first_nl == std::string::npos ? "" : buf.c_str() + first_nl + 1,
                 t + 1 < n_states ? "," : "");
  }
  std::fprintf(f, ">>\n");
  return std::fclose(f) == 0;
}

int main(int argc, char** argv) {
  bool deep_terminal = false, deep_constraint = false, deep_action = false;
  bool deep_predicates = false, constrained = false, action_constrained = false, walk_constrained = false, walk_action_constrained = false;
  for (int i = 1; i < argc; i++) {
    if (std::string(argv[i]) == "-walkConstraint") walk_constrained = true;
    if (std::string(argv[i]) == "-walkActionConstraint") walk_action_constrained = true;
    if (std::string(argv[i]) == "-deepPredicates") deep_predicates = true;
    if (std::string(argv[i]) == "-deepTerminal") deep_terminal = true;
    if (std::string(argv[i]) == "-constraint") constrained = true;
    if (std::string(argv[i]) == "-deepConstraint") deep_constraint = true;
    if (std::string(argv[i]) == "-actionConstraint") action_constrained = true;
    if (std::string(argv[i]) == "-deepActionConstraint") deep_action = true;
  }
  for (int i = 1; i + 1 < argc; i++)
    if (std::string(argv[i]) == "-gpus" && std::atoi(argv[i + 1]) > 1) {
      if (deep_predicates) { std::fprintf(stderr, "Error: -deepPredicates runs on one GPU: sharded checkers are not scanned (-gpus 1)\n"); return 2; }
      if (deep_terminal) { std::fprintf(stderr, "Error: -deepTerminal runs on one GPU: sharded checkers are not scanned (-gpus 1)\n"); return 2; }
      if (constrained) { std::fprintf(stderr, "Error: -constraint runs on one GPU: sharded checkers are not constrained (-gpus 1)\n"); return 2; }
      if (action_constrained) { std::fprintf(stderr, "Error: -actionConstraint runs on one GPU: sharded checkers are not constrained (-gpus 1)\n"); return 2; }
      return exec_sharded(argc, argv, i);
    }
  std::string cfg, tla, trace_file, chk_file, recover_file, dump_file, dump_trace_file, predicates_file, reach_arg, invariant_arg, constraint_arg, action_constraint_arg, walk_constraint_arg, walk_action_constraint_arg, steps_file, step_reach_arg, step_invariant_arg;
  bool where_report = false, step_report = false;
  unsigned long long dump_max = 1000000ull, dumped = 0;
  double chk_minutes = 30.0;
  bool check_deadlock = false, no_tla = false, json = false, simulate = false, host_frontier = false, probe_last = false, coverage = false, audit = false, terminal_report = false;
  int sim_depth = 100;
  unsigned sim_walkers = 1u << 17;
  unsigned long long sim_seed = 1;
  double sim_seconds = 60.0;
  unsigned long long sim_rounds = 0;
  int max_depth = 1 << 30, device = 0, table_log2 = 0, probe2_at = 0, probe3_at = 0, host_mask = 0;   // 0 = sized from the free device memory
  double frontier_gib = 0.0, frontier_b_gib = 0.0;
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    if (a == "--help" || a == "-h" || a == "-help") { usage(); return 0; }
    else if (a == "-config" && i + 1 < argc) cfg = argv[++i];
    else if (a == "-deadlock") check_deadlock = false;
    else if (a == "-checkDeadlock") check_deadlock = true;
    else if (a == "-maxDepth" && i + 1 < argc) max_depth = std::atoi(argv[++i]);
    else if (a == "-device" && i + 1 < argc) device = std::atoi(argv[++i]);
    else if (a == "-gpus" && i + 1 < argc) ++i;                   // 1: this process
    else if (a == "-tableLog2" && i + 1 < argc) table_log2 = std::atoi(argv[++i]);
    else if (a == "-frontierGiB" && i + 1 < argc) frontier_gib = std::atof(argv[++i]);
    else if (a == "-frontierBGiB" && i + 1 < argc) frontier_b_gib = std::atof(argv[++i]);
    else if (a == "-noTLA") no_tla = true;
    else if (a == "-hostFrontier") host_frontier = true;
    else if (a == "-probeLast") probe_last = true;
    else if (a == "-probe2At" && i + 1 < argc) probe2_at = std::atoi(argv[++i]);
    else if (a == "-probe3At" && i + 1 < argc) probe3_at = std::atoi(argv[++i]);
    else if (a == "-hostFrontierMask" && i + 1 < argc) host_mask = std::atoi(argv[++i]);
    else if (a == "-validateTrace" && i + 1 < argc) trace_file = argv[++i];
    else if (a == "-checkpoint" && i + 1 < argc) chk_file = argv[++i];
    else if (a == "-checkpointMinutes" && i + 1 < argc) chk_minutes = std::atof(argv[++i]);
    else if (a == "-recover" && i + 1 < argc) recover_file = argv[++i];
    else if (a == "-dump" && i + 1 < argc) dump_file = argv[++i];
    else if (a == "-dumpTrace" && i + 2 < argc && std::string(argv[i + 1]) == "tla") { dump_trace_file = argv[i + 2]; i += 2; }
    else if (a == "-dumpMax" && i + 1 < argc) dump_max = std::strtoull(argv[++i], nullptr, 10);
    else if (a == "-simulate") simulate = true;
    else if (a == "-depth" && i + 1 < argc) sim_depth = std::atoi(argv[++i]);
    else if (a == "-walkers" && i + 1 < argc) sim_walkers = (unsigned)std::strtoul(argv[++i], nullptr, 10);
    else if (a == "-seed" && i + 1 < argc) sim_seed = std::strtoull(argv[++i], nullptr, 10);
    else if (a == "-maxSeconds" && i + 1 < argc) sim_seconds = std::atof(argv[++i]);
    else if (a == "-simRounds" && i + 1 < argc) sim_rounds = std::strtoull(argv[++i], nullptr, 10);
    else if (a == "-json") json = true;
    else if (a == "-coverage") coverage = true;
    else if (a == "-audit") audit = true;
    else if (a == "-terminalReport") terminal_report = true;
    else if (a == "-predicates" && i + 1 < argc) predicates_file = argv[++i];
    else if (a == "-reach" && i + 1 < argc) reach_arg = argv[++i];
    else if (a == "-invariant" && i + 1 < argc) invariant_arg = argv[++i];
    else if (a == "-whereReport") where_report = true;
    else if (a == "-constraint" && i + 1 < argc) constraint_arg = argv[++i];
    else if (a == "-actionConstraint" && i + 1 < argc) action_constraint_arg = argv[++i];
    else if (a == "-walkConstraint" && i + 1 < argc) walk_constraint_arg = argv[++i];
    else if (a == "-walkActionConstraint" && i + 1 < argc) walk_action_constraint_arg = argv[++i];
    else if (a == "-steps" && i + 1 < argc) steps_file = argv[++i];
    else if (a == "-stepReach" && i + 1 < argc) step_reach_arg = argv[++i];
    else if (a == "-stepInvariant" && i + 1 < argc) step_invariant_arg = argv[++i];
    else if (a == "-stepReport") step_report = true;
    else if (a == "-deepPredicates") deep_predicates = true;
    else if (a == "-deepTerminal") deep_terminal = true;
    else if (a == "-deepConstraint") deep_constraint = true;
    else if (a == "-deepActionConstraint") deep_action = true;
    else if (a == "-workers" && i + 1 < argc) ++i;   // accepted for command-line compatibility; the GPU is the worker pool
    else if (!a.empty() && a[0] != '-') tla = a;
    else { std::fprintf(stderr, "vsrmc: unknown option %s\n", a.c_str()); usage(); return 2; }
  }
  if (cfg.empty()) { usage(); return 2; }
  if (deep_constraint) {                                          // refused before any device call
    const char* why = !constrained ? "-deepConstraint needs -constraint NAME: it is that constraint which is applied beyond the record buffers"
                      : action_constrained ? "-deepConstraint cannot be combined with -actionConstraint: beyond the record buffers the transitions are not judged, only a state constraint is applied there"
                      : deep_predicates ? "-deepConstraint cannot be combined with -deepPredicates: the probed level's successors are judged on arrival, which the attached scans do not know about"
                      : deep_terminal ? "-deepConstraint cannot be combined with -deepTerminal: the probed level's successors are judged on arrival, which the terminal attachment does not know about"
                      : (probe2_at > 0 || probe3_at > 0) ? "-deepConstraint cannot be combined with -probe2At / -probe3At: those passes do not filter" : nullptr;
    if (why) { std::fprintf(stderr, "Error: %s\n", why); return 2; }
  }
  if (deep_action) {                                              // refused before any device call
    const char* why = !action_constrained ? "-deepActionConstraint needs -actionConstraint NAME: it is that constraint which is applied beyond the record buffers"
                      : constrained ? "-deepActionConstraint cannot be combined with -constraint: the record-less pass beyond the record buffers cannot judge states"
                      : deep_predicates ? "-deepActionConstraint cannot be combined with -deepPredicates: the attached scans read transitions the gate does not take"
                      : deep_terminal ? "-deepActionConstraint cannot be combined with -deepTerminal: the terminal attachment scans passes that do not know the gate"
                      : (probe_last || probe2_at > 0 || probe3_at > 0) ? "-deepActionConstraint cannot be combined with -probeLast / -probe2At / -probe3At: those passes do not gate" : nullptr;
    if (why) { std::fprintf(stderr, "Error: %s\n", why); return 2; }
  }
  if (constrained) {                                              // refused before any device call
    const char* why = constraint_arg.empty() ? "-constraint needs a NAME"
                      : predicates_file.empty() ? "-constraint NAME needs -predicates FILE"
                      : simulate ? "-constraint belongs to the exhaustive search: a random walk (-simulate) is not constrained: use -walkConstraint NAME"
                      : deep_predicates ? "-constraint cannot be combined with -deepPredicates: the levels beyond the record buffers are not constrained"
                      : ((probe_last && !deep_constraint) || probe2_at > 0 || probe3_at > 0) ? "-constraint cannot be combined with -probeLast / -probe2At / -probe3At: the levels beyond the record buffers are not constrained"
                      : (!chk_file.empty() || !recover_file.empty()) ? "-constraint cannot be combined with -checkpoint / -recover: a checkpoint does not name the constraint"
                      : audit ? "-constraint cannot be combined with -audit" : nullptr;
    if (why) { std::fprintf(stderr, "Error: %s\n", why); return 2; }
  }
  if (action_constrained) {                                       // refused before any device call
    const char* why = action_constraint_arg.empty() ? "-actionConstraint needs a NAME"
                      : steps_file.empty() ? "-actionConstraint NAME needs -steps FILE"
                      : simulate ? "-actionConstraint belongs to the exhaustive search: a random walk (-simulate) is not constrained: use -walkActionConstraint NAME"
                      : deep_predicates ? "-actionConstraint cannot be combined with -deepPredicates: the levels beyond the record buffers are not constrained"
                      : (probe_last || probe2_at > 0 || probe3_at > 0) ? "-actionConstraint cannot be combined with -probeLast / -probe2At / -probe3At: the levels beyond the record buffers are not constrained"
                      : (!chk_file.empty() || !recover_file.empty()) ? "-actionConstraint cannot be combined with -checkpoint / -recover: a checkpoint does not name the constraint"
                      : audit ? "-actionConstraint cannot be combined with -audit" : nullptr;
    if (why) { std::fprintf(stderr, "Error: %s\n", why); return 2; }
  }
  if (walk_constrained || walk_action_constrained) {              // refused before any device call
    const char* why = walk_constrained && walk_constraint_arg.empty() ? "-walkConstraint needs a NAME"
                      : walk_action_constrained && walk_action_constraint_arg.empty() ? "-walkActionConstraint needs a NAME"
                      : !simulate ? "-walkConstraint / -walkActionConstraint belong to -simulate: the exhaustive search takes -constraint NAME / -actionConstraint NAME"
                      : walk_constrained && predicates_file.empty() ? "-walkConstraint NAME needs -predicates FILE"
                      : walk_action_constrained && steps_file.empty() ? "-walkActionConstraint NAME needs -steps FILE"
                      : json ? "-walkConstraint / -walkActionConstraint cannot be combined with -json" : nullptr;
    if (why) { std::fprintf(stderr, "Error: %s\n", why); return 2; }
  }
  if (deep_predicates) {                                          // refused before any device call
    const bool state_query = !reach_arg.empty() || !invariant_arg.empty(), step_query = !step_reach_arg.empty() || !step_invariant_arg.empty();
    if (!state_query && !where_report && !step_query && !step_report) {
      std::fprintf(stderr, "Error: -deepPredicates needs -reach / -invariant / -whereReport (with -predicates FILE) or -stepReach / -stepInvariant / -stepReport (with -steps FILE)\n");
      return 2;
    }
    if (simulate) { std::fprintf(stderr, "Error: -deepPredicates belongs to the exhaustive search: -simulate evaluates the predicates on its walks\n"); return 2; }
    if (probe2_at > 0 || probe3_at > 0) { std::fprintf(stderr, "Error: -deepPredicates cannot be combined with -probe2At / -probe3At\n"); return 2; }
    if ((state_query && where_report) || (step_query && step_report)) {
      std::fprintf(stderr, "Error: -deepPredicates attaches one program of each kind: either -whereReport or -reach / -invariant, either -stepReport or -stepReach / -stepInvariant\n");
      return 2;
    }
  }
  if (deep_terminal) {                                            // refused before any device call
    const char* why = simulate ? "-deepTerminal belongs to the exhaustive search: -simulate ends a walk at a terminal state by itself"
                      : (probe2_at > 0 || probe3_at > 0) ? "-deepTerminal cannot be combined with -probe2At / -probe3At"
                      : (constrained || action_constrained) ? "-deepTerminal cannot be combined with -constraint / -actionConstraint: the levels beyond the record buffers are not constrained"
                      : nullptr;
    if (why) { std::fprintf(stderr, "Error: %s\n", why); return 2; }
  }
  vsrmc_model* m = nullptr;
  if (vsrmc_model_load(no_tla || tla.empty() ? nullptr : tla.c_str(), cfg.c_str(), &m) != 0) {
    std::fprintf(stderr, "Error: %s\n", vsrmc_last_error());
    return 1;
  }
  vsrmc_layout lay;
  vsrmc_model_info(m, &lay);
  if (lay.check_deadlock) check_deadlock = true;
  if (deep_terminal && !check_deadlock && !terminal_report) {     // (the cfg is a file: still no device call)
    std::fprintf(stderr, "Error: -deepTerminal needs -checkDeadlock (or CHECK_DEADLOCK TRUE in the cfg) and / or -terminalReport\n");
    return 2;
  }
  if (!trace_file.empty()) {   // import of a TLC trace: is it a behaviour of the lowered model?
    std::ifstream f(trace_file, std::ios::binary);
    if (!f) { std::fprintf(stderr, "Error: cannot read %s\n", trace_file.c_str()); return 1; }
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    uint64_t n = 0;
    if (vsrmc_model_parse_states(m, text.c_str(), nullptr, 0, nullptr, nullptr, 0, &n) != 0) {
      std::fprintf(stderr, "Error: %s\n", vsrmc_last_error());
      return 1;
    }
    std::vector<uint64_t> words((n + 1) * 320), off(n + 1);
    std::vector<int32_t> named(n + 1), acts(n + 1, -1);
    std::vector<uint32_t> ords(n + 1);
    int64_t bad = -1;
    int32_t inv = 0;
    if (vsrmc_model_parse_states(m, text.c_str(), words.data(), words.size(), off.data(), named.data(), n + 1, &n) != 0 ||
        vsrmc_model_check_trace(m, device, words.data(), off.data(), n, ords.data(), acts.data(), &bad, &inv) != 0) {
      std::fprintf(stderr, "Error: %s\n", vsrmc_last_error());
      return 1;
    }
    std::printf("%llu states read from %s.\n", (unsigned long long)n, trace_file.c_str());
    const uint64_t good = bad < 0 ? n : (uint64_t)bad;
    for (uint64_t t = 0; t < good; t++) {
      const char* mark = (named[t] >= 0 && named[t] != acts[t]) ? "   (the file names a different action for the same step)" : "";
      if (t == 0) std::printf("State 1: <Initial predicate>%s\n", mark);
      else std::printf("State %llu: <%s> ordinal %u%s\n", (unsigned long long)(t + 1), vsrmc_action_name(acts[t]), ords[t - 1], mark);
    }
    int code = 0;
    if (bad >= 0) {
      std::printf("Error: state %lld is not %s.\n", (long long)(bad + 1), bad == 0 ? "the initial state" : "a successor of its predecessor");
      code = 1;
    } else {
      std::printf("The trace is a behaviour of the model.\n");
      const char* const* names = INVARIANT_NAMES;
      for (int b = 0; b < 5; b++)
        if (inv & (1 << b)) { std::printf("Its last state violates invariant %s.\n", names[b]); code = 12; }
    }
    vsrmc_model_destroy(m);
    return code;
  }
  // state predicates (-predicates FILE): `w_all` = the file as written (-whereReport counts its exported names); `w_query` = the names of -reach, then
  // the negations of the names of -invariant, over the file with every definition made LOCAL
  vsrmc_where *w_all = nullptr, *w_query = nullptr, *w_con = nullptr;   // w_con (-constraint): the negations of the names of -invariant, then the constraint
  int con_index = -1;
  std::vector<std::string> con_inv_names;
  std::vector<std::string> where_names, query_names;
  size_t n_reach = 0;
  auto split_names = [](const std::string& arg, std::vector<std::string>& out) {
    std::stringstream ss(arg);
    std::string name;
    while (std::getline(ss, name, ','))
      if (!name.empty()) out.push_back(name);
  };
  auto make_local = [](const std::string& text) {               // every `Name ==` that is not LOCAL already gets the word in front
    std::string local;
    for (size_t i = 0; i < text.size(); i++) {
      if (text.compare(i, 2, "==") == 0 && (i == 0 || text[i - 1] != '=') && (i + 2 >= text.size() || text[i + 2] != '=')) {
        size_t e = local.size();
        while (e > 0 && std::isspace((unsigned char)local[e - 1])) e--;
        size_t b = e;
        while (b > 0 && (std::isalnum((unsigned char)local[b - 1]) || local[b - 1] == '_')) b--;
        size_t q = b;
        while (q > 0 && std::isspace((unsigned char)local[q - 1])) q--;
        if (b < e && !(q >= 5 && local.compare(q - 5, 5, "LOCAL") == 0)) local.insert(b, "LOCAL ");
      }
      local.push_back(text[i]);
    }
    return local;
  };
  // step predicates (-steps FILE): the same two programs over pairs
  vsrmc_where *s_all = nullptr, *s_query = nullptr;
  std::vector<std::string> step_names, step_query_names;
  size_t n_step_reach = 0;
  // -walkConstraint / -walkActionConstraint (with -simulate): `w_walk` / `s_walk` = the query program of the kind (may have no query) with the constraint
  // as one more exported predicate behind the queries, at index walk_con / walk_act; a report counts over w_all / s_all, where the constraint is the
  // export of its own name, at index walk_con_all / walk_act_all
  vsrmc_where *w_walk = nullptr, *s_walk = nullptr;
  int walk_con = -1, walk_act = -1, walk_con_all = -1, walk_act_all = -1;
  if (!step_reach_arg.empty() || !step_invariant_arg.empty() || step_report || walk_action_constrained) {
    if (steps_file.empty()) { std::fprintf(stderr, "Error: -stepReach / -stepInvariant / -stepReport need -steps FILE\n"); return 2; }
    std::ifstream pf(steps_file, std::ios::binary);
    if (!pf) { std::fprintf(stderr, "Error: cannot read %s\n", steps_file.c_str()); return 1; }
    std::stringstream pss;
    pss << pf.rdbuf();
    const std::string text = pss.str();
    if (vsrmc_step_predicates_compile(m, text.c_str(), &s_all) != 0) { std::fprintf(stderr, "Error: %s:%s\n", steps_file.c_str(), vsrmc_last_error()); return 1; }
    vsrmc_where_desc wd;
    vsrmc_where_describe(s_all, &wd);
    for (int k = 0; k < wd.n_names; k++) step_names.push_back(wd.names[k]);
    split_names(step_reach_arg, step_query_names);
    n_step_reach = step_query_names.size();
    split_names(step_invariant_arg, step_query_names);
    if (!step_query_names.empty()) {
      std::string local = make_local(text);
      for (size_t k = 0; k < step_query_names.size(); k++) {
        bool known = false;
        for (const std::string& n : step_names) known = known || n == step_query_names[k];
        if (!known) { std::fprintf(stderr, "Error: %s exports no predicate %s\n", steps_file.c_str(), step_query_names[k].c_str()); return 2; }
        local += "\nQuery" + std::to_string(k) + " == " + (k < n_step_reach ? "" : "~") + step_query_names[k];
      }
      if (vsrmc_step_predicates_compile(m, local.c_str(), &s_query) != 0) { std::fprintf(stderr, "Error: %s\n", vsrmc_last_error()); return 1; }
    }
    if (walk_action_constrained) {
      for (size_t k = 0; k < step_names.size(); k++)
        if (step_names[k] == walk_action_constraint_arg) walk_act_all = (int)k;
      if (walk_act_all < 0) { std::fprintf(stderr, "Error: %s exports no predicate %s\n", steps_file.c_str(), walk_action_constraint_arg.c_str()); return 2; }
      if (step_query_names.size() > 7) { std::fprintf(stderr, "Error: -walkActionConstraint with more than 7 -stepReach / -stepInvariant names\n"); return 2; }
      std::string local = make_local(text);
      for (size_t k = 0; k < step_query_names.size(); k++) local += "\nQuery" + std::to_string(k) + " == " + (k < n_step_reach ? "" : "~") + step_query_names[k];
      local += "\nWalkActionConstraintQuery == " + walk_action_constraint_arg;
      walk_act = (int)step_query_names.size();
      if (vsrmc_step_predicates_compile(m, local.c_str(), &s_walk) != 0) { std::fprintf(stderr, "Error: %s\n", vsrmc_last_error()); return 1; }
    }
  }
  // -actionConstraint NAME: a program of its own over the same file, every definition LOCAL and the constraint its one exported predicate
  vsrmc_where* s_act = nullptr;
  if (action_constrained) {
    std::ifstream pf(steps_file, std::ios::binary);
    if (!pf) { std::fprintf(stderr, "Error: cannot read %s\n", steps_file.c_str()); return 1; }
    std::stringstream pss;
    pss << pf.rdbuf();
    const std::string text = pss.str();
    vsrmc_where* whole = nullptr;
    if (vsrmc_step_predicates_compile(m, text.c_str(), &whole) != 0) { std::fprintf(stderr, "Error: %s:%s\n", steps_file.c_str(), vsrmc_last_error()); return 1; }
    vsrmc_where_desc wd;
    vsrmc_where_describe(whole, &wd);
    bool known = false;
    for (int k = 0; k < wd.n_names; k++) known = known || action_constraint_arg == wd.names[k];
    vsrmc_where_destroy(whole);
    if (!known) { std::fprintf(stderr, "Error: %s exports no predicate %s\n", steps_file.c_str(), action_constraint_arg.c_str()); return 2; }
    const std::string local = make_local(text) + "\nActionConstraintQuery == " + action_constraint_arg;
    if (vsrmc_step_predicates_compile(m, local.c_str(), &s_act) != 0) { std::fprintf(stderr, "Error: %s\n", vsrmc_last_error()); return 1; }
  }
  if (!reach_arg.empty() || !invariant_arg.empty() || where_report || constrained || walk_constrained) {
    if (predicates_file.empty()) { std::fprintf(stderr, "Error: -reach / -invariant / -whereReport need -predicates FILE\n"); return 2; }
    std::ifstream pf(predicates_file, std::ios::binary);
    if (!pf) { std::fprintf(stderr, "Error: cannot read %s\n", predicates_file.c_str()); return 1; }
    std::stringstream pss;
    pss << pf.rdbuf();
    const std::string text = pss.str();
    if (vsrmc_predicates_compile(m, text.c_str(), &w_all) != 0) { std::fprintf(stderr, "Error: %s:%s\n", predicates_file.c_str(), vsrmc_last_error()); return 1; }
    vsrmc_where_desc wd;
    vsrmc_where_describe(w_all, &wd);
    for (int k = 0; k < wd.n_names; k++) where_names.push_back(wd.names[k]);
    split_names(reach_arg, query_names);
    n_reach = query_names.size();
    split_names(invariant_arg, query_names);
    if (!query_names.empty()) {
      std::string local = make_local(text);
      for (size_t k = 0; k < query_names.size(); k++) {
        bool known = false;
        for (const std::string& n : where_names) known = known || n == query_names[k];
        if (!known) { std::fprintf(stderr, "Error: %s exports no predicate %s\n", predicates_file.c_str(), query_names[k].c_str()); return 2; }
        local += "\nQuery" + std::to_string(k) + " == " + (k < n_reach ? "" : "~") + query_names[k];
      }
      if (vsrmc_predicates_compile(m, local.c_str(), &w_query) != 0) { std::fprintf(stderr, "Error: %s\n", vsrmc_last_error()); return 1; }
    }
    if (constrained) {
      bool known = false;
      for (const std::string& n : where_names) known = known || n == constraint_arg;
      if (!known) { std::fprintf(stderr, "Error: %s exports no predicate %s\n", predicates_file.c_str(), constraint_arg.c_str()); return 2; }
      split_names(invariant_arg, con_inv_names);
      if (con_inv_names.size() > 7) { std::fprintf(stderr, "Error: -constraint with more than 7 -invariant names\n"); return 2; }
      std::string local = make_local(text);
      for (size_t k = 0; k < con_inv_names.size(); k++) local += "\nPrunedQuery" + std::to_string(k) + " == ~" + con_inv_names[k];
      local += "\nConstraintQuery == " + constraint_arg;
      con_index = (int)con_inv_names.size();
      if (vsrmc_predicates_compile(m, local.c_str(), &w_con) != 0) { std::fprintf(stderr, "Error: %s\n", vsrmc_last_error()); return 1; }
    }
    if (walk_constrained) {
      for (size_t k = 0; k < where_names.size(); k++)
        if (where_names[k] == walk_constraint_arg) walk_con_all = (int)k;
      if (walk_con_all < 0) { std::fprintf(stderr, "Error: %s exports no predicate %s\n", predicates_file.c_str(), walk_constraint_arg.c_str()); return 2; }
      if (query_names.size() > 7) { std::fprintf(stderr, "Error: -walkConstraint with more than 7 -reach / -invariant names\n"); return 2; }
      std::string local = make_local(text);
      for (size_t k = 0; k < query_names.size(); k++) local += "\nQuery" + std::to_string(k) + " == " + (k < n_reach ? "" : "~") + query_names[k];
      local += "\nWalkConstraintQuery == " + walk_constraint_arg;
      walk_con = (int)query_names.size();
      if (vsrmc_predicates_compile(m, local.c_str(), &w_walk) != 0) { std::fprintf(stderr, "Error: %s\n", vsrmc_last_error()); return 1; }
    }
  }
  if (simulate) {   // ≙ tlc2.TLC -simulate -depth N
    // the walk Init .. ords[n_steps), printed the way the BFS prints a behaviour
    auto print_walk = [&](const char* header, const uint32_t* ords, int n_steps, std::vector<int32_t>* acts_out) -> bool {
      std::printf("%s\n", header);
      uint64_t cap_w = (uint64_t)(n_steps + 3) * 256, n_states = 0;
      std::vector<uint64_t> words(cap_w), off(n_steps + 3);
      std::vector<int32_t> acts(n_steps + 3);
      if (vsrmc_model_replay(m, device, ords, n_steps, words.data(), cap_w, off.data(), acts.data(), off.size(), &n_states) != 0) {
        std::printf("Error: %s\n", vsrmc_last_error());
        return false;
      }
      for (uint64_t t = 0; t < n_states; t++) {
        int64_t need = 0;
        vsrmc_model_format_state(m, &words[off[t]], nullptr, 0, &need);
        std::string buf((size_t)need, '\0');
        vsrmc_model_format_state(m, &words[off[t]], &buf[0], need, &need);
        std::printf("State %llu: <%s>\n%s\n\n", (unsigned long long)(t + 1), vsrmc_action_name(acts[t]), buf.c_str());
      }
      if (acts_out) acts_out->assign(acts.begin(), acts.begin() + n_states);
      if (acts_out && !dump_trace_file.empty()) {
        if (write_trace_expression(dump_trace_file, m, words, off, acts, n_states))
          std::printf("The counter-example was written to %s (TLA+ trace expression).\n", dump_trace_file.c_str());
        else
          std::printf("Warning: cannot write %s\n", dump_trace_file.c_str());
      }
      return true;
    };
    auto destroy_all = [&]() {
      if (w_all) vsrmc_where_destroy(w_all);
      if (w_query) vsrmc_where_destroy(w_query);
      if (s_all) vsrmc_where_destroy(s_all);
      if (s_query) vsrmc_where_destroy(s_query);
      if (w_walk) vsrmc_where_destroy(w_walk);
      if (s_walk) vsrmc_where_destroy(s_walk);
      vsrmc_model_destroy(m);
    };
    const bool walk_any = walk_constrained || walk_action_constrained;
    if (!w_all && !s_all) {                                         // no question of the user's: the built-in invariants alone (k_simulate)
      if (!predicates_file.empty() || !steps_file.empty() || sim_rounds) {
        std::fprintf(stderr, "Error: -simulate: -predicates FILE needs -reach / -invariant / -whereReport, -steps FILE needs -stepReach / -stepInvariant / -stepReport, "
                             "-simRounds N needs one of them\n");
        return 2;
      }
      vsrmc_sim_result r;
      if (vsrmc_simulate(m, device, sim_walkers, sim_depth, sim_seed, sim_seconds, &r) != 0) {
        std::fprintf(stderr, "Error: %s\n", vsrmc_last_error());
        return 1;
      }
      std::printf("Running Random Simulation with seed %llu: %u walkers on the GPU, depth %d.\n", sim_seed, sim_walkers, sim_depth);
      int code = 0;
      if (r.found == 1) {
        const char* const* names = INVARIANT_NAMES;
        for (int b = 0; b < 5; b++)
          if (r.viol_mask & (1 << b)) std::printf("Error: Invariant %s is violated.\n", names[b]);
        if (!print_walk("Error: The behavior up to this point is:", r.ords, r.viol_steps, nullptr)) return 1;
        code = 12;
      } else if (r.found == 2) {
        std::printf("Error: a walk raised device error %d after %d steps.\n", r.viol_mask, r.viol_steps);
        code = 1;
      } else {
        std::printf("Simulation stopped after %.1f s without a violation.\n", r.seconds);
      }
      std::printf("%llu states checked in %llu walks, %.3f s (%.3g steps/s).\n", (unsigned long long)r.steps, (unsigned long long)r.walks,
                  r.seconds, r.seconds > 0 ? (double)r.steps / r.seconds : 0.0);
      vsrmc_model_destroy(m);
      return code;
    }
    // the user's predicates on every walk (k_simulate_where): first the report (count only), then the query (stop at the first hit)
    std::printf("Running Random Simulation with seed %llu: %u walkers on the GPU, depth %d.\n", sim_seed, sim_walkers, sim_depth);
    int code = 0;
    vsrmc_sim_where_result r;
    vsrmc_sim_constrained_result rc;
    auto totals = [&]() {
      std::printf("%llu states and %llu steps evaluated in %llu walks, %llu rounds, %.3f s (%.3g steps/s).\n", (unsigned long long)r.n_states, (unsigned long long)r.n_pairs,
                  (unsigned long long)r.walks, (unsigned long long)r.rounds, r.seconds, r.seconds > 0 ? (double)r.steps / r.seconds : 0.0);
      if (walk_any)
        std::printf("Walk constraints: %llu tries blocked by the action constraint, %llu tries pruned by the state constraint, %llu walks ended stuck (every enabled "
                    "instance refused); %llu steps taken.\n", (unsigned long long)rc.blocked, (unsigned long long)rc.pruned, (unsigned long long)rc.stuck,
                    (unsigned long long)rc.steps);
    };
    // one run: under the walk constraints (k_simulate_constrained; `r` gets the fields the two results share) or as before (k_simulate_where)
    auto run_walks = [&](const vsrmc_where* ws, int ks, const vsrmc_where* wp, int kp, uint32_t pruned_stop, int stop) -> int {
      if (!walk_any) return vsrmc_simulate_where(m, device, ws, wp, stop, sim_walkers, sim_depth, sim_seed, sim_seconds, sim_rounds, &r);
      const int code = vsrmc_simulate_constrained(m, device, ws, ks, wp, kp, pruned_stop, stop, sim_walkers, sim_depth, sim_seed, sim_seconds, sim_rounds, &rc);
      if (code != 0) return code;
      r.found = rc.found; r.viol_mask = rc.viol_mask; r.viol_steps = rc.viol_steps;
      r.steps = rc.steps; r.walks = rc.walks; r.rounds = rc.rounds; r.n_states = rc.n_states; r.n_pairs = rc.n_pairs; r.seconds = rc.seconds;
      for (int k = 0; k < 8; k++) { r.count_state[k] = rc.count_state[k]; r.count_step[k] = rc.count_step[k]; }
      for (int k = 0; k < 512; k++) r.ords[k] = rc.ords[k];
      if (rc.init_pruned) std::printf("The initial state fails the constraint %s: there is nothing to walk.\n", walk_constraint_arg.c_str());
      return 0;
    };
    if (where_report || step_report) {
      if (run_walks((where_report || walk_constrained) ? w_all : nullptr, walk_con_all, (step_report || walk_action_constrained) ? s_all : nullptr, walk_act_all, 0, 0) != 0) {
        std::fprintf(stderr, "Error: %s\n", vsrmc_last_error());
        return 1;
      }
      if (r.found == 2) {
        std::printf("Error: a walk raised device error %d after %d steps.\n", r.viol_mask, r.viol_steps);
        code = 1;
      }
      if (where_report)
        for (size_t k = 0; k < where_names.size(); k++)
          std::printf("Where report: %s holds in %llu of %llu states stood on by the walks.\n", where_names[k].c_str(), (unsigned long long)r.count_state[k],
                      (unsigned long long)r.n_states);
      if (step_report)
        for (size_t k = 0; k < step_names.size(); k++)
          std::printf("Step report: %s holds on %llu of %llu pairs taken by the walks.\n", step_names[k].c_str(), (unsigned long long)r.count_step[k],
                      (unsigned long long)r.n_pairs);
      if (json) {
        std::string j = "{\"simulate\": true, \"rounds\": " + std::to_string((unsigned long long)r.rounds) + ", \"states\": " + std::to_string((unsigned long long)r.n_states) +
                        ", \"pairs\": " + std::to_string((unsigned long long)r.n_pairs) + ", \"where\": {";
        for (size_t k = 0; where_report && k < where_names.size(); k++) j += (k ? ", \"" : "\"") + where_names[k] + "\": " + std::to_string((unsigned long long)r.count_state[k]);
        j += "}, \"steps\": {";
        for (size_t k = 0; step_report && k < step_names.size(); k++) j += (k ? ", \"" : "\"") + step_names[k] + "\": " + std::to_string((unsigned long long)r.count_step[k]);
        std::printf("%s}}\n", j.c_str());
      }
      totals();
    }
    // under a walk constraint a run with no query and no report still walks: the built-in invariants on the constrained walks
    if ((w_query || s_query || (walk_any && !where_report && !step_report)) && code == 0) {
      uint32_t pruned_stop = 0;                                     // the -invariant names: checked on the states the constraint prunes as well
      for (size_t k = n_reach; walk_constrained && k < query_names.size(); k++) pruned_stop |= 1u << k;
      if (run_walks(walk_constrained ? w_walk : w_query, walk_con, walk_action_constrained ? s_walk : s_query, walk_act, pruned_stop, 1) != 0) {
        std::fprintf(stderr, "Error: %s\n", vsrmc_last_error());
        return 1;
      }
      if (r.found == 3 || r.found == 4) {
        // an invariant's (action property's) violation is reported before a reachability hit of the same state (pair), as the BFS does
        const std::vector<std::string>& names = r.found == 3 ? query_names : step_query_names;
        const size_t nr = r.found == 3 ? n_reach : n_step_reach;
        int hit = -1;
        for (size_t k = nr; k < names.size() && hit < 0; k++)
          if (r.viol_mask & (1 << k)) hit = (int)k;
        for (size_t k = 0; k < nr && hit < 0; k++)
          if (r.viol_mask & (1 << k)) hit = (int)k;
        if (hit < 0) { std::printf("Error: the walk that was reported has no bit of the query set.\n"); return 1; }
        const bool inv = (size_t)hit >= nr;
        const char* header = inv ? "Error: The behavior up to this point is:" : "The behavior up to this point is:";
        if (inv) std::printf(r.found == 3 ? "Error: Invariant %s is violated.\n" : "Error: Action property %s is violated.\n", names[hit].c_str());
        else std::printf(r.found == 3 ? "State satisfying %s found at depth %d by a random walk.\n" : "Step satisfying %s found by a random walk: the step out of depth %d.\n",
                         names[hit].c_str(), r.found == 3 ? r.viol_steps + 1 : r.viol_steps);
        std::vector<int32_t> acts;
        if (!print_walk(header, r.ords, r.viol_steps, &acts)) return 1;
        if (r.found == 4 && !acts.empty()) std::printf("The last step is %s of State %d.\n", vsrmc_action_name(acts.back()), r.viol_steps);
        if (json)
          std::printf("{\"simulate\": true, \"%s\": \"%s\", \"steps\": %d, \"action\": \"%s\"}\n",
                      r.found == 3 ? (inv ? "invariant_violated" : "reached") : (inv ? "action_property_violated" : "step_reached"), names[hit].c_str(), r.viol_steps,
                      acts.empty() ? "" : vsrmc_action_name(acts.back()));
        code = inv ? 12 : 0;
      } else if (r.found == 1) {
        const char* const* names = INVARIANT_NAMES;
        for (int b = 0; b < 5; b++)
          if (r.viol_mask & (1 << b)) std::printf("Error: Invariant %s is violated.\n", names[b]);
        std::vector<int32_t> acts;
        if (!print_walk("Error: The behavior up to this point is:", r.ords, r.viol_steps, &acts)) return 1;
        code = 12;
      } else if (r.found == 2) {
        std::printf("Error: a walk raised device error %d after %d steps.\n", r.viol_mask, r.viol_steps);
        code = 1;
      } else {
        for (size_t k = 0; k < n_reach; k++) std::printf("No state satisfying %s was met by the walks.\n", query_names[k].c_str());
        for (size_t k = 0; k < n_step_reach; k++) std::printf("No step satisfying %s was met by the walks.\n", step_query_names[k].c_str());
        std::printf("Simulation stopped after %.1f s without a violation.\n", r.seconds);
        if (n_reach || n_step_reach) code = 14;
      }
      totals();
    }
    destroy_all();
    return code;
  }
  vsrmc_options o;
  vsrmc_options_default(&o);
  o.device = device;
  o.table_log2 = table_log2;
  o.host_frontier = host_frontier ? 3 : (host_mask & 3);
  o.frontier_words = (uint64_t)(frontier_gib * 1024.0 * 1024.0 * 1024.0 / 8.0);
  o.frontier_words_b = (uint64_t)(frontier_b_gib * 1024.0 * 1024.0 * 1024.0 / 8.0);   // 0 = like the first
  o.frontier_states = o.frontier_words / 24;                   // (0 with -frontierGiB 0: derived with the words)
  o.pending_entries = (uint64_t)1 << 20;   // single-pass levels keep no pending list (the buffer only collects violators of probe levels)
  // one entry per state plus the unused tails of the per-block index chunks (<= 4096 per block per level, 510 levels at most)
  o.trace_entries = ((uint64_t)1 << table_log2) / 2 + ((uint64_t)1 << 28);   // + chunk tails: <= 1024 blocks x 8192 indices x ~30 large levels
  vsrmc_checker* c = nullptr;
  if ((recover_file.empty() ? vsrmc_checker_create(m, &o, &c) : vsrmc_checker_load(m, &o, recover_file.c_str(), &c)) != 0) {
    std::fprintf(stderr, "Error: %s\n", vsrmc_last_error());
    return 1;
  }
  vsrmc_where* const deep_state = !deep_predicates ? nullptr : w_query ? w_query : where_report ? w_all : nullptr;
  vsrmc_where* const deep_step = !deep_predicates ? nullptr : s_query ? s_query : step_report ? s_all : nullptr;
  if (deep_predicates && vsrmc_checker_deep_attach(c, deep_state, deep_step) != 0) {
    std::fprintf(stderr, "Error: %s\n", vsrmc_last_error());
    return 1;
  }
  if (deep_terminal && vsrmc_checker_deep_terminal_attach(c) != 0) {
    std::fprintf(stderr, "Error: %s\n", vsrmc_last_error());
    return 1;
  }
  if (w_con && vsrmc_checker_constrain_attach(c, w_con, con_index) != 0) {
    std::fprintf(stderr, "Error: %s\n", vsrmc_last_error());
    return 1;
  }
  if (w_con && deep_constraint && vsrmc_checker_constrain_deep(c, 1) != 0) {
    std::fprintf(stderr, "Error: %s\n", vsrmc_last_error());
    return 1;
  }
  if (s_act && vsrmc_checker_action_constrain_attach(c, s_act, 0) != 0) {
    std::fprintf(stderr, "Error: %s\n", vsrmc_last_error());
    return 1;
  }
  if (s_act && deep_action && vsrmc_checker_action_constrain_deep(c, 1) != 0) {
    std::fprintf(stderr, "Error: %s\n", vsrmc_last_error());
    return 1;
  }
  static const char* const MODULES[3] = {"VSR.tla", "VR_STATE_TRANSFER.tla", "VR_APP_STATE.tla"};
  std::printf("vsrmc: %s lowered: ReplicaCount=%d ClientCount=%d |Values|=%d StartViewOnTimerLimit=%d, %d permutation(s), "
              "invariant mask %d\n", MODULES[lay.module >= 0 && lay.module < 3 ? lay.module : 0], lay.replica_count, lay.client_count, lay.value_count, lay.start_view_on_timer_limit,
              lay.permutations, lay.invariant_mask);
  auto t0 = std::chrono::steady_clock::now();
  auto t_chk = t0;
  vsrmc_level_info info;
  vsrmc_checker_status(c, &info);
  if (w_con) std::printf("Finished computing initial states: 1 state generated, %llu in the model of CONSTRAINT %s.\n", (unsigned long long)info.distinct, constraint_arg.c_str());
  else if (recover_file.empty()) std::printf("Finished computing initial states: 1 distinct state generated.\n");
  else std::printf("Recovered from %s: level %d, %llu distinct states found, %llu states left on queue.\n", recover_file.c_str(), info.level,
                   (unsigned long long)info.distinct, (unsigned long long)info.n_new);
  int rc = 0;
  FILE* dump = nullptr;
  if (!dump_file.empty()) {
    dump = std::fopen(dump_file.c_str(), "w");
    if (!dump) { std::fprintf(stderr, "Error: cannot write %s\n", dump_file.c_str()); return 1; }
  }
  // the newest level in TLC's -dump text form: "State k:" + one "/\ var = value" conjunct per variable
  auto dump_level = [&](uint64_t n_states) -> bool {
    if (!dump || n_states == 0) return true;
    if (dumped + n_states > dump_max) {
      std::fprintf(stderr, "Error: -dump stops at %llu states (-dumpMax)\n", dump_max);
      return false;
    }
    std::vector<uint64_t> words(n_states * (uint64_t)lay.max_record_words), off(n_states + 1);
    uint64_t n = 0;
    if (vsrmc_checker_frontier(c, words.data(), words.size(), off.data(), off.size(), &n) != 0) return false;
    for (uint64_t t = 0; t < n; t++) {
      int64_t need = 0;
      vsrmc_model_format_state(m, &words[off[t]], nullptr, 0, &need);
      std::string buf((size_t)need, '\0');
      vsrmc_model_format_state(m, &words[off[t]], &buf[0], need, &need);
      std::fprintf(dump, "State %llu:\n", ++dumped);
      size_t pos = 0;
      while (pos < buf.size()) {                              // "[\nvar |-> value,\n...\n]" -> conjuncts
        size_t eol = buf.find('\n', pos);
        if (eol == std::string::npos) eol = buf.size();
        std::string line = buf.substr(pos, eol - pos);
        pos = eol + 1;
        size_t arrow = line.find(" |-> ");
        if (arrow == std::string::npos) continue;             // the brackets
        if (!line.empty() && line.back() == ',') line.pop_back();
        std::fprintf(dump, "/\\ %s = %s\n", line.substr(0, arrow).c_str(), line.substr(arrow + 5).c_str());
      }
      std::fprintf(dump, "\n");
    }
    return true;
  };
  if (dump && recover_file.empty() && !dump_level(1)) return 1;
  bool violated = false, deadlocked = false, probed_violation = false, incomplete = false;
  // -constraint: the figures of every level the filter ran on (level 1 = Init), the run's total, a user's invariant that fails among the pruned states
  bool con_no_room = false;
  std::string con_reason;
  unsigned long long con_pruned_total = 0;
  int con_seen_level = 0, con_hit = -1, con_hit_level = 0;
  uint64_t con_hit_fp = 0;
  vsrmc_constraint_info con_info;
  std::memset(&con_info, 0, sizeof(con_info));
  auto con_collect = [&]() -> bool {                              // true: the newest filtered level is one not seen before (con_info holds it)
    if (!w_con || vsrmc_checker_constraint_info(c, 0, &con_info) != 0 || con_info.level <= con_seen_level) return false;
    con_seen_level = con_info.level;
    con_pruned_total += (unsigned long long)con_info.pruned;
    for (size_t k = 0; k < con_inv_names.size() && con_hit < 0; k++)
      if (con_info.pruned_count[k]) { con_hit = (int)k; con_hit_level = con_info.level; con_hit_fp = con_info.pruned_min_fp_k[k]; }
    return true;
  };
  con_collect();                                                  // (Init)
  // -deepConstraint: a pass beyond the record buffers records up to two levels (one that was inserted before it could be judged, and the one it inserted)
  unsigned long long con_kept_deep = 0, con_pruned_deep = 0;
  int con_deep_levels = 0;
  auto con_collect_deep = [&](int inserted_level) {
    vsrmc_constraint_info newest;
    if (!w_con || vsrmc_checker_constraint_info(c, 0, &newest) != 0) return;
    for (int lvl = con_seen_level + 1; lvl <= newest.level; lvl++) {
      vsrmc_constraint_info ci;
      if (vsrmc_checker_constraint_info(c, lvl, &ci) != 0) continue;
      con_seen_level = lvl;
      con_pruned_total += (unsigned long long)ci.pruned;
      con_kept_deep += (unsigned long long)ci.kept;
      con_pruned_deep += (unsigned long long)ci.pruned;
      con_deep_levels++;
      for (size_t k = 0; k < con_inv_names.size() && con_hit < 0; k++)
        if (ci.pruned_count[k]) { con_hit = (int)k; con_hit_level = ci.level; con_hit_fp = ci.pruned_min_fp_k[k]; }
      if (lvl == inserted_level) con_info = ci;
      else if (json) std::printf("{\"filtered_level\": %d, \"kept\": %llu, \"pruned\": %llu}\n", lvl, (unsigned long long)ci.kept, (unsigned long long)ci.pruned);
      else std::printf("Filtered(%d): %llu in the model, %llu out of model (regenerated and judged before it was expanded).\n", lvl, (unsigned long long)ci.kept, (unsigned long long)ci.pruned);
    }
  };
  // -actionConstraint: the figures of every step taken under it, the run's totals
  unsigned long long act_blocked_total = 0, act_blocked_by[16] = {0}, act_blocked_violating = 0;
  int act_seen_level = 0;
  vsrmc_action_constraint_info act_info;
  std::memset(&act_info, 0, sizeof(act_info));
  auto act_collect = [&]() -> bool {                              // true: a step not seen before (act_info holds it)
    if (!s_act || vsrmc_checker_action_constraint_info(c, 0, &act_info) != 0 || act_info.level <= act_seen_level) return false;
    act_seen_level = act_info.level;
    act_blocked_total += (unsigned long long)act_info.blocked;
    act_blocked_violating += (unsigned long long)act_info.blocked_violating;
    for (int a2 = 0; a2 < 16; a2++) act_blocked_by[a2] += (unsigned long long)act_info.blocked_act[a2];
    return true;
  };
  // -deepActionConstraint: the gated passes into a level beyond the record buffers (an inserted level joins the totals; a probed one is printed only — the pass
  // that inserts it counts it)
  vsrmc_action_constraint_deep_info act_deep;
  std::memset(&act_deep, 0, sizeof(act_deep));
  auto act_collect_deep = [&](int level, bool inserted) -> bool {
    if (!s_act || !deep_action || vsrmc_checker_action_constraint_deep_info(c, level, &act_deep) != 0) return false;
    if (inserted) {
      act_blocked_total += (unsigned long long)act_deep.blocked;
      act_blocked_violating += (unsigned long long)act_deep.blocked_violating;
      for (int a2 = 0; a2 < 16; a2++) act_blocked_by[a2] += (unsigned long long)act_deep.blocked_act[a2];
    }
    return true;
  };
  unsigned long long cov[16] = {0};
  uint64_t viol_level = 0, viol_index = 0;
  int depth = info.level + info.reserved0;                        // (a recovered deep search: the levels beyond the stored one)
  struct Row { int level; unsigned long long n_new, generated, deadlocks; };
  std::vector<Row> rows;                                          // what -audit compares
  auto checkpoint_now = [&](int level) {
    if (chk_file.empty() || std::chrono::duration<double>(std::chrono::steady_clock::now() - t_chk).count() < 60.0 * chk_minutes) return;
    if (vsrmc_checker_save(c, chk_file.c_str()) != 0) std::printf("Warning: %s\n", vsrmc_last_error());
    else std::printf("Checkpointing of run %s completed (level %d).\n", chk_file.c_str(), level);
    t_chk = std::chrono::steady_clock::now();
  };
  // terminal states (-checkDeadlock / -terminalReport): the newest stored level is scanned before it is expanded
  struct TermRow { int level; unsigned long long n_terminal, n_unsettled; };
  std::vector<TermRow> term_rows;
  vsrmc_terminal_info ti;
  std::memset(&ti, 0, sizeof(ti));
  int last_scanned = 0, uns_level = 0, levels_scanned = 0;
  uint64_t uns_fp = 0;
  unsigned long long unlisted_levels = 0, unlisted_deadlocks = 0;
  bool scanned_this_step = false;
  // -deepTerminal: the levels the terminal attachment has examined (level -> its row; a level examined as the probed level and, one pass later, as a scanned
  // level has ONE row: the scanned one replaces the probed one) and the shallowest terminal state a pass found for -checkDeadlock
  struct DeepTermRow { int kind, exact; unsigned long long n_states, n_terminal, n_unsettled; uint64_t min_fp, min_fp_unsettled; };
  std::map<int, DeepTermRow> dterm_rows;
  std::vector<std::pair<int, int>> dterm_seen;
  struct DeepDead { int level = 0, probed = 0; unsigned long long n = 0; } deep_dead;
  auto dterm_scanned = [&](int level) { const auto it = dterm_rows.find(level); return it != dterm_rows.end() && it->second.kind != 2; };
  static const char* const DTERM_KIND[3] = {"regenerated", "inserted", "probed"};
  auto dterm_collect = [&]() -> int {                              // the (level, probed) pairs the last pass examined for the first time
    uint64_t n = 0;
    if (vsrmc_checker_deep_terminal_levels(c, nullptr, nullptr, 0, &n) != 0) return -1;
    std::vector<int32_t> lv((size_t)n + 1), pr((size_t)n + 1);
    if (vsrmc_checker_deep_terminal_levels(c, lv.data(), pr.data(), n, &n) != 0) return -1;
    for (uint64_t i = 0; i < n; i++) {
      const std::pair<int, int> key((int)lv[i], (int)pr[i]);
      if (std::find(dterm_seen.begin(), dterm_seen.end(), key) != dterm_seen.end()) continue;
      dterm_seen.push_back(key);
      vsrmc_deep_terminal_info di;
      if (vsrmc_checker_deep_terminal_result(c, lv[i], pr[i], &di) != 0) return -1;
      dterm_rows[di.level] = DeepTermRow{di.kind, di.exact, (unsigned long long)di.n_states, (unsigned long long)di.n_terminal, (unsigned long long)di.n_unsettled, di.min_fp, di.min_fp_unsettled};
      if (json)
        std::printf("{\"level\": %d, \"stored\": false, \"kind\": \"%s\", \"exact\": %s, \"terminal\": %llu, \"unsettled\": %llu}\n", di.level, DTERM_KIND[di.kind],
                    di.exact ? "true" : "false", (unsigned long long)di.n_terminal, (unsigned long long)di.n_unsettled);
      if (di.n_terminal && (!deep_dead.level || di.level < deep_dead.level)) { deep_dead.level = di.level; deep_dead.probed = pr[i]; deep_dead.n = (unsigned long long)di.n_terminal; }
    }
    return 0;
  };
  std::vector<std::pair<int, unsigned long long>> expanded_unstored;   // (level, deadlocks) of the levels that were expanded from the seen-set alone
  int bt_probed = -1, bt_unsettled = 0;                            // print_behaviour_to: >= 0 = the behaviour comes from the terminal attachment (1: a probed level)
  auto scan_newest = [&]() -> int {                               // 0, or the error of the scan; a level without records is counted, not listed
    scanned_this_step = false;
    vsrmc_level_info st;
    if (vsrmc_checker_status(c, &st) != 0) return -1;
    if (st.reserved0 != 0 || st.level == last_scanned || st.n_new == 0) return 0;
    if (deep_terminal && dterm_scanned(st.level)) { last_scanned = st.level; return 0; }   // (scanned by a descent, then re-based onto: reported once)
    const int32_t r = vsrmc_checker_terminal_scan(c, &ti);
    if (r == VSRMC_E_STATE) return 0;
    if (r != 0) return r;
    last_scanned = ti.level;
    levels_scanned++;
    scanned_this_step = true;
    dterm_rows.erase(ti.level);                                   // (examined earlier as a probed level, stored since — after a re-basing: the stored scan is the level's one row)
    if (ti.n_terminal) term_rows.push_back(TermRow{ti.level, (unsigned long long)ti.n_terminal, (unsigned long long)ti.n_unsettled});
    if (ti.n_unsettled && !uns_level) { uns_level = ti.level; uns_fp = ti.min_fp_unsettled; }
    return 0;
  };
  // -deepPredicates: the (level, as the probed level) pairs the attached programs have examined.  A level that a descent scanned and that the search then
  // re-based onto is a stored level from there on: it is not scanned, and not reported, a second time
  std::vector<std::pair<int, int>> deep_seen;
  auto deep_scanned = [&](int level) { return std::find(deep_seen.begin(), deep_seen.end(), std::make_pair(level, 0)) != deep_seen.end(); };
  // state predicates: the newest stored level is scanned where the terminal scan scans it
  struct WhereRow { int level; unsigned long long n_states; unsigned long long count[8]; };
  std::vector<WhereRow> where_rows;
  vsrmc_where_info wi_all, wi_query;
  std::memset(&wi_all, 0, sizeof(wi_all));
  std::memset(&wi_query, 0, sizeof(wi_query));
  int where_last = 0, where_hit = -1;
  unsigned long long where_unexamined = 0;
  bool where_scanned_this_step = false;
  auto where_newest = [&]() -> int {
    where_scanned_this_step = false;
    vsrmc_level_info st;
    if (vsrmc_checker_status(c, &st) != 0) return -1;
    if (st.reserved0 != 0 || st.level == where_last || st.n_new == 0) return 0;
    if (deep_predicates && (w_query || where_report) && deep_scanned(st.level)) { where_last = st.level; return 0; }
    int32_t r = 0;
    if (w_all && where_report && (r = vsrmc_checker_where_scan(c, w_all, &wi_all)) != 0) return r == VSRMC_E_STATE ? 0 : r;
    if (w_query && (r = vsrmc_checker_where_scan(c, w_query, &wi_query)) != 0) return r == VSRMC_E_STATE ? 0 : r;
    where_last = st.level;
    where_scanned_this_step = true;
    if (where_report) {
      WhereRow row{wi_all.level, (unsigned long long)wi_all.n_states, {0}};
      for (size_t k = 0; k < where_names.size(); k++) row.count[k] = (unsigned long long)wi_all.count[k];
      where_rows.push_back(row);
    }
    if (w_query) {                                                // an invariant's violation is reported before a reachability hit of the same level
      for (size_t k = n_reach; k < query_names.size() && where_hit < 0; k++)
        if (wi_query.count[k]) where_hit = (int)k;
      for (size_t k = 0; k < n_reach && where_hit < 0; k++)
        if (wi_query.count[k]) where_hit = (int)k;
    }
    return 0;
  };
  // step predicates: every transition out of the newest stored level, where the state predicates scan it
  struct StepRow { int level; unsigned long long n_states, n_pairs, n_err; unsigned long long count[8]; };
  std::vector<StepRow> step_rows;
  vsrmc_step_info si_all, si_query;
  std::memset(&si_all, 0, sizeof(si_all));
  std::memset(&si_query, 0, sizeof(si_query));
  int step_last = 0, step_hit = -1;
  unsigned long long step_unexamined = 0;
  bool step_scanned_this_step = false;
  auto step_newest = [&]() -> int {
    step_scanned_this_step = false;
    vsrmc_level_info st;
    if (vsrmc_checker_status(c, &st) != 0) return -1;
    if (st.reserved0 != 0 || st.level == step_last || st.n_new == 0) return 0;
    if (deep_predicates && (s_query || step_report) && deep_scanned(st.level)) { step_last = st.level; return 0; }
    int32_t r = 0;
    if (s_all && step_report && (r = vsrmc_checker_step_scan(c, s_all, &si_all)) != 0) return r == VSRMC_E_STATE ? 0 : r;
    if (s_query && (r = vsrmc_checker_step_scan(c, s_query, &si_query)) != 0) return r == VSRMC_E_STATE ? 0 : r;   // (last: vsrmc_checker_step_successor follows it)
    step_last = st.level;
    step_scanned_this_step = true;
    if (step_report) {
      StepRow row{si_all.level, (unsigned long long)si_all.n_states, (unsigned long long)si_all.n_pairs, (unsigned long long)si_all.n_err, {0}};
      for (size_t k = 0; k < step_names.size(); k++) row.count[k] = (unsigned long long)si_all.count[k];
      step_rows.push_back(row);
    }
    if (s_query) {                                                // an action property's violation is reported before a reachability hit of the same level
      for (size_t k = n_step_reach; k < step_query_names.size() && step_hit < 0; k++)
        if (si_query.count[k]) step_hit = (int)k;
      for (size_t k = 0; k < n_step_reach && step_hit < 0; k++)
        if (si_query.count[k]) step_hit = (int)k;
    }
    return 0;
  };
  auto step_json_of = [&]() {
    std::string j = "\"steps\": {\"pairs\": " + std::to_string((unsigned long long)si_all.n_pairs) + ", \"errors\": " + std::to_string((unsigned long long)si_all.n_err) +
                    ", \"count\": {";
    for (size_t k = 0; k < step_names.size(); k++) j += (k ? ", \"" : "\"") + step_names[k] + "\": " + std::to_string((unsigned long long)si_all.count[k]);
    return j + "}}";
  };
  // Init .. the level-`level` state `fp`, printed the way a violation is; `stutter`: a last line "State k+1: Stuttering"; step_index / step_ordinal: one
  // more state, the successor that instance of that state leads to (the pair a step predicate stopped at)
  const char* behaviour_header = "Error: The behavior up to this point is:";
  auto print_behaviour_to = [&](int level, uint64_t fp, bool stutter, bool with_step = false, uint64_t step_index = 0, uint32_t step_ordinal = 0) -> bool {
    uint64_t cap_w = ((uint64_t)level + 3) * (uint64_t)lay.max_record_words, n_states = 0;
    std::vector<uint64_t> words(cap_w), off((size_t)level + 3);
    std::vector<int32_t> acts((size_t)level + 3);
    if ((bt_probed >= 0 ? vsrmc_checker_deep_terminal_witness(c, level, bt_probed, bt_unsettled, words.data(), cap_w, off.data(), acts.data(), off.size() - 1, &n_states)
                        : vsrmc_checker_trace_fp(c, level, fp, words.data(), cap_w, off.data(), acts.data(), off.size() - 1, &n_states)) != 0) {
      std::printf("Error: %s\n", vsrmc_last_error());
      return false;
    }
    if (with_step) {
      uint64_t len = 0;
      int32_t act = 0;
      if (n_states == 0 ||
          vsrmc_checker_step_successor(c, step_index, step_ordinal, &words[off[n_states - 1]], off[n_states] - off[n_states - 1], &words[off[n_states]],
                                       cap_w - off[n_states], &len, &act) != 0) {
        std::printf("Error: %s\n", vsrmc_last_error());
        return false;
      }
      acts[n_states] = act;
      off[n_states + 1] = off[n_states] + len;
      n_states++;
    }
    std::printf("%s\n", behaviour_header);
    for (uint64_t t = 0; t < n_states; t++) {
      int64_t need = 0;
      vsrmc_model_format_state(m, &words[off[t]], nullptr, 0, &need);
      std::string buf((size_t)need, '\0');
      vsrmc_model_format_state(m, &words[off[t]], &buf[0], need, &need);
      std::printf("State %llu: <%s>\n%s\n\n", (unsigned long long)(t + 1), vsrmc_action_name(acts[t]), buf.c_str());
    }
    if (stutter) std::printf("State %llu: Stuttering\n", (unsigned long long)(n_states + 1));
    if (!dump_trace_file.empty()) {
      if (write_trace_expression(dump_trace_file, m, words, off, acts, n_states))
        std::printf("The counter-example was written to %s (TLA+ trace expression).\n", dump_trace_file.c_str());
      else
        std::printf("Warning: cannot write %s\n", dump_trace_file.c_str());
    }
    return true;
  };
  // -deepPredicates: the levels the last pass examined for the first time (vsrmc_checker_deep_levels): report rows, and the first hit of a query
  struct DeepHit { int level = 0, probed = 0, step = 0, k = -1, exact = 1; uint64_t fp = 0, count = 0, of = 0; } deep_hit;
  std::vector<int> virtual_levels;
  std::vector<int> deep_inexact;                                  // probed levels whose list of collected copies overflowed: their figures are lower bounds
  std::vector<WhereRow> where_probed_rows;
  std::vector<int> where_probed_exact;
  static const char* const DEEP_KIND[3] = {"regenerated", "inserted", "probed"};
  auto deep_collect = [&]() -> int {
    uint64_t n = 0;
    if (vsrmc_checker_deep_levels(c, nullptr, nullptr, 0, &n) != 0) return -1;
    std::vector<int32_t> lv((size_t)n + 1), pr((size_t)n + 1);
    if (vsrmc_checker_deep_levels(c, lv.data(), pr.data(), n, &n) != 0) return -1;
    for (uint64_t i = 0; i < n && deep_hit.k < 0; i++) {
      const std::pair<int, int> key(lv[i], pr[i]);
      if (std::find(deep_seen.begin(), deep_seen.end(), key) != deep_seen.end()) continue;
      deep_seen.push_back(key);
      vsrmc_deep_info di;
      vsrmc_where_info wi;
      vsrmc_step_info si;
      if (vsrmc_checker_deep_result(c, lv[i], pr[i], &di, &wi, &si) != 0) return -1;
      if (!di.exact) deep_inexact.push_back(di.level);
      std::string line;
      if (di.has_state && where_report) {
        WhereRow row{di.level, (unsigned long long)wi.n_states, {0}};
        for (size_t k = 0; k < where_names.size(); k++) row.count[k] = (unsigned long long)wi.count[k];
        if (di.kind == 2) { where_probed_rows.push_back(row); where_probed_exact.push_back(di.exact); }
        else where_rows.push_back(row);
        line += json ? ", \"where\": {" : "";
        for (size_t k = 0; k < where_names.size(); k++)
          line += json ? (k ? ", \"" : "\"") + where_names[k] + "\": " + std::to_string(row.count[k]) : ", " + where_names[k] + " " + std::to_string(row.count[k]);
        line += json ? "}" : "";
      }
      if (di.has_step && step_report) {
        StepRow row{di.level, (unsigned long long)si.n_states, (unsigned long long)si.n_pairs, (unsigned long long)si.n_err, {0}};
        for (size_t k = 0; k < step_names.size(); k++) row.count[k] = (unsigned long long)si.count[k];
        step_rows.push_back(row);
        line += json ? ", \"steps\": {\"pairs\": " + std::to_string(row.n_pairs) + ", \"errors\": " + std::to_string(row.n_err) + ", \"count\": {"
                     : "; " + std::to_string(row.n_pairs) + " pairs, " + std::to_string(row.n_err) + " errors";
        for (size_t k = 0; k < step_names.size(); k++)
          line += json ? (k ? ", \"" : "\"") + step_names[k] + "\": " + std::to_string(row.count[k]) : ", " + step_names[k] + " " + std::to_string(row.count[k]);
        line += json ? "}}" : "";
      }
      if (!line.empty()) {
        if (json) std::printf("{\"level\": %d, \"stored\": false, \"kind\": \"%s\", \"exact\": %s%s}\n", di.level, DEEP_KIND[di.kind], di.exact ? "true" : "false", line.c_str());
        else std::printf("Examined(%d, %s%s)%s\n", di.level, DEEP_KIND[di.kind], di.exact ? "" : ", lower bounds", line.c_str());
      }
      // a query: an invariant's violation before a reachability hit, state predicates before step predicates, as on a stored level
      if (di.has_state && w_query) {
        int hit = -1;
        for (size_t k = n_reach; k < query_names.size() && hit < 0; k++) if (wi.count[k]) hit = (int)k;
        for (size_t k = 0; k < n_reach && hit < 0; k++) if (wi.count[k]) hit = (int)k;
        if (hit >= 0) { deep_hit.level = di.level; deep_hit.probed = di.kind == 2; deep_hit.step = 0; deep_hit.k = hit; deep_hit.exact = di.exact; deep_hit.fp = wi.min_fp[hit]; deep_hit.count = wi.count[hit]; deep_hit.of = wi.n_states; }
      }
      if (deep_hit.k < 0 && di.has_step && s_query) {
        int hit = -1;
        for (size_t k = n_step_reach; k < step_query_names.size() && hit < 0; k++) if (si.count[k]) hit = (int)k;
        for (size_t k = 0; k < n_step_reach && hit < 0; k++) if (si.count[k]) hit = (int)k;
        if (hit >= 0) { deep_hit.level = di.level; deep_hit.probed = 0; deep_hit.step = 1; deep_hit.k = hit; deep_hit.fp = si.min_fp[hit]; deep_hit.count = si.count[hit]; deep_hit.of = si.n_pairs; }
      }
    }
    return 0;
  };
  while (depth < max_depth) {
    if ((probe2_at > 0 && depth + 1 == probe2_at) || (probe3_at > 0 && depth + 1 == probe3_at)) {
      const int nv = probe3_at > 0 && depth + 1 == probe3_at ? 2 : 1;        // virtual levels before the probed one
      vsrmc_level_info li[3];
      rc = nv == 2 ? vsrmc_checker_probe3(c, &li[0], &li[1], &li[2]) : vsrmc_checker_probe2(c, &li[0], &li[1]);
      if (rc != 0) break;
      double dtp = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      for (int k = 0; k <= nv && !probed_violation; k++) {
        const vsrmc_level_info& x = li[k];
        if (x.level == 0) break;
        if (k < nv) {
          std::printf("Virtual(%d): %llu states generated, %llu distinct states found, %llu states in the level (not stored). (%.2f s)\n", x.level,
                      (unsigned long long)x.total_generated, (unsigned long long)x.distinct, (unsigned long long)x.n_new, dtp);
          info.distinct = x.distinct;
          info.n_new = x.n_new;
        } else {
          std::printf("Probe(%d): %llu states generated from %llu states, %llu violating successors seen. (%.2f s)\n", x.level,
                      (unsigned long long)x.generated, (unsigned long long)x.frontier, (unsigned long long)x.pending, dtp);
        }
        info.total_generated = x.total_generated;
        depth = x.level;
        if (x.viol_mask) {
          probed_violation = true;
          info.viol_mask = x.viol_mask;
          viol_level = (uint64_t)x.level;
        } else if (k == nv) {
          std::printf("No violation up to level %d; the search is incomplete beyond it.\n", x.level);
        }
      }
      break;
    }
    // the automatic level scheme: an ordinary level while the next one is predicted to fit the record buffers, else one more level through
    // the seen-set alone (vsrmc_checker_deepen: inserted, counted and checked, its records regenerated when needed) and a probe of the one after
    int32_t what = 0, room = 0;
    vsrmc_level_info probed;
    rc = vsrmc_checker_room(c, &room);                            // grows the seen-set while the device has the memory
    if (rc != 0) break;
    if (room == 1 && !json) std::printf("The seen-set was re-hashed into twice the slots.\n");
    if (room == 2) { incomplete = true; break; }
    if (check_deadlock || terminal_report) {
      rc = scan_newest();
      if (rc != 0) break;
      if (check_deadlock && scanned_this_step && ti.n_terminal) { deadlocked = true; break; }
    }
    if (w_all) {
      rc = where_newest();
      if (rc != 0) break;
      if (where_hit >= 0) break;
    }
    if (s_all) {
      rc = step_newest();
      if (rc != 0) break;
      if (step_hit >= 0) break;
    }
    if (con_hit >= 0) break;                                      // (Init is out of model and violates a user's invariant)
    rc = vsrmc_checker_advance(c, &info, &probed, &what);
    if (rc != 0) break;
    if (what == 4) { con_no_room = true; con_reason = vsrmc_last_error(); break; }   // a constraint is attached and the next level does not fit
    if (what == 3) {                                              // no new level: the deep search was re-based (the levels shrink again)
      if (!json) std::printf("Re-based(%d): %llu states regenerated into the record buffers (%llu launches, %.2f s); stored levels from here on.\n", info.level,
                             (unsigned long long)info.n_new, (unsigned long long)info.pending, info.seconds);
      continue;
    }
    if (what == 2) {
      for (int a2 = 1; a2 < 16; a2++) cov[a2] += info.act_generated[a2];
      const double dtp = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (dump) { std::printf("Level %d is not stored (it does not fit the record buffers): -dump ends at level %d.\n", info.level, depth); std::fclose(dump); dump = nullptr; }
      con_info.level = 0;
      if (deep_constraint) con_collect_deep(info.n_new ? info.level : info.level + 1);   // (first: a level that was inserted unfiltered gets its Filtered line before the Virtual line of the level above it)
      const bool act_deep_new = act_collect_deep(info.n_new ? info.level : info.level + 1, true);   // (an empty level: the pass into it blocked what it blocked)
      if (info.n_new == 0 && !info.viol_mask) break;
      if (info.n_new) depth = info.level;
      if (info.n_new) rows.push_back(Row{info.level, (unsigned long long)info.n_new, (unsigned long long)info.generated, (unsigned long long)info.deadlocks});
      if (terminal_report && !scanned_this_step) expanded_unstored.push_back(std::make_pair(info.level - 1, (unsigned long long)info.deadlocks));   // the level this pass expanded has no records
      if (w_all && !deep_state) where_unexamined++;               // the level this pass inserted is never stored
      if (s_all && !deep_step) step_unexamined++;
      virtual_levels.push_back(info.level);
      if (json && deep_constraint)                                  // "filtered": false = the unfiltered figures of a level the next pass judges
        std::printf("{\"level\": %d, \"stored\": false, \"generated\": %llu, \"new\": %llu, \"distinct\": %llu, \"deadlocks\": %llu, \"launches\": %llu, \"filtered\": %s, \"kept\": %llu, "
                    "\"pruned\": %llu, \"seconds\": %.4f}\n", info.level, (unsigned long long)info.generated, (unsigned long long)info.n_new, (unsigned long long)info.distinct,
                    (unsigned long long)info.deadlocks, (unsigned long long)info.pending, con_info.level == info.level ? "true" : "false",
                    con_info.level == info.level ? (unsigned long long)con_info.kept : 0ull, con_info.level == info.level ? (unsigned long long)con_info.pruned : 0ull, dtp);
      else if (json && act_deep_new)
        std::printf("{\"level\": %d, \"stored\": false, \"generated\": %llu, \"new\": %llu, \"distinct\": %llu, \"deadlocks\": %llu, \"launches\": %llu, \"permitted\": %llu, "
                    "\"blocked\": %llu, \"seconds\": %.4f}\n", info.level, (unsigned long long)info.generated, (unsigned long long)info.n_new, (unsigned long long)info.distinct,
                    (unsigned long long)info.deadlocks, (unsigned long long)info.pending, (unsigned long long)act_deep.permitted, (unsigned long long)act_deep.blocked, dtp);
      else if (json)
        std::printf("{\"level\": %d, \"stored\": false, \"generated\": %llu, \"new\": %llu, \"distinct\": %llu, \"deadlocks\": %llu, \"launches\": %llu, \"seconds\": %.4f}\n",
                    info.level, (unsigned long long)info.generated, (unsigned long long)info.n_new, (unsigned long long)info.distinct,
                    (unsigned long long)info.deadlocks, (unsigned long long)info.pending, dtp);
      else if (deep_constraint && con_info.level == info.level)     // filtered sub-slice by sub-slice before it was counted: the in-model figures
      std::printf("Virtual(%d): %llu states generated, %llu distinct states found, %llu states in the level (not stored; %llu launches); %llu in the model, %llu out of model. (%.2f s)\n", info.level,
                  (unsigned long long)info.total_generated, (unsigned long long)info.distinct, (unsigned long long)info.n_new, (unsigned long long)info.pending,
                  (unsigned long long)con_info.kept, (unsigned long long)con_info.pruned, dtp);
      else if (deep_constraint)
      std::printf("Virtual(%d): %llu states generated, %llu distinct states found, %llu states in the level (not stored; %llu launches); not judged yet: the next pass filters it. (%.2f s)\n", info.level,
                  (unsigned long long)info.total_generated, (unsigned long long)info.distinct, (unsigned long long)info.n_new, (unsigned long long)info.pending, dtp);
      else if (act_deep_new)
      std::printf("Virtual(%d): %llu states generated, %llu distinct states found, %llu states in the level (not stored; %llu launches); %llu of %llu transitions were not taken. (%.2f s)\n",
                  info.level, (unsigned long long)info.total_generated, (unsigned long long)info.distinct, (unsigned long long)info.n_new, (unsigned long long)info.pending,
                  (unsigned long long)act_deep.blocked, (unsigned long long)act_deep.pairs, dtp);
      else
      std::printf("Virtual(%d): %llu states generated, %llu distinct states found, %llu states in the level (not stored; %llu launches). (%.2f s)\n", info.level,
                  (unsigned long long)info.total_generated, (unsigned long long)info.distinct, (unsigned long long)info.n_new, (unsigned long long)info.pending, dtp);
      // -deepTerminal: what this pass examined.  The shallowest level wins, a built-in violation before a deadlock within a level
      if (deep_terminal && dterm_collect() != 0) { rc = -1; break; }
      const bool dead_here = deep_terminal && check_deadlock && deep_dead.level != 0;
      if (info.viol_mask && !(dead_here && deep_dead.level < info.level)) { probed_violation = true; viol_level = (uint64_t)info.level; break; }
      if (info.viol_mask) { info.viol_mask = 0; deadlocked = true; break; }
      if (probed.level) {
        const bool act_prb = act_collect_deep(probed.level, false);
        if (json && act_prb)
          std::printf("{\"probed_level\": %d, \"generated\": %llu, \"from\": %llu, \"violating_successors\": %llu, \"blocked\": %llu, \"seconds\": %.4f}\n", probed.level,
                      (unsigned long long)probed.generated, (unsigned long long)probed.frontier, (unsigned long long)probed.pending, (unsigned long long)act_deep.blocked, dtp);
        else if (json)
          std::printf("{\"probed_level\": %d, \"generated\": %llu, \"from\": %llu, \"violating_successors\": %llu, \"seconds\": %.4f}\n", probed.level,
                      (unsigned long long)probed.generated, (unsigned long long)probed.frontier, (unsigned long long)probed.pending, dtp);
        else if (act_prb)
        std::printf("Probe(%d): %llu states generated from %llu states, %llu of them by transitions not taken, %llu violating successors seen. (%.2f s)\n", probed.level,
                    (unsigned long long)probed.generated, (unsigned long long)probed.frontier, (unsigned long long)act_deep.blocked, (unsigned long long)probed.pending, dtp);
        else
        std::printf("Probe(%d): %llu states generated from %llu states, %llu violating successors seen. (%.2f s)\n", probed.level,
                    (unsigned long long)probed.generated, (unsigned long long)probed.frontier, (unsigned long long)probed.pending, dtp);
        if (probed.viol_mask && !(dead_here && deep_dead.level < probed.level)) {
          probed_violation = true;
          info.viol_mask = probed.viol_mask;
          info.total_generated = probed.total_generated;
          viol_level = (uint64_t)probed.level;
          break;
        }
      }
      if (dead_here) { deadlocked = true; break; }
      if (con_hit >= 0) break;                                    // -invariant fails among the states this pass pruned
      if (info.n_new == 0) break;
      if (deep_predicates) {
        if (deep_collect() != 0) { rc = -1; break; }
        if (deep_hit.k >= 0) break;
      }
      checkpoint_now(info.level);
      continue;
    }
    if (rc != 0) break;
    for (int a2 = 1; a2 < 16; a2++) cov[a2] += info.act_generated[a2];
    if (info.n_new) depth = info.level;
    if (info.n_new) rows.push_back(Row{info.level, (unsigned long long)info.n_new, (unsigned long long)info.generated, (unsigned long long)info.deadlocks});
    double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::string where_json;                                       // (of the level this step expanded, like terminal / unsettled)
    if (json && where_report && where_scanned_this_step) {
      where_json = ", \"where\": {";
      for (size_t k = 0; k < where_names.size(); k++)
        where_json += (k ? ", \"" : "\"") + where_names[k] + "\": " + std::to_string((unsigned long long)wi_all.count[k]);
      where_json += "}";
    }
    if (json && step_report && step_scanned_this_step) where_json += ", " + step_json_of();
    const bool con_new = con_collect();                           // the level this step stored and filtered (none: the step found no new state)
    if (json && w_con)
      where_json += ", \"kept\": " + std::to_string(con_new ? (unsigned long long)con_info.kept : 0ull) + ", \"pruned\": " + std::to_string(con_new ? (unsigned long long)con_info.pruned : 0ull);
    const bool act_new = act_collect();                           // the step this call took under the action constraint
    if (json && s_act)
      where_json += ", \"permitted\": " + std::to_string(act_new ? (unsigned long long)act_info.permitted : 0ull) + ", \"blocked\": " + std::to_string(act_new ? (unsigned long long)act_info.blocked : 0ull);
    if (!json && act_new)
      std::printf("ActionConstraint(%d): %llu of %llu transitions were not taken, %llu taken, %llu new states.\n", act_info.level, (unsigned long long)act_info.blocked,
                  (unsigned long long)act_info.pairs, (unsigned long long)act_info.permitted, (unsigned long long)act_info.n_new);
    if (json && scanned_this_step)                                // (terminal / unsettled: of the level this step expanded, like deadlocks)
      std::printf("{\"level\": %d, \"generated\": %llu, \"new\": %llu, \"distinct\": %llu, \"deadlocks\": %llu, \"terminal\": %llu, \"unsettled\": %llu%s, \"seconds\": %.4f}\n",
                  info.level, (unsigned long long)info.generated, (unsigned long long)info.n_new, (unsigned long long)info.distinct,
                  (unsigned long long)info.deadlocks, (unsigned long long)ti.n_terminal, (unsigned long long)ti.n_unsettled, where_json.c_str(), dt);
    else if (json && !where_json.empty())
      std::printf("{\"level\": %d, \"generated\": %llu, \"new\": %llu, \"distinct\": %llu, \"deadlocks\": %llu%s, \"seconds\": %.4f}\n",
                  info.level, (unsigned long long)info.generated, (unsigned long long)info.n_new, (unsigned long long)info.distinct,
                  (unsigned long long)info.deadlocks, where_json.c_str(), dt);
    else if (json)
      std::printf("{\"level\": %d, \"generated\": %llu, \"new\": %llu, \"distinct\": %llu, \"deadlocks\": %llu, \"seconds\": %.4f}\n",
                  info.level, (unsigned long long)info.generated, (unsigned long long)info.n_new, (unsigned long long)info.distinct,
                  (unsigned long long)info.deadlocks, dt);
    else if (info.n_new)
      std::printf("Progress(%d): %llu states generated, %llu distinct states found, %llu states left on queue. (%.2f s)\n", info.level,
                  (unsigned long long)info.total_generated, (unsigned long long)info.distinct, (unsigned long long)info.n_new, dt);
    if (!dump_level(info.n_new)) { rc = -1; break; }
    if (info.viol_mask) { violated = true; viol_level = (uint64_t)(w_con && con_new ? con_info.level : info.level); viol_index = info.viol_index; break; }
    if (con_hit >= 0) break;
    if (check_deadlock && info.deadlocks) { deadlocked = true; break; }
    if (info.n_new == 0) break;
    checkpoint_now(info.level);
  }
  // the report covers the newest stored level too when the loop ended before expanding it (-maxDepth, a violation, a full seen-set); an exhausted search's
  // last level is empty and a level already scanned is not scanned again (scan_newest)
  if (terminal_report && rc == 0 && !deadlocked) rc = scan_newest();
  if (deep_predicates && rc == 0) {                               // which never-stored levels stayed unexamined (by number): those of a run that ends after the virtual level
    for (int lvl : virtual_levels) {
      const bool scanned = std::find(deep_seen.begin(), deep_seen.end(), std::make_pair(lvl, 0)) != deep_seen.end();
      const bool probed = std::find(deep_seen.begin(), deep_seen.end(), std::make_pair(lvl, 1)) != deep_seen.end();
      if (deep_state && !scanned && !probed) where_unexamined++;
      if (deep_step && !scanned) step_unexamined++;
      if ((deep_state && !scanned && !probed) || (deep_step && !scanned)) std::printf("Level %d was never stored and no later pass regenerated it: not examined.\n", lvl);
    }
  }
  if (s_all && rc == 0 && step_hit < 0 && where_hit < 0 && deep_hit.k < 0 && !deadlocked && !violated && !probed_violation) {
    rc = step_newest();
    if (json && step_report && step_scanned_this_step && rc == 0)       // the newest level was not expanded: a line of its own
      std::printf("{\"level\": %d, \"expanded\": false, %s}\n", si_all.level, step_json_of().c_str());
  }
  if (w_all && rc == 0 && where_hit < 0 && deep_hit.k < 0 && !deadlocked) {
    rc = where_newest();
    if (json && where_report && where_scanned_this_step && rc == 0) {   // the newest level was not expanded: a line of its own
      std::printf("{\"level\": %d, \"expanded\": false, \"where\": {", wi_all.level);
      for (size_t k = 0; k < where_names.size(); k++) std::printf("%s\"%s\": %llu", k ? ", " : "", where_names[k].c_str(), (unsigned long long)wi_all.count[k]);
      std::printf("}}\n");
    }
  }
  double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  int exit_code = 0;
  if (rc != 0) {
    std::printf("Error: %s\n", vsrmc_last_error());
    exit_code = rc == VSRMC_E_EVAL ? 12 : 1;
  } else if (violated || probed_violation) {
    const char* const* names = INVARIANT_NAMES;
    for (int b = 0; b < 5; b++)
      if (info.viol_mask & (1 << b)) std::printf("Error: Invariant %s is violated.\n", names[b]);
    std::printf("Error: The behavior up to this point is:\n");
    uint64_t cap_w = (viol_level + 2) * (uint64_t)lay.max_record_words, n_states = 0;
    std::vector<uint64_t> words(cap_w), off(viol_level + 2);
    std::vector<int32_t> acts(viol_level + 2);
    if ((probed_violation ? vsrmc_checker_probe_trace(c, words.data(), cap_w, off.data(), acts.data(), off.size(), &n_states)
         : w_con          ? vsrmc_checker_trace_fp(c, (int32_t)viol_level, info.viol_fp, words.data(), cap_w, off.data(), acts.data(), off.size(), &n_states)   // (the violator may be out of model)
                          : vsrmc_checker_trace(c, (int32_t)viol_level, viol_index, words.data(), cap_w, off.data(), acts.data(), off.size(),
                                                &n_states)) != 0) {
      std::printf("Error: %s\n", vsrmc_last_error());
      exit_code = 1;
    } else {
      for (uint64_t t = 0; t < n_states; t++) {
        int64_t need = 0;
        vsrmc_model_format_state(m, &words[off[t]], nullptr, 0, &need);
        std::string buf((size_t)need, '\0');
        vsrmc_model_format_state(m, &words[off[t]], &buf[0], need, &need);
        std::printf("State %llu: <%s>\n%s\n\n", (unsigned long long)(t + 1), vsrmc_action_name(acts[t]), buf.c_str());
      }
      if (!dump_trace_file.empty()) {
        if (write_trace_expression(dump_trace_file, m, words, off, acts, n_states))
          std::printf("The counter-example was written to %s (TLA+ trace expression).\n", dump_trace_file.c_str());
        else
          std::printf("Warning: cannot write %s\n", dump_trace_file.c_str());
      }
      exit_code = 12;   // TLC's exit code for a safety violation
    }
  } else if (deep_hit.k >= 0) {                                 // -deepPredicates: a hit beyond the record buffers, with the messages and exit codes of the stored path
    const bool inv = deep_hit.step ? deep_hit.k >= (int)n_step_reach : deep_hit.k >= (int)n_reach;
    const char* name = deep_hit.step ? step_query_names[deep_hit.k].c_str() : query_names[deep_hit.k].c_str();
    if (inv) std::printf(deep_hit.step ? "Error: Action property %s is violated.\n" : "Error: Invariant %s is violated.\n", name);
    else if (deep_hit.step)
      std::printf("Step satisfying %s found at depth %d (%llu of the level's %llu transitions satisfy it).\n", name, deep_hit.level, (unsigned long long)deep_hit.count,
                  (unsigned long long)deep_hit.of);
    else if (deep_hit.probed)
      std::printf("State satisfying %s found at depth %d (%s%llu states of the probed level satisfy it).\n", name, deep_hit.level, deep_hit.exact ? "" : "at least ",
                  (unsigned long long)deep_hit.count);
    else
      std::printf("State satisfying %s found at depth %d (%llu of the level's %llu states satisfy it).\n", name, deep_hit.level, (unsigned long long)deep_hit.count,
                  (unsigned long long)deep_hit.of);
    const uint64_t cap_w = ((uint64_t)deep_hit.level + 3) * (uint64_t)lay.max_record_words;
    uint64_t n_states = 0;
    std::vector<uint64_t> words(cap_w), off((size_t)deep_hit.level + 4);
    std::vector<int32_t> acts((size_t)deep_hit.level + 4);
    if (vsrmc_checker_deep_witness(c, deep_hit.level, deep_hit.step ? 1 : deep_hit.probed ? 2 : 0, deep_hit.k, words.data(), cap_w, off.data(), acts.data(), off.size() - 1,
                                   &n_states) != 0) {
      std::printf("Error: %s\n", vsrmc_last_error());
      exit_code = 1;
    } else {
      if (json && deep_hit.step)
        std::printf("{\"%s\": \"%s\", \"level\": %d, \"parent_fp\": \"%016llx\", \"action\": \"%s\", \"pairs\": %llu}\n", inv ? "action_property_violated" : "step_reached", name,
                    deep_hit.level, (unsigned long long)deep_hit.fp, vsrmc_action_name(acts[n_states - 1]), (unsigned long long)deep_hit.count);
      std::printf("%s\n", inv ? "Error: The behavior up to this point is:" : "The behavior up to this point is:");
      for (uint64_t t = 0; t < n_states; t++) {
        int64_t need = 0;
        vsrmc_model_format_state(m, &words[off[t]], nullptr, 0, &need);
        std::string buf((size_t)need, '\0');
        vsrmc_model_format_state(m, &words[off[t]], &buf[0], need, &need);
        std::printf("State %llu: <%s>\n%s\n\n", (unsigned long long)(t + 1), vsrmc_action_name(acts[t]), buf.c_str());
      }
      if (deep_hit.step) std::printf("The last step is %s of State %d.\n", vsrmc_action_name(acts[n_states - 1]), deep_hit.level);
      if (!dump_trace_file.empty()) {
        if (write_trace_expression(dump_trace_file, m, words, off, acts, n_states))
          std::printf("The counter-example was written to %s (TLA+ trace expression).\n", dump_trace_file.c_str());
        else
          std::printf("Warning: cannot write %s\n", dump_trace_file.c_str());
      }
      exit_code = inv ? 12 : 0;
    }
  } else if (con_hit >= 0) {                                    // a user's invariant that fails on a state the constraint pruned
    std::printf("Error: Invariant %s is violated (by a state of level %d that is outside CONSTRAINT %s).\n", con_inv_names[con_hit].c_str(), con_hit_level, constraint_arg.c_str());
    exit_code = print_behaviour_to(con_hit_level, con_hit_fp, false) ? 12 : 1;
  } else if (where_hit >= (int)n_reach) {                       // a user's invariant: reported like a built-in one
    std::printf("Error: Invariant %s is violated.\n", query_names[where_hit].c_str());
    exit_code = print_behaviour_to(wi_query.level, wi_query.min_fp[where_hit], false) ? 12 : 1;
  } else if (where_hit >= 0) {
    std::printf("State satisfying %s found at depth %d (%llu of the level's %llu states satisfy it).\n", query_names[where_hit].c_str(), wi_query.level,
                (unsigned long long)wi_query.count[where_hit], (unsigned long long)wi_query.n_states);
    behaviour_header = "The behavior up to this point is:";
    exit_code = print_behaviour_to(wi_query.level, wi_query.min_fp[where_hit], false) ? 0 : 1;
  } else if (step_hit >= 0) {
    const bool inv = step_hit >= (int)n_step_reach;
    const char* name = step_query_names[step_hit].c_str();
    if (inv) std::printf("Error: Action property %s is violated.\n", name);
    else {
      std::printf("Step satisfying %s found at depth %d (%llu of the level's %llu transitions satisfy it).\n", name, si_query.level,
                  (unsigned long long)si_query.count[step_hit], (unsigned long long)si_query.n_pairs);
      behaviour_header = "The behavior up to this point is:";
    }
    if (json)
      std::printf("{\"%s\": \"%s\", \"level\": %d, \"parent_fp\": \"%016llx\", \"ordinal\": %u, \"action\": \"%s\", \"pairs\": %llu}\n", inv ? "action_property_violated" : "step_reached",
                  name, si_query.level, (unsigned long long)si_query.min_fp[step_hit], si_query.min_ordinal[step_hit], vsrmc_action_name(si_query.min_action[step_hit]),
                  (unsigned long long)si_query.count[step_hit]);
    const bool ok = print_behaviour_to(si_query.level, si_query.min_fp[step_hit], false, true, si_query.min_index[step_hit], si_query.min_ordinal[step_hit]);
    if (ok) std::printf("The last step is %s of State %d.\n", vsrmc_action_name(si_query.min_action[step_hit]), si_query.level);
    exit_code = ok ? (inv ? 12 : 0) : 1;
  } else if (deadlocked && deep_dead.level) {                    // -deepTerminal: found beyond the record buffers, by the terminal attachment
    std::printf("Error: Deadlock reached (%s%llu state(s) of level %d have no successor).\n", dterm_rows[deep_dead.level].exact ? "" : "at least ", deep_dead.n, deep_dead.level);
    bt_probed = deep_dead.probed;
    exit_code = print_behaviour_to(deep_dead.level, dterm_rows[deep_dead.level].min_fp, false) ? 11 : 1;
    bt_probed = -1;
  } else if (deadlocked && scanned_this_step && ti.n_terminal) {  // found by the scan, before the level was expanded: there is a behaviour to show
    std::printf("Error: Deadlock reached (%llu state(s) of level %d have no successor).\n", (unsigned long long)ti.n_terminal, ti.level);
    exit_code = print_behaviour_to(ti.level, ti.min_fp, false) ? 11 : 1;
  } else if (deadlocked) {
    std::printf("Error: Deadlock reached (%llu state(s) of level %d have no successor).\n", (unsigned long long)info.deadlocks, info.level - 1);
    exit_code = 11;
  } else if (incomplete) {
    std::printf("Model checking INCOMPLETE at depth %d: the seen-set is more than 85 %% full and the device has no memory for a larger one "
                "(no error has been found up to that depth).\n", depth);
    exit_code = 4;
  } else if (con_no_room) {
    std::printf("Model checking INCOMPLETE at depth %d: %s.\n", depth, con_reason.c_str());
    exit_code = 4;
  } else if (info.n_new == 0) {
    std::printf("Model checking completed. No error has been found.\n");
  }
  if (w_con && rc == 0)
    std::printf("CONSTRAINT %s: %llu states were out of model and not explored; the distinct states below are the in-model ones.\n", constraint_arg.c_str(), con_pruned_total);
  if (w_con && deep_constraint && rc == 0)
    std::printf("CONSTRAINT %s, levels beyond the record buffers included: %llu in-model states kept and %llu pruned in the %d level(s) filtered there.\n", constraint_arg.c_str(),
                con_kept_deep, con_pruned_deep, con_deep_levels);
  if (s_act && rc == 0) {
    std::string per;
    for (int a2 = 0; a2 < 16; a2++)
      if (act_blocked_by[a2]) per += std::string(per.empty() ? "" : ", ") + vsrmc_action_name(a2) + ": " + std::to_string(act_blocked_by[a2]);
    std::printf("ACTION_CONSTRAINT %s: %llu transitions were not taken (per action: %s); %llu of their successors fail a built-in invariant (counted, not reported).\n",
                action_constraint_arg.c_str(), act_blocked_total, per.empty() ? "none" : per.c_str(), act_blocked_violating);
  }
  if (terminal_report && rc == 0) {
    unsigned long long n_term = 0, n_uns = 0;
    int dterm_through = 0, dterm_uns_level = 0, dterm_inexact = 0;
    for (const auto& kv : dterm_rows) {                            // -deepTerminal: the levels beyond the record buffers join the stored ones, in level order
      levels_scanned++;
      dterm_through = std::max(dterm_through, kv.first);
      if (!kv.second.exact) dterm_inexact++;
      if (kv.second.n_terminal) term_rows.push_back(TermRow{kv.first, kv.second.n_terminal, kv.second.n_unsettled});
      if (kv.second.n_unsettled && !dterm_uns_level) dterm_uns_level = kv.first;
    }
    std::sort(term_rows.begin(), term_rows.end(), [](const TermRow& a, const TermRow& b) { return a.level < b.level; });
    for (const auto& e : expanded_unstored)
      if (!dterm_scanned(e.first)) { unlisted_levels++; unlisted_deadlocks += e.second; }
    for (const TermRow& r : term_rows) { n_term += r.n_terminal; n_uns += r.n_unsettled; }
    std::printf("Terminal report: %llu terminal states in %zu of %d scanned levels", n_term, term_rows.size(), levels_scanned);
    if (!term_rows.empty()) {
      std::printf(" (");
      for (size_t k = 0; k < term_rows.size(); k++) std::printf("%slevel %d: %llu", k ? ", " : "", term_rows[k].level, term_rows[k].n_terminal);
      std::printf(")");
    }
    std::printf(", %llu unsettled (AllReplicasMoveToSameView false).\n", n_uns);
    if (unlisted_levels && deep_terminal)
      std::printf("%llu level(s) were expanded from the seen-set alone before a descent could scan them: %llu terminal states counted, not listed.\n", unlisted_levels, unlisted_deadlocks);
    else if (unlisted_levels)
      std::printf("%llu level(s) were expanded from the seen-set alone (the parents of the Virtual lines): %llu terminal states counted, not listed.  "
                  "Probed levels are not expanded: their terminal states are neither counted nor listed.\n", unlisted_levels, unlisted_deadlocks);
    if (probe2_at > 0 || probe3_at > 0)
      std::printf("The levels of -probe2At / -probe3At were not scanned: they have no records.\n");
    if (deep_terminal) {
      if (dterm_inexact) std::printf("%d probed level(s) listed more terminal copies than the list holds: their figures are lower bounds.\n", dterm_inexact);
      std::printf("Terminal states were examined through level %d (stored levels through %d%s).\n", std::max(last_scanned, dterm_through), last_scanned,
                  dterm_rows.empty() ? "" : dterm_rows.rbegin()->second.kind == 2 ? "; beyond them by the descents, the last one as the probed level" : "; beyond them by the descents");
    }
    if (dterm_uns_level && (!uns_level || dterm_uns_level < uns_level)) {
      std::printf("A terminal state of level %d has AllReplicasMoveToSameView false: the behaviour below reaches it and stutters there for ever, which is fair under "
                  "WF_vars(Next) — a counter-example to ViewChangeCompletes.\n", dterm_uns_level);
      bt_probed = dterm_rows[dterm_uns_level].kind == 2 ? 1 : 0;
      bt_unsettled = 1;
      if (!print_behaviour_to(dterm_uns_level, dterm_rows[dterm_uns_level].min_fp_unsettled, true)) exit_code = exit_code ? exit_code : 1;
      bt_probed = -1;
      bt_unsettled = 0;
    } else if (uns_level) {
      std::printf("A terminal state of level %d has AllReplicasMoveToSameView false: the behaviour below reaches it and stutters there for ever, which is fair under "
                  "WF_vars(Next) — a counter-example to ViewChangeCompletes.\n", uns_level);
      if (!print_behaviour_to(uns_level, uns_fp, true)) exit_code = exit_code ? exit_code : 1;
    } else {
      std::printf("No terminal state with AllReplicasMoveToSameView false was found: this is no verdict on ViewChangeCompletes (a behaviour that never reaches a "
                  "terminal state could still violate it; loops are not examined).\n");
    }
  }
  if (n_reach && rc == 0 && where_hit < 0 && deep_hit.k < 0 && !violated && !probed_violation && !deadlocked) {
    for (size_t k = 0; k < n_reach; k++)
      std::printf("No state satisfying %s was found in the %s.\n", query_names[k].c_str(),
                  where_unexamined ? "levels that were examined" : info.n_new == 0 && !incomplete ? "state space" : "levels searched");
    if (where_unexamined) std::printf("%llu level(s) were never stored (the Virtual lines): not examined.\n", where_unexamined);
    exit_code = exit_code ? exit_code : 14;
  }
  if (n_step_reach && rc == 0 && step_hit < 0 && where_hit < 0 && deep_hit.k < 0 && !violated && !probed_violation && !deadlocked) {
    for (size_t k = 0; k < n_step_reach; k++)
      std::printf("No step satisfying %s was found in the %s.\n", step_query_names[k].c_str(),
                  step_unexamined ? "levels that were examined" : info.n_new == 0 && !incomplete ? "state space" : "levels searched");
    if (step_unexamined) std::printf("%llu level(s) were never stored (the Virtual lines): not examined.\n", step_unexamined);
    exit_code = exit_code ? exit_code : 14;
  }
  if (step_report && rc == 0) {
    unsigned long long pairs = 0, errs = 0;
    for (const StepRow& r : step_rows) { pairs += r.n_pairs; errs += r.n_err; }
    if (!json)
      for (const StepRow& r : step_rows) {
        std::printf("Step report: level %d: %llu pairs from %llu states, %llu errors", r.level, r.n_pairs, r.n_states, r.n_err);
        for (size_t k = 0; k < step_names.size(); k++) std::printf(", %s %llu", step_names[k].c_str(), r.count[k]);
        std::printf("\n");
      }
    for (size_t k = 0; k < step_names.size(); k++) {
      unsigned long long total = 0;
      size_t with = 0;
      for (const StepRow& r : step_rows) { total += r.count[k]; with += r.count[k] ? 1 : 0; }
      std::printf("Step report: %s holds on %llu of %llu pairs, in %zu of %zu examined levels", step_names[k].c_str(), total, pairs, with, step_rows.size());
      bool first = true;
      for (const StepRow& r : step_rows)
        if (r.count[k] != r.n_pairs) { std::printf("%slevel %d: false on %llu", first ? " (" : ", ", r.level, r.n_pairs - r.count[k]); first = false; }
      std::printf("%s.\n", first ? "" : ")");
    }
    std::printf("Step report: %llu instances raise an evaluation error (not evaluated).\n", errs);
    if (step_unexamined) std::printf("%llu level(s) were never stored (the Virtual lines): not examined.  Probed levels are not examined either.\n", step_unexamined);
    if (probe2_at > 0 || probe3_at > 0) std::printf("The levels of -probe2At / -probe3At were not examined: they have no records.\n");
  }
  if (where_report && rc == 0) {
    for (size_t k = 0; k < where_names.size(); k++) {
      unsigned long long total = 0, states = 0;
      size_t with = 0;
      for (const WhereRow& r : where_rows) { total += r.count[k]; with += r.count[k] ? 1 : 0; }
      for (const WhereRow& r : where_rows) states += r.n_states;
      std::printf("Where report: %s holds in %llu of %llu states, in %zu of %zu examined levels", where_names[k].c_str(), total, states, with, where_rows.size());
      bool first = true;
      for (const WhereRow& r : where_rows)
        if (r.count[k]) { std::printf("%slevel %d: %llu", first ? " (" : ", ", r.level, r.count[k]); first = false; }
      std::printf("%s.\n", first ? "" : ")");
    }
    for (size_t i = 0; i < where_probed_rows.size(); i++) {       // a probed level that no later pass inserted: its figures stand alone (distinct states)
      const WhereRow& r = where_probed_rows[i];
      bool later = false;
      for (const WhereRow& q : where_rows) later = later || q.level == r.level;
      if (later) continue;
      std::printf("Where report: probed level %d (%s)", r.level, where_probed_exact[i] ? "exact" : "lower bounds: the list of collected copies overflowed");
      for (size_t k = 0; k < where_names.size(); k++) std::printf(", %s %llu", where_names[k].c_str(), r.count[k]);
      std::printf(".\n");
    }
    if (where_unexamined) std::printf("%llu level(s) were never stored (the Virtual lines): not examined.  Probed levels are not examined either.\n", where_unexamined);
    if (probe2_at > 0 || probe3_at > 0) std::printf("The levels of -probe2At / -probe3At were not examined: they have no records.\n");
  }
  if (deep_predicates && rc == 0 && !deep_seen.empty()) {
    int through_states = 0, through_steps = 0;
    for (const auto& kv : deep_seen) { through_states = std::max(through_states, kv.first); if (!kv.second) through_steps = std::max(through_steps, kv.first); }
    if (deep_state && deep_step) std::printf("Beyond the record buffers, states were examined through level %d and the transitions out of the levels through %d.\n", through_states, through_steps);
    else if (deep_state) std::printf("Beyond the record buffers, states were examined through level %d.\n", through_states);
    else std::printf("Beyond the record buffers, the transitions out of the levels through %d were examined.\n", through_steps);
    for (int lvl : deep_inexact) {
      bool later = false;                                         // (a later pass that inserted the level scanned every state of it)
      for (const auto& kv : deep_seen) later = later || (kv.first == lvl && kv.second == 0);
      if (!later)
        std::printf("Probed level %d: the list of collected copies overflowed — its counts are lower bounds, and a predicate that holds in few of its states may "
                    "have been missed there.\n", lvl);
    }
  }
  if (coverage) {   // ≙ tlc2.TLC -coverage, per action of Next: successors generated in the stored levels (probed / virtual levels not included)
    std::printf("The coverage statistics (successors generated per action):\n");
    for (int a2 = 1; a2 < 16; a2++) std::printf("  %s: %llu\n", vsrmc_action_name(a2), (unsigned long long)cov[a2]);
  }
  {  // TLC prints the same estimate: every generated state that was judged "seen" could be a 64-bit fingerprint collision
    const double n = (double)info.distinct, g = (double)info.total_generated;
    std::printf("The probability of a fingerprint collision hiding a state is estimated (optimistically) at %.1e.\n",
                n * (g > n ? g - n : 0.0) / 18446744073709551616.0);
  }
  std::printf("%llu states generated, %llu distinct states found, %llu states left on queue.\n", (unsigned long long)info.total_generated,
              (unsigned long long)info.distinct, (unsigned long long)(info.n_new));
  std::printf("The depth of the complete state graph search is %d.\nFinished in %.3f s (%.3g distinct states/s).\n", depth, dt,
              dt > 0 ? (double)info.distinct / dt : 0.0);
  if (dump) {
    std::fclose(dump);
    std::printf("%llu states dumped to %s.\n", dumped, dump_file.c_str());
  }
  if (audit && rc == 0 && recover_file.empty() && !rows.empty()) {
    // the second-hash audit: the same search under another member of the fingerprint family, to the depth the first one reached; only the counts are compared
    vsrmc_checker_destroy(c);
    c = nullptr;
    const uint64_t seed2 = 0x5EED5EED5EED5EEDull;
    size_t k = 0, first_diff = (size_t)-1;
    if (vsrmc_model_set_fp_seed(m, seed2) != 0 || vsrmc_checker_create(m, &o, &c) != 0) {
      std::printf("Error: audit run: %s\n", vsrmc_last_error());
      exit_code = exit_code ? exit_code : 1;
    } else {
      const int last = rows.back().level;
      int rc2 = 0;
      while (k < rows.size()) {
        int32_t what = 0, room = 0;
        vsrmc_level_info a, b;
        if ((rc2 = vsrmc_checker_room(c, &room)) != 0 || room == 2) break;
        if ((rc2 = vsrmc_checker_advance(c, &a, &b, &what)) != 0 || a.n_new == 0) break;
        if (what == 3) continue;
        const Row& r = rows[k];
        if (first_diff == (size_t)-1 && (a.level != r.level || a.n_new != r.n_new || a.generated != r.generated || a.deadlocks != r.deadlocks)) first_diff = k;
        k++;
        if (a.level >= last) break;
      }
      if (rc2 != 0) { std::printf("Error: audit run: %s\n", vsrmc_last_error()); exit_code = exit_code ? exit_code : 1; }
      else if (first_diff != (size_t)-1 || k != rows.size()) {
        const size_t d = first_diff != (size_t)-1 ? first_diff : k;
        std::printf("Audit: the per-level counts under fingerprint seed %016llx DIFFER from level %d on: a 64-bit fingerprint collision hid a state "
                    "under one of the two functions (TLC: rerun with another -fp).\n", (unsigned long long)seed2, d < rows.size() ? rows[d].level : last);
        exit_code = exit_code ? exit_code : 13;
      } else {
        std::printf("Audit: %zu levels, every new / generated / deadlock count equal under fingerprint seed %016llx.\n", rows.size(), (unsigned long long)seed2);
      }
    }
  }
  if (c) vsrmc_checker_destroy(c);
  if (w_all) vsrmc_where_destroy(w_all);
  if (w_query) vsrmc_where_destroy(w_query);
  if (w_con) vsrmc_where_destroy(w_con);
  if (s_all) vsrmc_where_destroy(s_all);
  if (s_query) vsrmc_where_destroy(s_query);
  vsrmc_model_destroy(m);
  return exit_code;
}
