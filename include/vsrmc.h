/* vsrmc.h — C ABI of libvsrmc.so, the MI355X-native explicit-state checker for VSR.tla.
 *
 * Drop-in boundary for the BFS hot path of TLC when it checks
 *   /root/reference/vsr-revisited/paper/VSR.tla  under  /root/reference/vsr-revisited/paper/VSR.cfg.
 * The reference repository holds no code of its own: the interfaces replaced are those of the TLC
 * classes the north star names — tlc2.tool.fp.FPSet, tlc2.tool.queue.StateQueue, tlc2.tool.Worker /
 * tlc2.tool.ModelChecker, tlc2.tool.impl.Tool, tlc2.tool.TLCTrace (recalled from TLC's public API) —
 * parameterised by VSR.cfg:3-37 (CONSTANTS / INIT / NEXT / VIEW / SYMMETRY / INVARIANT).
 *
 * Conventions: every entry point returns 0 on success and a negative VSRMC_E_* code on failure, with a text in
 * vsrmc_last_error() (thread-local).  Plain pointers and sizes only; the caller owns every buffer it passes, the
 * library copies in/out; handles are library-owned until *_destroy.  One host thread per handle.
 * "Wire layout" of a state record = 64-bit words [header][R replica blocks][bag words], documented in DESIGN.md
 * ("Packed record"); `off` arrays hold n+1 word offsets.
 */
#ifndef VSRMC_H
#define VSRMC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSRMC_E_ARG (-1)         /* bad argument / buffer too small */
#define VSRMC_E_CFG (-2)         /* .cfg / .tla not accepted by the lowering (names the line) */
#define VSRMC_E_HIP (-3)         /* HIP runtime failure or no GPU */
#define VSRMC_E_EVAL (-4)        /* TLC-style evaluation error inside the spec (e.g. VSR.tla:421) */
#define VSRMC_E_REP (-5)         /* a state left the range of the packed record / a capacity was exceeded */
#define VSRMC_E_STATE (-6)       /* call not valid in the handle's current state */

typedef struct vsrmc_model vsrmc_model;
typedef struct vsrmc_fpset vsrmc_fpset;
typedef struct vsrmc_checker vsrmc_checker;

const char* vsrmc_last_error(void);
int32_t vsrmc_version(void);
/* number of visible HIP devices (0 when there is no GPU; never an error) */
int32_t vsrmc_device_count(void);

/* ---- model = (VSR.tla, VSR.cfg) lowered to a record layout + action table ------------------------------------
 * vsrmc_model_load ≙ tlc2.TLC reading `-config VSR.cfg VSR.tla` (ModelConfig + SpecProcessor); grammar accepted:
 * VSR.cfg:3-37.  tla_path may be NULL (then only the cfg is read); if given, its SHA-256 must be the VSR.tla this
 * build lowers, any other module is refused. */
typedef struct vsrmc_layout {
  int32_t replica_count, client_count, value_count, start_view_on_timer_limit;
  int32_t symmetry, invariant_mask, assume_commit_number, check_deadlock;
  int32_t words_per_replica;     /* wire layout */
  int32_t fixed_words;           /* wire layout: index of the first bag word */
  int32_t permutations;          /* |Permutations(Values)| hashed per state */
  int32_t max_bag;               /* largest message bag a record may hold */
  int32_t max_record_words;      /* wire layout upper bound */
  int32_t module;                /* 0 = VSR.tla, 1 = VR_STATE_TRANSFER.tla, 2 = VR_APP_STATE.tla */
  int32_t reserved[2];
} vsrmc_layout;

int32_t vsrmc_model_load(const char* tla_path, const char* cfg_path, vsrmc_model** out);
int32_t vsrmc_model_from_constants(int32_t replica_count, int32_t client_count, int32_t value_count,
                                   int32_t start_view_on_timer_limit, int32_t restart_empty_limit, int32_t symmetry,
                                   int32_t invariant_mask, int32_t assume_commit_number, vsrmc_model** out);
/* The second model this build lowers: analysis/03-state-transfer/VR_STATE_TRANSFER.tla under the constants of
 * VR_STATE_TRANSFER.cfg:4-7.  invariant_mask: 1 AcknowledgedWriteNotLost, 2 AcknowledgedWritesExistOnMajority, 4 NoLogDivergence,
 * 8 CommitNumberNeverHigherThanOpNumber (the shipped cfg checks 2 + 4 + 8).  vsrmc_model_load recognises either module by the
 * SHA-256 of the .tla (or, without a .tla, by the cfg's constants); every other entry point takes either model. */
int32_t vsrmc_model2_from_constants(int32_t replica_count, int32_t value_count, int32_t start_view_on_timer_limit,
                                    int32_t no_progress_change_limit, int32_t symmetry, int32_t invariant_mask, vsrmc_model** out);
/* The third model ("then 04-application-state"): analysis/04-application-state/VR_APP_STATE.tla under the constants
 * of VR_APP_STATE.cfg:4-7 (ReplicaCount <= 3).  invariant_mask as above plus 16 NoAppStateDivergence (the shipped cfg checks
 * 2 + 4 + 8 + 16 = 30).  Without a .tla, vsrmc_model_load takes an analysis cfg that lists NoAppStateDivergence for this model. */
int32_t vsrmc_model3_from_constants(int32_t replica_count, int32_t value_count, int32_t start_view_on_timer_limit,
                                    int32_t no_progress_change_limit, int32_t symmetry, int32_t invariant_mask, vsrmc_model** out);
int32_t vsrmc_model_info(const vsrmc_model* m, vsrmc_layout* out);
/* Second-hash audit (TLC: a run repeated with another -fp N polynomial).  The seen-set knows a state by 64 bits of a hash; a false
 * merge of two states would drop one of them from every count, silently, in this checker AND in an oracle keyed by the same function.
 * `seed` is xor-ed into every salt of the view hash (csrc/vsr_model.hpp): seed 0 is the function the committed fixtures were made
 * with, every other seed an independent member of the same family — fingerprints, checksums and the counter-example's tie-breaks
 * change, distinct-state counts, generated / deadlock / per-action counts must not.  Set it before a checker is created from the
 * model (a checker copies the model); a checkpoint written under one seed is refused under another. */
int32_t vsrmc_model_set_fp_seed(vsrmc_model* m, uint64_t seed);
uint64_t vsrmc_model_fp_seed(const vsrmc_model* m);
/* Init (VSR.tla:323-348) in wire layout */
int32_t vsrmc_model_init_state(const vsrmc_model* m, uint64_t* rec, int32_t cap_words, int32_t* n_words);
/* TLC-syntax text of one state (the format of state_transfer_violation_trace.txt); returns needed size in *n */
int32_t vsrmc_model_format_state(const vsrmc_model* m, const uint64_t* rec, char* buf, int64_t cap, int64_t* n);
const char* vsrmc_action_name(int32_t action_id);
void vsrmc_model_destroy(vsrmc_model* m);

/* ---- FPSet ≙ tlc2.tool.fp.FPSet (init / putBlock / containsBlock / size / close) ---------------------------------
 * Open-addressing table of 2^log2_slots 16-byte slots in HBM.  put: was_present[i] = 1 iff fp[i] was already in the
 * set (FPSet.put's return value); equal fingerprints inside one batch: exactly one reports 0. */
int32_t vsrmc_fpset_create(int32_t device, int32_t log2_slots, vsrmc_fpset** out);
int32_t vsrmc_fpset_put_batch(vsrmc_fpset* s, const uint64_t* fps, uint64_t n, uint8_t* was_present);
int32_t vsrmc_fpset_contains_batch(vsrmc_fpset* s, const uint64_t* fps, uint64_t n, uint8_t* present);
/* same, buffers already in HBM (device pointers), enqueued on `hip_stream` (a hipStream_t, may be NULL) */
int32_t vsrmc_fpset_put_batch_device(vsrmc_fpset* s, const uint64_t* d_fps, uint64_t n, uint8_t* d_was_present,
                                     void* hip_stream);
int32_t vsrmc_fpset_contains_batch_device(vsrmc_fpset* s, const uint64_t* d_fps, uint64_t n, uint8_t* d_present,
                                          void* hip_stream);
int32_t vsrmc_fpset_size(vsrmc_fpset* s, uint64_t* size);
void vsrmc_fpset_destroy(vsrmc_fpset* s);

/* ---- Tool.getNextStates over all actions, for a batch of states (≙ tlc2.tool.impl.Tool.getNextStates) ------------
 * in: n records (wire layout).  out: successors in (parent, ordinal) order, wire layout, plus 8 words of meta each:
 * [parent index, ordinal, action id, fingerprint, auxkey, violated-invariant mask, error code, word offset]. */
int32_t vsrmc_expand_batch(const vsrmc_model* m, int32_t device, const uint64_t* words, const uint64_t* off, uint64_t n,
                           uint64_t* out_words, uint64_t out_words_cap, uint64_t* out_meta, uint64_t out_cap,
                           uint64_t* n_out, uint64_t* words_out);
/* ---- TLC state / trace import (≙ reading a TLC trace file or -dump output) ------------------------------
 * `text` holds states in TLC's value syntax: a trace expression  << [ _TEAction |-> [...], var |-> value, ... ], ... >>
 * (the format of the reference's state_transfer_violation_trace.txt), one state record  [ var |-> value, ... ]  (what
 * vsrmc_model_format_state prints), or TLC's console form ("State k: <Action ...>" + "/\ var = value" conjuncts).
 * out: wire records (bag words sorted), n+1 offsets, per state the action id named in the text (-1 if none).
 * words == NULL: only *n_states is set.  Variables the text leaves out keep their Init value. */
int32_t vsrmc_model_parse_states(const vsrmc_model* m, const char* text, uint64_t* words, uint64_t cap_words, uint64_t* off,
                                 int32_t* actions, uint64_t cap_states, uint64_t* n_states);
/* Is this sequence of states a behaviour of the model?  State 0 must be Init and every later state one of the successors the
 * GPU generates for its predecessor.  ords[i] / actions[i+1]: ordinal and action id of the step into state i+1 (ords can be fed
 * to vsrmc_model_replay); *first_bad: index of the first state that does not follow, -1 if none; *inv_mask_last: invariants
 * the last state violates. */
int32_t vsrmc_model_check_trace(const vsrmc_model* m, int32_t device, const uint64_t* words, const uint64_t* off, uint64_t n_states,
                                uint32_t* ords, int32_t* actions, int64_t* first_bad, int32_t* inv_mask_last);
/* canonical VIEW fingerprints (TLCState.fingerPrint with VIEW + SYMMETRY) of n records */
int32_t vsrmc_fingerprint_batch(const vsrmc_model* m, int32_t device, const uint64_t* words, const uint64_t* off,
                                uint64_t n, uint64_t* fps, uint32_t* auxkeys);

/* ---- TLC's own fingerprint: tlc2.util.FP64 over Value.fingerPrint of the `view` value (VSR.tla:140-150) ------------
 * A characterisation mode (VSR.tla only): the seen-set never uses it.  A TLC-STYLE FP64, not a parity-checked one: everything
 * TLC-specific is recalled, not pinned — see vsr_tlcfp.hpp.  One recalled detail is known to be doubtful: a model value is serialised
 * here as MODELVALUE + its index in cfg creation order, whereas ModelValue.fingerPrint may extend with the value's UniqueString token,
 * which is assigned in interning order over ALL strings of the parsed spec (module names, operators, fields ...), not over the model
 * values alone — if so, neither the FP64 values nor the min-permutation choice under SYMMETRY can be bit-equal to TLC's until a real
 * run's token table is supplied (tools/tlc_handoff.sh is where that would be found out).  With SYMMETRY the state fingerprinted is the permuted state TLC picks (TLCStateMut.fingerPrint: the smallest under
 * Value.compareTo, variable by variable in declaration order).
 * vsrmc_tlc_fingerprint_batch: n wire records -> FP64s, computed on the GPU.
 * vsrmc_tlc_view_bytes: the byte stream the fingerprint of ONE wire record is taken over, under value permutation `permutation`
 *   (0 = identity, < permutations); *n_bytes = its length, the first `cap` bytes stored.  Host code (a diagnostic).
 * vsrmc_tlc_min_permutation: the number of the permutation whose permuted state TLC fingerprints (host code).
 * vsrmc_fp64_new / vsrmc_fp64_extend: FP64.New() / FP64.Extend(fp, byte[]) (≙ tlc2.util.FP64).
 * vsrmc_checker_tlc_level_fps: FP64 of every state of the newest level, from the frontier in HBM, sorted; out may be NULL (time only);
 *   *kernel_ms = duration of the kernel. */
int32_t vsrmc_tlc_fingerprint_batch(const vsrmc_model* m, int32_t device, const uint64_t* words, const uint64_t* off, uint64_t n,
                                    uint64_t* fps);
int32_t vsrmc_tlc_view_bytes(const vsrmc_model* m, const uint64_t* record, int32_t permutation, uint8_t* out, uint64_t cap,
                             uint64_t* n_bytes);
int32_t vsrmc_tlc_min_permutation(const vsrmc_model* m, const uint64_t* record, int32_t* permutation);
uint64_t vsrmc_fp64_new(void);
uint64_t vsrmc_fp64_extend(uint64_t fp, const uint8_t* bytes, uint64_t n);

/* ---- the checker ≙ tlc2.tool.ModelChecker + Worker.run + StateQueue + TLCTrace ---------------------------------- */
typedef struct vsrmc_options {
  int32_t device;                /* HIP device ordinal */
  int32_t table_log2;            /* seen-set slots = 2^table_log2 (16 B each) */
  uint64_t frontier_words;       /* capacity of each of the two frontier buffers, in 8-byte words */
  uint64_t frontier_states;      /* capacity of each frontier in states */
  uint64_t pending_entries;      /* capacity of the per-level pending list (24 B each; only the exact scheme fills it) */
  int32_t keep_trace;            /* ignored (kept for ABI stability): predecessor pointers live in the seen-set slots, always */
  int32_t rank, world;           /* shard of the seen-set owned by this process (world = 1: everything) */
  uint64_t trace_entries;        /* ignored (there is no separate trace log any more) */
  int32_t exact_ties;            /* 0 (default): single-pass levels — the lane that inserts a fingerprint writes the successor;
                                    a same-level VIEW collision with different aux variables (never observed) stops the run
                                    with VSRMC_E_STATE.  1: two-kernel levels (k_expand + k_materialize) that arbitrate
                                    such ties exactly like the oracle (smallest canonical auxkey wins).  Sharded runs
                                    follow the same switch. */
  int32_t filter_log2;           /* sharded single-pass runs: entries (8 B) of this rank's sent-filter = 2^filter_log2;
                                    0 = table_log2 */
  int32_t host_frontier;         /* bit 0 / bit 1: the first (levels 1, 3, 5, ...) / second (levels 2, 4, ...) record buffer is
                                    pinned HOST memory that the kernels read and write over PCIe (3 = both); refs, fingerprints,
                                    trace log and seen-set stay in HBM.  For frontiers beyond 288 GB (≙ TLC's DiskStateQueue) */
  int32_t reserved0;
  uint64_t frontier_words_b;     /* capacity of the SECOND record buffer (levels 2, 4, 6, ...); 0 = frontier_words.  Level sizes
                                    grow geometrically, so the last two levels differ by that factor: size the buffers apart */
} vsrmc_options;

typedef struct vsrmc_level_info {
  int32_t level;                 /* level just completed (Init = 1) */
  int32_t error_code;            /* 0 or a device ERR_* code */
  uint64_t frontier;             /* states expanded in this step */
  uint64_t generated;            /* successors generated (TLC "states generated") */
  uint64_t n_new;                /* new distinct states = size of the next frontier */
  uint64_t distinct;             /* total distinct states so far */
  uint64_t total_generated;
  uint64_t deadlocks;            /* expanded states without successor */
  uint64_t pending;              /* candidates that raced for a slot claimed in this level */
  uint64_t probes;               /* seen-set slots inspected */
  uint64_t words_new;            /* words reserved in the next frontier buffer (device layout, chunk slack included) */
  uint64_t record_words;         /* words of the records of the next frontier themselves */
  uint64_t max_bag;
  uint64_t viol_fp;              /* smallest fingerprint of a violating new state, ~0 if none */
  uint64_t viol_index;           /* its index in the next frontier */
  int32_t viol_mask;
  int32_t reserved0;             /* vsrmc_checker_status: levels beyond `level` that exist in the seen-set only; 0 elsewhere */
  double seconds;                /* host wall time of the step */
  double expand_ms;              /* HIP-event time of k_expand (on the checker's stream) */
  double materialize_ms;         /* HIP-event time of k_materialize */
  uint64_t act_generated[16];    /* generated successors per action id */
  uint64_t phase_cycles[8];      /* k_expand shader clocks summed over blocks: stage, enumerate, sort, apply, tail */
  uint64_t fp_xor, fp_sum;       /* vsrmc_checker_probe2 / _probe3, the levels that are never stored: xor / sum (mod 2^64) of the level's
                                  * fingerprints (a stored level: vsrmc_checker_level_checksum) */
  uint64_t limit_rechecked;      /* a probed level: instances outside the invariants' footprint (not applied by a probe pass) that sat in a tile with a record
                                  * at a representation limit — bag within R - 1 entries of its capacity, a delivery count of 3.  Not 0: those passes were
                                  * run AGAIN with every action applied, so a limit hit by such a successor is reported like anywhere else (round 5: it went
                                  * unreported); 0 on every BASELINE configuration.  (k_probe_scan counts the RECORDS at such a limit that have such an
                                  * instance, not the instances of their tile: any value but 0 means the same) */
} vsrmc_level_info;

void vsrmc_options_default(vsrmc_options* o);
int32_t vsrmc_checker_create(const vsrmc_model* m, const vsrmc_options* o, vsrmc_checker** out);
/* the options the checker runs with: the caller's, with every size that was left 0 replaced by what was derived from the free memory */
int32_t vsrmc_checker_options(const vsrmc_checker* c, vsrmc_options* out);
/* back to the initial state: clears the seen-set and the trace log, keeps every allocation (≙ a fresh TLC run) */
int32_t vsrmc_checker_reset(vsrmc_checker* c);
/* expand the newest level by one BFS step; info->n_new == 0 means the search is exhausted */
int32_t vsrmc_checker_step(vsrmc_checker* c, vsrmc_level_info* info);
/* sorted fingerprints of the newest level */
int32_t vsrmc_checker_level_fps(vsrmc_checker* c, uint64_t* out, uint64_t cap, uint64_t* n);
int32_t vsrmc_checker_tlc_level_fps(vsrmc_checker* c, uint64_t* out, uint64_t cap, uint64_t* n, double* kernel_ms);
/* xor, sum (mod 2^64) and number of the fingerprints of the newest level, computed on the device (order-independent checksums
 * of a level's fingerprint SET: what the whole-workload fixtures of the CPU oracle hold per level) */
int32_t vsrmc_checker_level_checksum(vsrmc_checker* c, uint64_t* fp_xor, uint64_t* fp_sum, uint64_t* n_states);
/* the newest level in wire layout (≙ StateQueue.sDequeue(int) without removal) */
int32_t vsrmc_checker_frontier(vsrmc_checker* c, uint64_t* words, uint64_t cap_words, uint64_t* off, uint64_t cap_states,
                               uint64_t* n);
/* the states of the newest level in which at least one instance of an action of `action_mask` (bit a = action id a, the order of
 * `Next`, VSR.tla:896-918) is enabled — at most max_states of them, wire layout; *n_matching = how many there are in all
 * (≙ TLC's per-action coverage, as a filter) */
/* MEASUREMENT (not a product path; tools/bench_layout.py): one staging pass of k_expand's tile loop over the newest stored level, layout 0 =
 * the records as they are (refs + variable-length records), 1 = the same level as fixed-stride columns (SURVEY §8a row a1's SoA; a transposed copy is made
 * first, untimed).  Both fill the same LDS tile and read it back once.  *ms_per_pass = HIP-event time of one pass (mean of `reps`), *bytes_per_pass = what it reads.
 * Layouts 2-6 (round 6) are layout 0 with the tile loop software-pipelined / more resident blocks: 2 = refs one tile ahead, 3 = refs two and words one tile
 * ahead, 4 = layout 0 at eight blocks per CU, 5 / 6 = 2 / 3 at eight blocks per CU, 7 / 10 = layout 0 drawing 4 / 16 tiles from the cursor at a time, 8 / 9 =
 * 3 / 6 drawing 4 (csrc/vsr_bench_layout.hpp: k_stage_pipe). */
int32_t vsrmc_checker_bench_staging(vsrmc_checker* c, int32_t layout, int32_t reps, double* ms_per_pass, uint64_t* bytes_per_pass);
int32_t vsrmc_checker_select(vsrmc_checker* c, uint32_t action_mask, uint64_t max_states, uint64_t* words, uint64_t cap_words,
                             uint64_t* off, uint64_t* n_states, uint64_t* n_matching);
/* ≙ TLCTrace.getTrace: the path Init .. state `index` of the NEWEST level (level must be the current one); records in wire
 * layout, one action id per state (0 = Initial predicate).  The path is a function of the state alone: every state's slot in the
 * seen-set names its parent — of all states of the previous level that produce it the one with the smallest (canonical auxkey,
 * fingerprint) — and the step between two states of the path is the enabled instance with the smallest ordinal that leads from
 * one to the other; so the same counter-example comes back in every run, on any number of GPUs, in either level scheme. */
int32_t vsrmc_checker_trace(vsrmc_checker* c, int32_t level, uint64_t index, uint64_t* words, uint64_t cap_words,
                            uint64_t* off, int32_t* actions, uint64_t cap_states, uint64_t* n_states);
/* the same for any state of any completed level, addressed by its fingerprint */
int32_t vsrmc_checker_trace_fp(vsrmc_checker* c, int32_t level, uint64_t fp, uint64_t* words, uint64_t cap_words,
                               uint64_t* off, int32_t* actions, uint64_t cap_states, uint64_t* n_states);
/* forward half of TLCTrace.getTrace for a path given by the fingerprints of its states (fps[0] = Init's): at every step the
 * successor with the next fingerprint is taken — what a walk through the seen-set (vsrmc_checker_lookup) yields */
int32_t vsrmc_model_replay_fps(const vsrmc_model* m, int32_t device, const uint64_t* fps, int32_t n_fps, uint64_t* words,
                               uint64_t cap_words, uint64_t* off, int32_t* actions, uint64_t cap_states, uint64_t* n_states);
/* the same for a path of ordinals (simulation walks): re-execute `nsteps` ordinals from Init */
int32_t vsrmc_model_replay(const vsrmc_model* m, int32_t device, const uint32_t* ords, int32_t nsteps, uint64_t* words,
                           uint64_t cap_words, uint64_t* off, int32_t* actions, uint64_t cap_states, uint64_t* n_states);
/* one step of a trace walk through this checker's (shard of the) seen-set — what a walk that crosses ranks is made of.
 * by_low_bits = 0: the slot of fingerprint `key`; 1: the slot of the level-`level` state whose fingerprint ends in the 45 bits
 * `key` — *found = the number of such states in this shard: more than one (over all shards) is an ambiguous predecessor pointer,
 * which the walks report instead of following the first match.  meta = level(9) << 55 | auxkey(9) << 46 | parent fingerprint
 * bits(45) << 1 | taken(1). */
int32_t vsrmc_checker_lookup(vsrmc_checker* c, uint64_t key, int32_t level, int32_t by_low_bits, int32_t* found, uint64_t* fp,
                             uint64_t* meta);
/* index of fingerprint `fp` in the newest level (~0 if absent) */
int32_t vsrmc_checker_find_fp(vsrmc_checker* c, uint64_t fp, uint64_t* index);
void vsrmc_checker_destroy(vsrmc_checker* c);

/* ---- terminal states ≙ TLC's deadlock check (-deadlock / CHECK_DEADLOCK) with its counter-example ------------------------------
 * A state is TERMINAL when no (action, binding) instance is enabled in it — what vsrmc_level_info.deadlocks counts and where a simulation
 * walk ends.  k_terminal (csrc/vsr_terminal.hpp) finds them with a guards-only scan: no action applied, the seen-set untouched.
 * flags[i]: bit 0 = record i has no enabled (action, binding) instance; bit 1 = AllReplicasMoveToSameView (VSR.tla:958-962) is false in it.
 * A terminal state with bit 1 set is a counter-example to ViewChangeCompletes (VSR.tla:964-968) — the behaviour that stutters in it is fair;
 * finding none is no verdict: behaviours that loop are not examined.
 * vsrmc_terminal_batch: n wire records of the caller.
 * vsrmc_checker_terminal_scan: the newest STORED level, from the record buffer (HBM or pinned host memory).  Valid wherever
 *   vsrmc_checker_level_fps is, any number of times; changes nothing a later call can observe.  n_terminal of a scan of level L equals
 *   `deadlocks` of the step that then expands level L.  VSRMC_E_STATE on a sharded checker and while the deepest complete level exists in the
 *   seen-set only (after vsrmc_checker_deepen): those levels have no records, their terminal states stay counted.  The counter-example is
 *   vsrmc_checker_trace_fp(c, level, min_fp, ...) — the smallest fingerprint of the shallowest level that has a terminal state: the same state
 *   in every run, under every buffer size, in either level scheme.
 * vsrmc_checker_terminal_states: the terminal states the last scan found, fingerprints ascending (the rule of vsrmc_checker_probe_violators);
 *   fps == NULL asks for the number.  The scan keeps at most 2^20 of them: when the level has more, *n is still the true number, the call
 *   copies the ones held, returns VSRMC_E_REP and says so in vsrmc_last_error(); the scan's counters and minima are exact regardless.
 *   (Test knob: the environment variable VSRMC_TERMINAL_LIST_CAP=N, read by every scan, lowers the 2^20 to N so that the overflow path can be
 *   reached on a small space; it has no other use.) */
int32_t vsrmc_terminal_batch(const vsrmc_model* m, int32_t device, const uint64_t* words, const uint64_t* off, uint64_t n, uint8_t* flags);
typedef struct vsrmc_terminal_info {
  int32_t level, reserved0;                        /* the level scanned = the newest STORED level */
  uint64_t n_states, n_terminal, n_unsettled;      /* n_unsettled counts terminal states only */
  uint64_t min_fp, min_index;                      /* smallest fingerprint among the terminal states, its index in the level; ~0 if none */
  uint64_t min_fp_unsettled, min_index_unsettled;
  double kernel_ms;                                /* HIP-event time of k_terminal */
} vsrmc_terminal_info;
int32_t vsrmc_checker_terminal_scan(vsrmc_checker* c, vsrmc_terminal_info* out);
int32_t vsrmc_checker_terminal_states(vsrmc_checker* c, uint64_t* fps, uint8_t* flags, uint64_t cap, uint64_t* n);

/* ---- state predicates: user-written invariants and reachability queries ---------------------------------------------------------
 * A closed expression language over the lowered record, written in TLA+ syntax — the language, what is refused and where an evaluation
 * departs from TLC (accesses outside a domain have a defined result; model-value literals are refused under SYMMETRY; the aux variables are seen
 * through the representative the search keeps) are specified in csrc/vsr_where_parse.hpp.  The text holds one expression or definitions
 * `Name == expr`; every definition not written `LOCAL Name == expr` is exported, at most 8; exported predicate k is bit k everywhere below.
 * vsrmc_where_compile: needs no device.  VSRMC_E_ARG with "line:col: reason" in vsrmc_last_error() for a text that is refused (models 2 and 3:
 *   "state predicates: VSR.tla only"), VSRMC_E_REP for a program beyond 4096 ops or an operand depth beyond 32.
 * vsrmc_predicates_compile: the model-generic entry.  For a VSR.tla model it returns exactly what vsrmc_where_compile returns, op for op; for a model
 *   of vsrmc_model2_from_constants / vsrmc_model3_from_constants (or their cfgs) it compiles the same language over that spec's variables
 *   (no_progress, AnyDest, StateTransfer, m.log; on VR_APP_STATE.tla also rep_app_state and rep_recv_dvc — csrc/vsr_where_parse.hpp).  The object goes
 *   through every call below unchanged; a program is refused (VSRMC_E_ARG, "state predicates: compiled for another model") by any model but the
 *   one it was compiled for — the two analysis models with equal constants are different models.  vsrmc_where_compile and vsrmc_step_compile keep
 *   refusing the analysis models.
 * vsrmc_where_batch: n wire records of the caller (the layout of vsrmc_terminal_batch); flags[i] = the bits of record i.
 * vsrmc_checker_where_scan: k_where (csrc/vsr_where.hpp) over the newest STORED level.  Valid exactly where vsrmc_checker_terminal_scan is
 *   (VSRMC_E_STATE on a sharded checker, on seen-set-only levels, after a failed search), any number of times; changes nothing a later call
 *   can observe.  count / min_fp are exact.  The witness of predicate k is vsrmc_checker_trace_fp(c, level, min_fp[k], ...): with levels scanned
 *   shallowest first it is a shortest behaviour into a state that satisfies k, and the same one in every run.
 * vsrmc_checker_where_states: the records of the last scan with any bit set, fingerprints ascending, their bits beside them; fps == NULL asks
 *   for the number.  The contract of vsrmc_checker_terminal_states: at most 2^20 are kept, beyond that *n is the true number and the call
 *   returns VSRMC_E_REP.  (Test knob: the environment variable VSRMC_WHERE_LIST_CAP=N lowers the 2^20 to N; it has no other use.)
 * The compute calls fail with VSRMC_E_HIP without a device: there is no CPU evaluation. */
typedef struct vsrmc_where vsrmc_where;
typedef struct vsrmc_where_desc {
  int32_t n_names;                                 /* exported predicates */
  int32_t n_ops, depth;                            /* program length (the final END included), operand-stack depth */
  int32_t msg_loops;                               /* nesting of the quantifiers over DOMAIN messages that remain as loops: 0, 1 or 2 */
  int32_t n_bodies;                                /* quantifier bodies after unfolding (\E r1, r2 \in replicas at ReplicaCount 3: 9) */
  int32_t step;                                    /* 1: a step program (vsrmc_step_compile, below); 0: a state program */
  char names[8][64];
} vsrmc_where_desc;
typedef struct vsrmc_where_info {
  int32_t level, reserved0;                        /* the level scanned = the newest STORED level */
  uint64_t n_states;
  uint64_t count[8];                               /* records that satisfy predicate k */
  uint64_t min_fp[8], min_index[8];                /* the smallest fingerprint among them and its index in the level; ~0 if none */
  double kernel_ms;                                /* HIP-event time of k_where */
} vsrmc_where_info;
int32_t vsrmc_where_compile(const vsrmc_model* m, const char* text, vsrmc_where** out);
int32_t vsrmc_predicates_compile(const vsrmc_model* m, const char* text, vsrmc_where** out);
void vsrmc_where_destroy(vsrmc_where* w);
int32_t vsrmc_where_describe(const vsrmc_where* w, vsrmc_where_desc* out);
int32_t vsrmc_where_batch(const vsrmc_model* m, int32_t device, const vsrmc_where* w, const uint64_t* words, const uint64_t* off, uint64_t n, uint8_t* flags);
int32_t vsrmc_checker_where_scan(vsrmc_checker* c, const vsrmc_where* w, vsrmc_where_info* out);
int32_t vsrmc_checker_where_states(vsrmc_checker* c, uint64_t* fps, uint8_t* bits, uint64_t cap, uint64_t* n);

/* ---- state constraints: where the search does not go (TLC's CONSTRAINT) ---------------------------------------------
 * One exported predicate of a state program (vsrmc_predicates_compile / vsrmc_where_compile) attached to a checker.  A successor that fails it is OUT OF
 * MODEL: it is generated and counted in `generated`, the built-in invariants are checked on it, but it is no distinct state, is not expanded and is never
 * a parent in a trace; an in-model state that is reachable only through out-of-model states is NOT reached.  Init is subject to it.  Deadlock stays "no
 * successor generated", in the model or not.  [TLC-RECALLED: these semantics are written from memory of tlc2.tool.Worker / ModelChecker.doNext; they
 * are not pinned against a TLC run.]  A CONSTRAINT section of a cfg stays refused at load: the constraint is attached through this interface only.
 * How: k_constrain (csrc/vsr_constrain.hpp) runs over every level vsrmc_checker_step has just committed, before the call returns, and withdraws the
 *   states that fail (their index slots become unused ones); they keep their seen-set slot.  In the vsrmc_level_info of such a step n_new, distinct and
 *   record_words are the in-model figures; generated, act_generated and viol_* stay k_expand's.  A built-in violation on an out-of-model state is
 *   reported as ever, with viol_index ~0: its behaviour is vsrmc_checker_trace_fp(c, level, viol_fp, ...).  A level of which nothing is in the model ends
 *   the search like a level without new states (n_new 0, the checker stays at the level before; the pruned level can still be traced by fingerprint).
 *   Terminal, where and step scans of a stored level see the in-model states; pruned_count / pruned_min_fp_k below are the same program's other exported
 *   predicates over the PRUNED states, so that a user's invariant is not lost on them.
 * vsrmc_checker_constrain_attach: accepted only on a checker at level 1 (fresh, or after vsrmc_checker_reset); evaluates Init at once — Init out of
 *   model: the level is empty, distinct 0, the next step reports an exhausted search.  vsrmc_checker_reset keeps the attachment and evaluates Init again.
 *   w == NULL detaches and starts the search over.  The program is copied; its device buffers are allocated once per attachment.
 *   Refused: VSRMC_E_ARG for a step program, a program compiled for another model, a name_index the program does not export, and a program that reads
 *   aux_svc or aux_client_acked (outside VIEW: the copy of a state that arrived first would decide its membership; under SYMMETRY the compiler already
 *   refuses value literals, so every accepted predicate is symmetric); VSRMC_E_STATE on a sharded checker (world > 1), after level 1, with predicates
 *   attached by vsrmc_checker_deep_attach, and for a second attachment.
 * While a constraint is attached: vsrmc_checker_deepen, _probe, _probe2, _probe3, _deep_attach and _save are refused (VSRMC_E_STATE: the levels beyond
 *   the record buffers are not constrained; a checkpoint does not name the constraint).  vsrmc_checker_advance stores levels only: when the next level is
 *   not predicted to fit, or overflowed, it returns 0 with *what = 4 and the reason in vsrmc_last_error(); vsrmc_check then stops with stop_reason 5.
 *   The seen-set: a pruned state is no distinct state but keeps its slot, so vsrmc_checker_room counts distinct PLUS every state pruned since the search started
 *   as the table's load (it grows the table, or reports it full, by that figure).  The record buffers: k_expand writes a level before the filter runs, so the
 *   prediction of vsrmc_checker_advance scales the in-model figures by (kept + pruned) / kept of the newest filtered level; a level that overflows all the same is
 *   the *what = 4 stop in the single-pass scheme.  Under exact_ties there is neither prediction nor that path: an overflow is the plain "frontier full" error
 *   (VSRMC_E_REP) and the checker has failed.
 * vsrmc_checker_constraint_info: the figures of one filtered level (level 1 = Init; level 0 asks for the newest filtered one).  kept_xor / kept_sum / kept are what vsrmc_checker_level_checksum
 *   gives for the filtered level, without a second pass.
 * vsrmc_checker_constraint_pruned: the fingerprints of the newest filtered level's pruned states, ascending; fps == NULL asks for the number.  The
 *   contract of vsrmc_checker_where_states: at most 2^20 are kept (the same test knob VSRMC_WHERE_LIST_CAP=N lowers that), beyond that *n is the true
 *   number and the call returns VSRMC_E_REP; counts and minima are exact regardless.  The list is copied from the device and sorted by the first call after a level
 *   was filtered, not by the step: a run that never asks pays nothing for it.
 * (Test knob: the environment variable VSRMC_CONSTRAIN_GRID=N caps k_constrain's grid at N blocks, so that a small level drives its grid-stride loop
 *   through several trips; it has no other use.) */
typedef struct vsrmc_constraint_info {
  int32_t level, k;                                /* the level filtered; the exported predicate that is the constraint */
  uint64_t n_states;                               /* states of the level as k_expand left it = kept + pruned */
  uint64_t kept, pruned;
  uint64_t kept_xor, kept_sum;                     /* xor / sum mod 2^64 of the in-model fingerprints */
  uint64_t kept_max_bag, kept_words;               /* largest bag and record words among the in-model states */
  uint64_t pruned_min_fp;                          /* the smallest pruned fingerprint; ~0 if none */
  uint64_t pruned_count[8], pruned_min_fp_k[8];    /* per exported predicate p: PRUNED states with bit p set, the smallest fingerprint among them (~0 if none) */
  double kernel_ms;                                /* HIP-event time of k_constrain */
} vsrmc_constraint_info;
int32_t vsrmc_checker_constrain_attach(vsrmc_checker* c, const vsrmc_where* w, int32_t name_index);
int32_t vsrmc_checker_constraint_info(vsrmc_checker* c, int32_t level, vsrmc_constraint_info* out);
int32_t vsrmc_checker_constraint_pruned(vsrmc_checker* c, uint64_t* fps, uint64_t cap, uint64_t* n);

/* ---- the state constraint on the levels beyond the record buffers (opt-in) -----------------------------------------------
 * vsrmc_checker_constrain_deep(c, 1): valid on a checker with a state constraint attached and still at level 1 (right after the attachment, or after
 *   vsrmc_checker_reset, which keeps it).  From then on vsrmc_checker_advance, vsrmc_check, _deepen and _probe do what they do on an unconstrained checker,
 *   filtered, and the *what = 4 stop does not occur.  on = 0 turns it off again (at level 1).  Without it everything above holds as written.
 * How: every state of every seen-set-only level sits in a scratch buffer once per descent before anything reads it; k_constrain_slice
 *   (csrc/vsr_deep_constrain.hpp) runs on every such slice and withdraws the states that fail (off = 0, fp = 0), so that the next nesting level, the probe pass,
 *   the re-basing export and the inserted level's checksum see in-model states only.  A pruned state keeps its seen-set slot (membership is a function of the
 *   VIEW): it comes back with every regeneration and is filtered again, with the same verdict.  The figures of a level are recorded once, by the first
 *   descent that filters it; vsrmc_checker_constraint_info answers for such a level as for a stored one.
 *   The inserted level of a descent is filtered sub-slice by sub-slice before it is counted: n_new, fp_xor, fp_sum and distinct of its vsrmc_level_info are
 *   the in-model figures; generated, act_generated and viol_* stay the expand pass's.  The probed level is the successors of its in-model states.
 *   Two levels reach the seen-set before a record of theirs exists to be judged: the one the first vsrmc_checker_deepen after a stored level inserts, and a
 *   level adopted after "frontier full".  Their vsrmc_level_info carries the UNFILTERED figures and vsrmc_checker_constraint_deep_info says filtered = 0; the
 *   next descent regenerates and filters such a level before it expands it, records its figures, and lowers distinct by its pruned count.  No state is
 *   expanded, probed or exported before it was judged.  A descent whose filtered levels leave nothing to insert ends the search (n_new 0), also when the
 *   level inserted last turns out wholly out of model one descent later: the depth is then the level below it.
 * Still refused with the opt-in on (VSRMC_E_STATE): an action constraint (either order of attachment), sharded checkers, exact_ties, vsrmc_checker_probe2 /
 *   _probe3, _deep_attach, _deep_terminal_attach and _save.
 * vsrmc_checker_constraint_deep_info: what a level beyond the record buffers adds to its vsrmc_constraint_info.
 * vsrmc_checker_constraint_pruned_level: vsrmc_checker_constraint_pruned for a level by number — the newest filtered level (0, or its number) or the OTHER
 *   level the last filtering descent recorded (it records two when it meets a level with filtered = 0); VSRMC_E_ARG for any other level. */
typedef struct vsrmc_constraint_deep_info {
  int32_t level;
  int32_t kind;                                    /* 1: first filtered as a regenerated level, 2: as the inserted level of a descent */
  int32_t filtered;                                /* 0: complete in the seen-set, not judged yet (kind 1: the next descent does it) */
  int32_t list_overflowed;                         /* the level pruned more states than its list holds (counts and minima are exact) */
  uint64_t slices;                                 /* scratch slices the recording descent filtered it in */
  uint64_t launches;                               /* k_constrain_slice launches on the level, every descent since included */
  uint64_t regen_records, regen_pruned;            /* records of the level regenerated by every descent so far, and the pruned ones among them */
} vsrmc_constraint_deep_info;
int32_t vsrmc_checker_constrain_deep(vsrmc_checker* c, int32_t on);
int32_t vsrmc_checker_constraint_deep_info(vsrmc_checker* c, int32_t level, vsrmc_constraint_deep_info* out);
int32_t vsrmc_checker_constraint_pruned_level(vsrmc_checker* c, int32_t level, uint64_t* fps, uint64_t cap, uint64_t* n);

/* ---- action constraints: which steps the search does not take (TLC's ACTION_CONSTRAINT) ---------------------------------
 * One exported predicate P of a step program (vsrmc_step_predicates_compile, below) attached to a checker.  A transition (s, t) by an instance
 * (parent, ordinal) is GENERATED and counted in `generated` and act_generated as ever.  P true: t is fingerprinted and claimed in the seen-set; a new t
 * is written to the next level with s as its candidate parent (the min-key rule).  P false: the transition is BLOCKED — t is not fingerprinted into
 * the seen-set and not written, and may still enter the model through a permitted transition of the same or a later level (what separates an action
 * constraint from a state constraint, which judges t whatever led to it).  Init is not subject to it.  The parent pointer of every stored state is a
 * permitted parent, and vsrmc_checker_trace / _trace_fp take permitted steps only: where several instances of one parent lead to one child, the smallest
 * permitted ordinal is taken.  An instance whose action raises an evaluation error ends the run as without a constraint.  Deadlock stays "no successor
 * generated".  [TLC-RECALLED: written from memory of tlc2.tool.ModelChecker.doNext, not pinned against a TLC run.]  Departure: TLC (recalled) checks the
 * invariants on a successor it then discards; here the built-in invariants are evaluated on blocked successors only to COUNT them
 * (blocked_violating, blocked_viol_mask, blocked_viol_min_fp) — no violation is reported for a state that is not in the model.  An ACTION_CONSTRAINT
 * section of a cfg stays refused at load: the constraint is attached through this interface only.
 * How: vsrmc_checker_step runs k_step_list, k_step_apply (the verdict) and k_step_expand (csrc/vsr_action_constrain.hpp) over slices of the newest level
 *   in the place of k_expand; the level it leaves has k_expand's format (dense: no unused index), so every scan, trace and accessor works on it, and a
 *   state constraint (vsrmc_checker_constrain_attach) may be attached beside it.  A checker without an action constraint runs the code it ran before.
 *   vsrmc_checker_step_scan of a constrained checker judges the permitted transitions only: per slice the constraint's verdicts first (k_step_apply), the
 *   permitted entries of the list kept (k_step_keep), then the caller's program over those — n_pairs, counts, minima, the witness ordinal and
 *   vsrmc_checker_step_pairs are those of the constrained model, and the pair vsrmc_checker_step_successor gives is a permitted step.
 *   A permitted trace costs two batch calls (vsrmc_expand_batch, vsrmc_step_batch) of one record per state of the path: a report's cost, not a hot path.
 * vsrmc_checker_action_constrain_attach: accepted only on a checker at level 1 (fresh, or after vsrmc_checker_reset); starts the search over.  w == NULL
 *   detaches, at any level, and starts the search over.  The program is copied; its device buffers are allocated once per attachment.
 *   Refused: VSRMC_E_ARG for a state program (vsrmc_where_desc.step must be set), a program compiled for another model, a name_index the program
 *   does not export, and a program that reads aux_svc or aux_client_acked, primed or not (outside VIEW: the copy of a state that arrived first would decide
 *   which transitions are taken; under SYMMETRY the compiler already refuses value literals); VSRMC_E_STATE with exact_ties = 1, on a sharded checker
 *   (world > 1), after level 1, with predicates attached by vsrmc_checker_deep_attach, and for a second attachment.
 * While attached (and unless vsrmc_checker_action_constrain_deep, below, lifts it for _deepen, _probe and _advance): vsrmc_checker_deepen, _probe, _probe2,
 *   _probe3, _deep_attach and _save are refused (VSRMC_E_STATE), and vsrmc_checker_advance stores
 *   levels only — when the next level is not predicted to fit, or overflowed, it returns 0 with *what = 4 (vsrmc_check: stop_reason 5), as with a state
 *   constraint.  Blocked successors take neither record room nor a seen-set slot: the prediction is not scaled for them and vsrmc_checker_room counts the
 *   distinct states as the table's load.
 * vsrmc_checker_action_constraint_info: the figures of the step that led INTO `level` (>= 2; 0 asks for the newest step, which may have found no state).
 * (Test knobs: the environment variable VSRMC_ACTION_SLICE=N fixes the parents per slice at N — without it the first slice of a level is sized so that
 *   the list cannot overflow and the later ones from the instances per parent seen so far, times 1.5; VSRMC_ACTION_LIST_CAP=N, read at attach, shortens
 *   the instance list (default 2^22 entries, at least 64), so that slices overflow it and are listed again in halves.  They have no other use.) */
typedef struct vsrmc_action_constraint_info {
  int32_t level, k;                                /* the level the step led into; the exported predicate that is the constraint */
  uint64_t parents;                                /* states expanded */
  uint64_t pairs, permitted, blocked;              /* transitions generated = taken + not taken */
  uint64_t blocked_act[16];                        /* blocked per action id */
  uint64_t blocked_violating, blocked_viol_mask;   /* blocked successors that fail a built-in invariant; the or of their masks */
  uint64_t blocked_min_fp, blocked_viol_min_fp;    /* the smallest PARENT fingerprint of a blocked pair / of one whose successor fails an invariant; ~0 if none */
  uint64_t n_new;                                  /* new states the step wrote */
  uint64_t slices, relisted, launches;             /* k_step_list launches; of them slices that overflowed the list and were listed again in halves; kernel launches in all */
  double list_ms, verdict_ms, expand_ms;           /* HIP-event time of k_step_list, k_step_apply, k_step_expand, summed over the slices */
} vsrmc_action_constraint_info;
int32_t vsrmc_checker_action_constrain_attach(vsrmc_checker* c, const vsrmc_where* step_program, int32_t name_index);
int32_t vsrmc_checker_action_constraint_info(vsrmc_checker* c, int32_t level, vsrmc_action_constraint_info* out);
/* ---- an action constraint on the levels beyond the record buffers (opt-in) -----------------------------------------------
 * vsrmc_checker_action_constrain_deep(c, 1): called on a checker with an action constraint attached and still at level 1 (right after the attachment, or
 *   after vsrmc_checker_reset), like vsrmc_checker_constrain_deep.  From then on vsrmc_checker_advance, vsrmc_check, vsrmc_checker_deepen and
 *   vsrmc_checker_probe go on past the record buffers as on an unconstrained checker, taking PERMITTED transitions only — *what = 4 no longer occurs, and a
 *   stored level that overflowed is adopted as the first seen-set-only level.  (c, 0) turns it off again, at level 1.  Without the call every answer is what
 *   it was.
 * The semantics are those above, carried over: a blocked transition is generated and counted and not taken — its successor is not fingerprinted into the
 *   seen-set by that edge, not written and not probed; the same state may enter through a permitted edge of the same or a later level.  Every parent pointer
 *   in the seen-set was written by a permitted transition, so vsrmc_checker_trace_fp on a fingerprint of a deep level and vsrmc_checker_probe_trace (its last
 *   step into a violator of the probed level included) take permitted steps only.  On the probed level only successors of permitted transitions are
 *   candidates for a violation.  A blocked successor's invariants are evaluated only to count it.  Two successors of one level with one VIEW fingerprint and
 *   different aux keys fail the run with the stored path's message.
 * How: the record-less first pass, the level a descent inserts and the probed level run k_step_list, k_step_apply and k_step_expand (its insert, stored and
 *   probe modes: csrc/vsr_action_constrain.hpp) over slices of their parents in the place of k_expand; the regenerating passes run k_expand unchanged — a
 *   regenerating lane takes a state only under the key a permitted transition wrote, so the regenerated level is the recorded one (§9m).  No claim bitmap is
 *   kept: regeneration asks the seen-set.
 * Refused with the opt-in on (VSRMC_E_STATE): beside a state constraint, deep or not (the record-less pass cannot judge states — the combination is the
 *   follow-up), and vsrmc_checker_constrain_deep / _constrain_attach after it; vsrmc_checker_deep_attach, _deep_terminal_attach, _probe2, _probe3, _save;
 *   exact_ties and sharded checkers refuse the attachment already.
 * vsrmc_checker_action_constraint_deep_info: the figures of the gated passes that led INTO `level`, a level beyond the record buffers: kind 1 = inserted
 *   record-less (the first pass, or a stored level that overflowed and was adopted), 2 = inserted by a descent, 3 = probed (the level after the inserted
 *   one: nothing of it is in the seen-set; the next pass inserts it and files it anew as kind 2).  VSRMC_E_ARG for any other level. */
typedef struct vsrmc_action_constraint_deep_info {
  int32_t level, kind;
  uint64_t parents;                                /* states expanded (a probed level after a violation in the inserted one: fewer than the level has) */
  uint64_t pairs, permitted, blocked;              /* transitions generated = taken (kind 3: looked up) + not taken */
  uint64_t blocked_act[16];                        /* blocked per action id */
  uint64_t blocked_violating, blocked_viol_mask;   /* as in vsrmc_action_constraint_info */
  uint64_t blocked_min_fp, blocked_viol_min_fp;    /* the smallest PARENT fingerprint of a blocked pair / of one whose successor fails an invariant; ~0 if none */
  uint64_t slices, relisted, launches;             /* k_step_list launches over all the gated passes into the level; the void ones among them; kernel launches in all */
  double list_ms, verdict_ms, expand_ms;           /* HIP-event time of k_step_list, k_step_apply, k_step_expand, summed */
} vsrmc_action_constraint_deep_info;
int32_t vsrmc_checker_action_constrain_deep(vsrmc_checker* c, int32_t on);
int32_t vsrmc_checker_action_constraint_deep_info(vsrmc_checker* c, int32_t level, vsrmc_action_constraint_deep_info* out);
/* the seen-set's load as the table shows it: slots that hold a fingerprint, of how many.  Counted on the host from a copy of the table (tests, reports). */
int32_t vsrmc_checker_seen_set_load(vsrmc_checker* c, uint64_t* occupied, uint64_t* slots);

/* ---- step predicates: user-written predicates over a state AND its successor, checked on every transition -------------------------
 * The safety half of PROPERTY: an action property [][P]_vars is a predicate over a (state, successor) pair.  The language of the state predicates
 * plus primed variables (rep_view_number'[r], Len(rep_log[r])', (...)', \A m \in DOMAIN messages', messages'[m]), UNCHANGED e and step_action (the
 * Next disjunct that produced the pair — not TLA+) — csrc/vsr_where_parse.hpp specifies it, what is refused, and where it departs from TLC: the
 * primed aux variables are those of the successor AS GENERATED (before the search picks the representative of its VIEW class), and a pair whose
 * successor equals its state is evaluated like any other (TLC's [][P]_vars would skip it).  Exported predicate k is bit k everywhere below.
 * vsrmc_step_compile: needs no device.  A text without primes compiles to exactly the ops vsrmc_where_compile gives it; the program carries a step
 *   flag (vsrmc_where_desc.step).  vsrmc_where_compile keeps refusing primes; vsrmc_where_batch / vsrmc_checker_where_scan refuse a step program
 *   (VSRMC_E_ARG), vsrmc_step_batch / vsrmc_checker_step_scan a state program.  The same caps: 4096 ops, depth 32, 8 exports.  Destroyed and
 *   described by vsrmc_where_destroy / vsrmc_where_describe.  Models 2 and 3: "step predicates: VSR.tla only".
 * vsrmc_step_predicates_compile: the model-generic entry, as vsrmc_predicates_compile is for states.  For a VSR.tla model it returns exactly what
 *   vsrmc_step_compile returns, op for op; for a model of vsrmc_model2_from_constants / vsrmc_model3_from_constants (or their cfgs) it compiles the step
 *   language over that spec's variables (rep_log'[r], no_progress'[r], \A m \in DOMAIN messages' with m.log; on VR_APP_STATE.tla also rep_app_state'[r],
 *   Cardinality(rep_recv_dvc[r])' and \A d \in rep_recv_dvc'[r] — csrc/vsr_where_parse.hpp).  The program records its model and the step flag: every
 *   call below takes it unchanged, and it is refused by any model but its own and by the state entry points.
 * vsrmc_step_batch: n wire records of the caller -> one row of five words per generated successor, in (parent, ordinal) order — the rows of
 *   vsrmc_expand_batch over the same batch, row for row: [parent, ordinal, action id, bits, error code].  An instance whose action raises an
 *   evaluation error (error code != 0) is not evaluated: its bits are 0.  rows == NULL asks for the number.
 * vsrmc_checker_step_scan: every transition out of the newest STORED level (csrc/vsr_step.hpp: k_step_list lists the enabled instances, k_step_apply
 *   evaluates each pair without writing a successor).  Valid exactly where vsrmc_checker_where_scan is, with the same VSRMC_E_STATE cases, any
 *   number of times; changes nothing a later call can observe.  n_pairs + n_err == `generated` of the step that then expands the level.  count /
 *   min_fp are exact; min_fp[k] is the smallest PARENT fingerprint with a pair that satisfies k, min_ordinal[k] the smallest ordinal of that parent
 *   with bit k, min_action[k] its action id: the same pair whatever the slice size and the list size.  Across runs min_fp and the counts are the same;
 *   the ordinal is a position in the bag of the record as THIS run's level stores it (under SYMMETRY a level may store another member of the state's
 *   orbit from run to run), so min_ordinal / min_action may name another instance of the same parent in another run.  The level is run in slices of parents sized
 *   so that the instance list (2^22 entries) cannot overflow; the device counter is checked after every slice regardless, and a slice that
 *   offered more is run again in halves.  (Test knob: the environment variable VSRMC_STEP_SLICE=N sets the parents per slice; it has no other use.)
 * vsrmc_checker_step_pairs: the pairs of the last scan with any bit set, by (parent fingerprint, ordinal), their bits beside them; fps == NULL
 *   asks for the number.  The contract of vsrmc_checker_where_states: at most 2^20 are kept, beyond that *n is the true number and the call
 *   returns VSRMC_E_REP.  (Test knob: the environment variable VSRMC_STEP_LIST_CAP=N lowers the 2^20 to N; it has no other use.) */
typedef struct vsrmc_step_info {
  int32_t level, reserved0;                        /* the level scanned = the newest STORED level */
  uint64_t n_states;                               /* parent records */
  uint64_t n_pairs, n_err;                         /* pairs evaluated; instances whose action raises an evaluation error (not evaluated) */
  uint64_t count[8];                               /* pairs that satisfy predicate k */
  uint64_t min_fp[8], min_index[8];                /* the smallest parent fingerprint among them and its index in the level; ~0 if none */
  uint32_t min_ordinal[8];                         /* of that parent, the smallest ordinal with bit k; ~0 if none */
  int32_t min_action[8];                           /* ... and its action id; -1 if none */
  double kernel_ms, list_ms, apply_ms;             /* HIP-event time of both kernels over all slices, and of each */
  uint64_t slices;                                 /* launches of k_step_list (slices run again in halves included) */
} vsrmc_step_info;
int32_t vsrmc_step_compile(const vsrmc_model* m, const char* text, vsrmc_where** out);
int32_t vsrmc_step_predicates_compile(const vsrmc_model* m, const char* text, vsrmc_where** out);
int32_t vsrmc_step_batch(const vsrmc_model* m, int32_t device, const vsrmc_where* w, const uint64_t* words, const uint64_t* off, uint64_t n, uint64_t* rows,
                         uint64_t cap_rows, uint64_t* n_rows);
int32_t vsrmc_checker_step_scan(vsrmc_checker* c, const vsrmc_where* w, vsrmc_step_info* out);
/* the successor pair (index, ordinal) of the level of the last step scan leads to — the record as the action generates it — and its action id.  Valid
 * while that level is the newest stored one (VSRMC_E_STATE afterwards): the ordinal names a position in the bag of the record as the level stores it.
 * parent != NULL: a wire record of the same state (the last record of vsrmc_checker_trace_fp: under SYMMETRY it may be another member of the state's
 * orbit than the stored one); the successor returned is then the one that record has under the same action with the same fingerprint, so that the
 * trace and its last step are one behaviour. */
int32_t vsrmc_checker_step_successor(vsrmc_checker* c, uint64_t index, uint32_t ordinal, const uint64_t* parent, uint64_t parent_words, uint64_t* words,
                                     uint64_t cap_words, uint64_t* n_words, int32_t* action);
int32_t vsrmc_checker_step_pairs(vsrmc_checker* c, uint64_t* fps, uint32_t* ordinals, uint8_t* bits, uint64_t cap, uint64_t* n);

/* Probe level: expand the newest level without storing its successors — invariants are evaluated on every successor that is
 * not a state of an earlier level, nothing is inserted or written, so the level costs no frontier memory; the search cannot
 * continue afterwards.  Finds a violation one level beyond what memory can hold.  Also valid right after a step that failed
 * with "frontier full".  Order of evaluation (the result is that of the sentence above): every enabled instance is enumerated and
 * counted; only the actions that write a variable the invariants read are applied (VSR.tla: rep_log, aux_client_acked — a successor
 * of any other action has the verdict of its parent, which passed); of their successors the invariants are evaluated first, and
 * only a successor that fails one is fingerprinted and looked up in the seen-set.  "Which passed" is the premise: when a level this
 * checker committed held a violating state (a caller that steps on after a reported violation), the probe passes apply EVERY action.
 * Representation errors (ERR_REP_*) of an action outside the footprint are not raised by a footprint pass — its instances are counted,
 * not applied.  `probes` counts those lookups only.  info: level (the probed one), generated, viol_fp / viol_mask, viol_index = index of the violator's
 * PARENT in the newest level, pending = violating successors seen.  vsrmc_checker_probe_trace: Init .. violator.
 * On a sharded checker (world > 1) the call probes this rank's part of the newest level against this rank's part of the seen-set and
 * resolves nothing: a violating successor owned by another rank may be a state that rank has seen, so the candidates
 * (vsrmc_checker_probe_candidates) must be shown to their owners (vsrmc_checker_seen_batch there) — sharded.py: ShardedChecker.probe. */
int32_t vsrmc_checker_probe(vsrmc_checker* c, vsrmc_level_info* info);
/* Two levels beyond the last materialised one: level L+1 becomes a VIRTUAL level (fingerprints claimed, invariants checked, exact
 * count, no records), then the newest level is expanded a second time in slices — the successors that won their slot are written
 * to the idle next buffer and at once expanded in probe mode (level L+2), then dropped.  Costs one extra expansion of the newest
 * level and no memory beyond a slice.  virt: level L+1 (n_new exact); probe: level L+2.  A violation in either is reported there
 * (viol_index = index in the newest level of the violator's parent resp. grandparent); vsrmc_checker_probe_trace gives the
 * counter-example.  The search cannot continue afterwards. */
int32_t vsrmc_checker_probe2(vsrmc_checker* c, vsrmc_level_info* virt, vsrmc_level_info* probe);
/* the same one level deeper: level L+1 virtual, level L+2 streamed through scratch buffers (inserted into the seen-set, exact
 * count, never kept), level L+3 probed.  Level L is expanded twice, L+1 and L+2 once; scratch buffers of a quarter of the record
 * buffers' size are allocated for the call.  virt2->pending = (slices of level L) << 32 | sub-slices of level L+1.  A violation
 * in level L+1 or L+2 is reported in that level's info (a violating level is still completed; nothing deeper is reported);
 * vsrmc_checker_probe_trace reconstructs the counter-example in every case. */
int32_t vsrmc_checker_probe3(vsrmc_checker* c, vsrmc_level_info* virt1, vsrmc_level_info* virt2, vsrmc_level_info* probe);
/* The general form of the two calls above (≙ TLC going on with DiskStateQueue / DiskFPSet when the frontier outgrows memory; here
 * nothing leaves the HBM): ONE MORE LEVEL beyond the record buffers per call.  The first call after the last vsrmc_checker_step makes
 * level L+1 a virtual level (inserted->level = L+1, probed->level = 0).  Every further call descends from the newest materialised
 * level L — regenerating levels L+1 .. L+j-1 slice inside slice from the seen-set's predecessor keys, each state exactly once —
 * inserts level L+j (exact count, per-action counts, checksums, invariants; its records pass through a scratch buffer) and probes level
 * L+j+1 (probed->level).  The search rolls on past the memory horizon at about 2.2 x the expansions of a stored BFS until the
 * seen-set is full, a level comes back empty (inserted->n_new == 0: exhausted) or an invariant fails (viol_mask of whichever info;
 * vsrmc_checker_probe_trace reconstructs the counter-example).  inserted->pending = k_expand launches of the pass, ->materialize_ms =
 * kernel time spent regenerating, ->words_new = (slices of level L) << 32 | slices of the levels below it.  vsrmc_checker_step is
 * refused from the first call on (the seen-set holds levels that have no frontier) until the search has been RE-BASED: when the levels shrink again
 * (the analysis models after their peak) and the newest seen-set-only level and the one predicted after it fit the record buffers, vsrmc_checker_advance
 * spends one descent on regenerating that level INTO the idle record buffer (*what = 3: a = the level, unchanged figures) and the rest of the run is
 * ordinary stored levels.  vsrmc_checker_save works between any two calls; vsrmc_checker_reset starts over. */
int32_t vsrmc_checker_deepen(vsrmc_checker* c, vsrmc_level_info* inserted, vsrmc_level_info* probed);
/* One unit of progress of the AUTOMATIC level scheme — no level numbers and no sizes from the caller: an ordinary BFS level while
 * the next one is predicted to fit the idle record buffer (*what = 1, a = its info), otherwise vsrmc_checker_deepen (*what = 2,
 * a = the inserted level, b = the probed one or b->level == 0; *what = 3: no new level, the deep search was re-based onto level a->level,
 * see vsrmc_checker_deepen).  The prediction: a level grows by at most the factor the last one
 * grew by (the factor falls from level to level in these models, tests/golden/oracle_levels_*.json) and by at most one bag entry
 * per record.  vsrmc_check is the loop over this call; vsrmc_options with table_log2 = 0 / frontier_words = 0 / frontier_states = 0 /
 * pending_entries = 0 are sized from the free memory of the device. */
int32_t vsrmc_checker_advance(vsrmc_checker* c, vsrmc_level_info* a, vsrmc_level_info* b, int32_t* what);
/* No fatal mispredictions.  (i) A level vsrmc_checker_advance stored although it did not fit ("frontier full": the prediction above was wrong, or the
 * caller's own vsrmc_checker_step ran out of buffer) is not lost: k_expand goes on claiming, counting and checking after the buffers are exhausted, so
 * the seen-set holds the whole level — the NEXT vsrmc_checker_advance (or the same one) keeps it as a seen-set-only level (*what = 2, its figures and
 * checksums exact) and the search rolls on.  (ii) The seen-set: *state = 0 there is room for the next level, 1 = it has just been re-hashed into a
 * table of twice the slots (device memory permitting; vsrmc_checker_options shows the new table_log2), 2 = it is more than 85 % full and cannot grow:
 * the search is incomplete at the depth reached.  vsrmc_check asks before every unit of progress; loops over vsrmc_checker_advance should too. */
int32_t vsrmc_checker_room(vsrmc_checker* c, int32_t* state);
/* the (fingerprint, key) pairs of the violating successors the last vsrmc_checker_probe saw and did not find in this checker's
 * seen-set (duplicates included; *n = their number; pairs == NULL asks for the number only).  Sharded runs show them to their owners. */
int32_t vsrmc_checker_probe_candidates(vsrmc_checker* c, uint64_t* pairs, uint64_t cap_pairs, uint64_t* n);
/* The distinct violating STATES of the level the last vsrmc_checker_probe / _deepen / _advance probed (unsharded checkers): the fingerprints,
 * ascending, of the violating successors that are states of no earlier level — viol_fp of the probe's info is fps[0].  Lets a caller ask whether
 * a KNOWN violating state (the last state of the reference's state_transfer_violation_trace.txt:556-577) is among the ones the search met, not
 * only which one it reports.  fps == NULL asks for the number only. */
int32_t vsrmc_checker_probe_violators(vsrmc_checker* c, uint64_t* fps, uint64_t cap, uint64_t* n);
/* How many regenerating passes of the deep search this checker has run with the kernel of their own (csrc/vsr_regen_bits.hpp: VSR.tla with R <= 3, one rank,
 * the claim bitmap of the first seen-set-only level) since it was created; the others ran k_expand's regenerating instantiation.  The environment variable
 * VSRMC_NO_REGEN_KERNEL, read when the checker is created, keeps it at 0.  (Test knob, read the same way: VSRMC_REGEN_TRIP=N, 1 .. 64, the instances a wave
 * of that kernel takes per trip.) */
int32_t vsrmc_checker_regen_launches(const vsrmc_checker* c, uint64_t* n);
/* seen[i] = 1 if fps[i] is in this checker's seen-set as a state of a level below `level` (host arrays) */
int32_t vsrmc_checker_seen_batch(vsrmc_checker* c, const uint64_t* fps, uint64_t n, int32_t level, uint8_t* seen);
int32_t vsrmc_checker_probe_trace(vsrmc_checker* c, uint64_t* words, uint64_t cap_words, uint64_t* off, int32_t* actions,
                                  uint64_t cap_states, uint64_t* n_states);
/* ≙ TLCTrace.getTrace for a violating state of the CALLER's choice: the counter-example that ends in `fp`, one of vsrmc_checker_probe_violators (unsharded
 * checkers).  vsrmc_checker_probe_trace walks to the violator with the smallest fingerprint; the reference's own counter-example
 * (state_transfer_violation_trace.txt:555-577) ends in another violating state of the same level — this call prints the path the search took to THAT state,
 * so that the two action sequences can be laid side by side.  Same layout as vsrmc_checker_trace. */
int32_t vsrmc_checker_trace_to_violator(vsrmc_checker* c, uint64_t fp, uint64_t* words, uint64_t cap_words, uint64_t* off, int32_t* actions,
                                        uint64_t cap_states, uint64_t* n_states);

/* ---- a user's predicates on the levels beyond the record buffers -----------------------------------------------------------------------
 * vsrmc_checker_where_scan / _step_scan read stored levels only.  The levels beyond them (vsrmc_checker_deepen) exist as seen-set entries; their records
 * pass through scratch buffers while a descent regenerates or inserts them, each state exactly once per descent, and the level after the inserted one —
 * the probed level — has no records at all.  Programs ATTACHED to a checker are evaluated there, by every vsrmc_checker_deepen, and by every deepen
 * inside vsrmc_checker_advance / vsrmc_check, while they are attached: with the attachment a user's state predicates see every state the built-in
 * invariants see, and a user's step predicates every transition the search takes.  Nothing else changes: without an attachment every call, count and
 * exit code is what it was, and with one the search itself (level infos, checksums, violations) is untouched.
 * vsrmc_checker_deep_attach: state_prog (vsrmc_where_compile / vsrmc_predicates_compile) and / or step_prog (vsrmc_step_compile /
 *   vsrmc_step_predicates_compile); either may be NULL, both NULL detaches.  The programs are copied: the caller may destroy its own.  VSRMC_E_ARG for a
 *   step program in the state position and the reverse, and for a program compiled for another model; VSRMC_E_STATE on a sharded checker (world > 1) and
 *   on an exact_ties checker.  While programs are attached vsrmc_checker_probe2 / _probe3 are refused (VSRMC_E_STATE).
 *   Each seen-set-only level K is scanned EXACTLY ONCE, in the first descent after the attachment whose scratch buffers its records pass through: as a
 *   regenerated level (kind 0) or as the inserted level (kind 1), slice by slice; the figures of the slices of a level accumulate.  The first deepen call
 *   (the virtual level L+1) writes no records: its level is scanned when the next descent regenerates it, and a run that ends there has not examined it.
 *   The same rule covers an attachment made after the deep search has begun and one made after vsrmc_checker_load: every level beyond the newest stored
 *   one is scanned by the next descent.  The attachment is NOT part of a checkpoint (vsrmc_checker_save): attach again after loading.  A re-basing descent
 *   scans what it regenerates, like any other.  vsrmc_checker_reset keeps the attachment and forgets its results.
 *   State program: k_where over every slice.  Step program: k_step_list / k_step_apply over every slice = the transitions out of level K, those into the
 *   probed level included.  The probed level (kind 2; state program only — the search takes no transition out of it): k_probe_where
 *   (csrc/vsr_deep_where.hpp) evaluates the program on every successor of the inserted level's sub-slices that the seen-set does not hold, without writing
 *   a record; when the pass is over the collected copies that are states of the inserted level after all are dropped and the rest de-duplicated by
 *   fingerprint, the copy with the smallest key standing for the state (csrc/vsr_where_parse.hpp: departures).  A violation of a built-in invariant in
 *   the inserted level ends the examination there: that pass reports no probed level.
 * vsrmc_checker_deep_levels: the (level, probed) pairs that have results, ascending; levels == NULL asks for the number.  A level appears once as a
 *   scanned level (probed = 0) and, one pass earlier, once as the probed level (probed = 1).
 * vsrmc_checker_deep_result: the figures of one of them.  info->kind: 0 regenerated, 1 inserted, 2 probed.  w (may be NULL): vsrmc_where_info with
 *   count / min_fp exact for kinds 0 and 1; n_states = the level's states (kind 2: the successors the program ran over, copies of one state counted each).
 *   Kind 2: count[k] = DISTINCT states of the probed level that satisfy k; exact while the list of collected copies (2^20) did not overflow
 *   (info->exact = 1), otherwise lower bounds (exact = 0) — never reported as exact; min_fp[k] is then the smallest among the copies that were kept, not necessarily
 *   the level's smallest: a witness from it is a valid behaviour into a hit, but not the same one in every run.  s (may be NULL): vsrmc_step_info of the transitions out of the level
 *   (kinds 0 and 1), n_pairs + n_err == `generated` of the level after it; count / min_fp exact.  min_index has no meaning for a transient level (~0);
 *   min_ordinal / min_action are ~0 / -1: an ordinal is a position in the bag of the scratch record, which is gone (vsrmc_checker_deep_witness finds the
 *   instance again).  kernel_ms / where_ms / step_ms are HOST times around the launches of a program, their synchronisation included.
 * vsrmc_checker_deep_where_states / _deep_step_pairs: the hit lists of a level, in the order and under the contract of vsrmc_checker_where_states /
 *   _step_pairs (the first 2^20 that arrive are kept, *n is the true number, VSRMC_E_REP beyond; the test knobs VSRMC_WHERE_LIST_CAP, VSRMC_STEP_LIST_CAP
 *   and VSRMC_STEP_SLICE apply: the two caps are read at the attachment, the slice size at every slice; VSRMC_DEEP_INSTANCE_CAP=N, a test knob
 *   with no other use, lowers the 2^22 entries of the attachment's instance list to N >= 64, so that a sub-slice overflows it and is run again in halves).  The ordinals of the pairs are positions in the scratch records of THIS descent.  Lists are kept
 *   for the levels the last scanning descent scanned; an earlier level's list is dropped (VSRMC_E_STATE), its figures stay.  Kind 2 with exact = 0:
 *   VSRMC_E_REP, *n = the copies offered.
 * vsrmc_checker_deep_witness: a behaviour Init .. hit, the same one in every run; the layout of vsrmc_checker_trace.  which_program 0: the state with
 *   the smallest fingerprint of the scanned level that satisfies state predicate k (vsrmc_checker_trace_fp — which accepts seen-set-only levels).
 *   which_program 2: the same in the level as a PROBED level: the parent is the state of the level below whose fingerprint ends in the 45 bits the
 *   state's smallest key keeps (an ambiguous pointer is reported as by vsrmc_checker_trace_to_violator), then the state itself.  which_program 1: the
 *   behaviour into the parent with the smallest fingerprint that has a pair satisfying step predicate k, then the successor of the LOWEST-ORDINAL instance
 *   of the replayed parent record whose pair has bit k (n_states = level + 1, actions[level] its action id). */
typedef struct vsrmc_deep_info {
  int32_t level, kind;                             /* kind: 0 regenerated, 1 inserted, 2 probed */
  int32_t exact;                                   /* 1: every figure is exact; 0 (kind 2 only): the counts are lower bounds */
  int32_t has_state, has_step, reserved0;          /* which programs were evaluated on this level */
  uint64_t slices;                                 /* scratch slices of the level that were scanned */
  uint64_t n_hit_states, n_hit_pairs;              /* states / pairs with any bit set: what the list calls report as *n */
  double where_ms, step_ms;
} vsrmc_deep_info;
int32_t vsrmc_checker_deep_attach(vsrmc_checker* c, const vsrmc_where* state_prog, const vsrmc_where* step_prog);
int32_t vsrmc_checker_deep_levels(vsrmc_checker* c, int32_t* levels, int32_t* probed, uint64_t cap, uint64_t* n);
int32_t vsrmc_checker_deep_result(vsrmc_checker* c, int32_t level, int32_t probed, vsrmc_deep_info* info, vsrmc_where_info* w, vsrmc_step_info* s);
int32_t vsrmc_checker_deep_where_states(vsrmc_checker* c, int32_t level, int32_t probed, uint64_t* fps, uint8_t* bits, uint64_t cap, uint64_t* n);
int32_t vsrmc_checker_deep_step_pairs(vsrmc_checker* c, int32_t level, uint64_t* fps, uint32_t* ordinals, uint8_t* bits, uint64_t cap, uint64_t* n);
int32_t vsrmc_checker_deep_witness(vsrmc_checker* c, int32_t level, int32_t which_program, int32_t k, uint64_t* words, uint64_t cap_words, uint64_t* off,
                                   int32_t* actions, uint64_t cap_states, uint64_t* n_states);

/* The deadlock check on the levels beyond the record buffers (csrc/host_deep_terminal.hpp).  vsrmc_checker_terminal_scan reads the newest
 * STORED level and refuses a seen-set-only one; the TERMINAL ATTACHMENT makes the check reach as deep as the built-in invariants do.  It is independent of
 * vsrmc_checker_deep_attach and combines with it (k_step_list then runs once for each on a sub-slice of the inserted level: the lists are not shared).
 * Without the attachment every call, count and exit code is what it was; with it the search itself (level infos, checksums, violations) is untouched.
 * vsrmc_checker_deep_terminal_attach: VSRMC_E_STATE on a sharded checker (world > 1), on an exact_ties checker and while a state or an action constraint
 *   is attached (and those attachments are refused while this one is; vsrmc_checker_probe2 / _probe3 are refused as well).  A second attachment is a
 *   no-op.  Its buffers are allocated once, here: one TermCtl per level of a descent (512), two lists of 2^20 entries, an instance list of 2^22 entries,
 *   and the child chunk (2^26 words of records with their refs / fingerprints / keys); VSRMC_E_HIP when the device has no room, and nothing is changed.
 *   Each seen-set-only level K is scanned EXACTLY ONCE by k_terminal, in the first descent after the attachment whose scratch buffers its records pass
 *   through (the rule of vsrmc_checker_deep_attach, a late attachment, one after vsrmc_checker_load and a re-basing descent included), as a regenerated
 *   (kind 0) or the inserted level (kind 1).  The attachment is NOT part of a checkpoint; vsrmc_checker_reset keeps it and forgets its results.
 *   The probed level (kind 2) has no records: k_probe_children (csrc/vsr_deep_terminal.hpp) writes the successors of every sub-slice of the inserted level
 *   that the seen-set does not hold into the child chunk, chunk by chunk, and k_terminal reads each chunk.  When the pass is over the terminal copies that
 *   are states of the inserted level after all are dropped and the rest de-duplicated by fingerprint (the copy with the smallest key stands for the
 *   state).  A violation of a built-in invariant in the inserted level ends the examination there: that pass reports no probed level.
 * vsrmc_checker_deep_terminal_levels: the contract of vsrmc_checker_deep_levels.
 * vsrmc_checker_deep_terminal_result: kinds 0 and 1: every figure exact (n_terminal == `deadlocks` of the pass that expands the level).  Kind 2: n_states =
 *   the COPIES scanned (one state arrives from several parents); n_terminal / n_unsettled / the minima = DISTINCT states of the probed level, exact while the
 *   list of terminal copies did not overflow (exact = 1), otherwise lower bounds (exact = 0; n_listed = the copies offered).  ms / children_ms: HOST times
 *   around the launches (k_terminal and its read-back; kind 2: k_step_list + k_probe_children beside it), synchronisation included.
 * vsrmc_checker_deep_terminal_states: the contract of vsrmc_checker_terminal_states (fingerprints ascending, flag bytes; VSRMC_E_REP with *n = the true
 *   number when the list overflowed).  Lists of all scanned levels are kept.  Test knobs, read at the attachment: VSRMC_TERMINAL_LIST_CAP=N lowers the 2^20,
 *   VSRMC_DEEP_CHILD_WORDS=N the child chunk (at least 64 records of the largest size), so that a sub-slice
 *   takes several chunks; VSRMC_STEP_SLICE is read at every slice.
 * vsrmc_checker_deep_terminal_witness: the behaviour Init .. the terminal state (unsettled != 0: the unsettled terminal state) with the smallest
 *   fingerprint of that level, the layout of vsrmc_checker_trace.  Kinds 0 / 1: vsrmc_checker_trace_fp.  Kind 2: the parent named by the 45 bits the
 *   state's smallest key keeps, then the state (n_states = level). */
typedef struct vsrmc_deep_terminal_info {
  int32_t level, kind;                             /* kind: 0 regenerated, 1 inserted, 2 probed */
  int32_t exact, reserved0;                        /* 0 (kind 2 only): n_terminal / n_unsettled are lower bounds */
  uint64_t slices;                                 /* scratch slices scanned (kind 2: instance lists of sub-slices consumed) */
  uint64_t chunks;                                 /* k_terminal launches over records (kind 2: k_probe_children launches) */
  uint64_t n_states;                               /* states scanned (kind 2: n_copies) */
  uint64_t n_terminal, n_unsettled;
  uint64_t min_fp, min_fp_unsettled;               /* ~0 = none */
  uint64_t n_listed;                               /* what vsrmc_checker_deep_terminal_states reports as *n */
  uint64_t bytes_written;                          /* kind 2: bytes k_probe_children wrote (records, refs, fingerprints, keys) */
  double ms, children_ms;
} vsrmc_deep_terminal_info;
int32_t vsrmc_checker_deep_terminal_attach(vsrmc_checker* c);
int32_t vsrmc_checker_deep_terminal_levels(vsrmc_checker* c, int32_t* levels, int32_t* probed, uint64_t cap, uint64_t* n);
int32_t vsrmc_checker_deep_terminal_result(vsrmc_checker* c, int32_t level, int32_t probed, vsrmc_deep_terminal_info* info);
int32_t vsrmc_checker_deep_terminal_states(vsrmc_checker* c, int32_t level, int32_t probed, uint64_t* fps, uint8_t* flags, uint64_t cap, uint64_t* n);
int32_t vsrmc_checker_deep_terminal_witness(vsrmc_checker* c, int32_t level, int32_t probed, int32_t unsettled, uint64_t* words, uint64_t cap_words,
                                            uint64_t* off, int32_t* actions, uint64_t cap_states, uint64_t* n_states);

/* ≙ TLC's checkpoints (ModelChecker.checkpoint → FPSet.beginChkpt/commitChkpt, StateQueue and TLCTrace checkpoints; `-recover`):
 * one file holds the search between two levels — the occupied seen-set slots, the newest stored frontier, what the automatic level scheme
 * has learnt and, once the search has gone beyond the record buffers (vsrmc_checker_deepen), the descriptors of the levels that exist in
 * the seen-set only: a deep search is saved between two passes and recovered to make every later pass as the uninterrupted run would.  It is written
 * to <path>.tmp and renamed.  vsrmc_checker_load creates a checker with `o` (capacities and table size may differ from the
 * run that saved; the model constants may not) and continues where the checkpoint stopped.  Unsharded checkers only. */
int32_t vsrmc_checker_save(vsrmc_checker* c, const char* path);
/* where the search stands (after create / reset / load / step / advance): level = the newest STORED level, n_new = its states, reserved0 = the
 * number of levels beyond it that are complete in the seen-set only (depth = level + reserved0), frontier = states of the deepest complete
 * level, distinct, total_generated (both over every complete level) */
int32_t vsrmc_checker_status(vsrmc_checker* c, vsrmc_level_info* info);
int32_t vsrmc_checker_load(const vsrmc_model* m, const vsrmc_options* o, const char* path, vsrmc_checker** out);

/* ≙ tlc2.tool.ModelChecker.runTLC / Worker.run until the queue is empty, an invariant fails, a bound is hit or the spec raises an
 * evaluation error: vsrmc_checker_step in a loop.  stop_reason: 0 exhausted, 1 invariant violated (last->viol_*), 2 max_depth,
 * 3 max_seconds, 4 the seen-set is full, 5 a constraint is attached and the next level does not fit the record buffers (the levels beyond them are
 * not constrained: the search is incomplete at last->level; the reason is in vsrmc_last_error()); errors come back as the return code, with `last` describing the last completed level. */
int32_t vsrmc_check(vsrmc_checker* c, int32_t max_depth, double max_seconds, int32_t* stop_reason, vsrmc_level_info* last);

/* ---- StateQueue ≙ tlc2.tool.queue.StateQueue (sEnqueue(TLCState[]) / sDequeue(int) / size): a FIFO of state records kept in
 * HBM; batches cross the boundary in wire layout (words + n+1 offsets).  The checker keeps its own two frontier buffers; this
 * handle is the stand-alone queue for callers that drive the loop themselves (e.g. with vsrmc_expand_batch). */
typedef struct vsrmc_queue vsrmc_queue;
int32_t vsrmc_queue_create(int32_t device, uint64_t capacity_words, uint64_t capacity_states, vsrmc_queue** out);
int32_t vsrmc_queue_enqueue_batch(vsrmc_queue* q, const uint64_t* words, const uint64_t* off, uint64_t n);
int32_t vsrmc_queue_dequeue_batch(vsrmc_queue* q, uint64_t max_states, uint64_t* words, uint64_t cap_words, uint64_t* off,
                                  uint64_t* n);
int32_t vsrmc_queue_size(vsrmc_queue* q, uint64_t* n_states);
void vsrmc_queue_destroy(vsrmc_queue* q);

/* ---- simulation mode ≙ `tlc2.TLC -simulate` (the reference README:22 recommends it for the state-transfer defect) -------------
 * n_walkers random walks run concurrently (one GPU lane each): start at Init, up to max_depth steps chosen uniformly among
 * the enabled (action, binding) instances, invariants checked after every step, restart at the depth limit or in a terminal
 * state.  Stops at the first violation or after max_seconds.  The violating walk comes back as ordinals; pass them to
 * vsrmc_model_replay for the states and action names. */
typedef struct vsrmc_sim_result {
  int32_t found;                 /* 1 = invariant violated, 2 = evaluation / representation error on a walk, 0 = time-out */
  int32_t viol_mask;             /* violated invariants (found = 1) or device error code (found = 2) */
  int32_t viol_steps;            /* number of steps of the reported walk (trace = viol_steps + 1 states) */
  int32_t reserved;
  uint64_t steps, walks;         /* totals over all walkers */
  double seconds;
  uint32_t ords[512];
} vsrmc_sim_result;
int32_t vsrmc_simulate(const vsrmc_model* m, int32_t device, uint32_t n_walkers, int32_t max_depth, uint64_t seed,
                       double max_seconds, vsrmc_sim_result* out);

/* ---- simulation mode with the user's own predicates on every walk (csrc/vsr_sim_where.hpp: k_simulate_where) ----------------------
 * The state predicates (vsrmc_predicates_compile) and step predicates (vsrmc_step_predicates_compile) of the sections above, evaluated on random walks
 * instead of stored BFS levels: walks reach the depths no level is ever stored at.  Either program may be NULL, not both.  vsrmc_simulate is unchanged.
 * THE ITERATION CONTRACT.  A launch ("round") is 64 iterations of every walker.  In one iteration a walker does exactly one of two things:
 *   start  it has no walk yet, or its depth equals max_depth, or its state has no enabled instance: it puts Init into its record.  The state program
 *          is evaluated on Init.  No random draw is taken.
 *   step   one draw of the walker's generator (xorshift64*: x ^= x >> 12; x ^= x << 25; x ^= x >> 27; draw = x * 0x2545F4914F6CDD1D; walker i's
 *          initial x is the i-th output of the splitmix64 stream that starts at `seed`, 1 if that is 0 — exactly vsrmc_simulate's); pick = draw % total
 *          over the enabled (action, binding) instances in ordinal order; the instance is generated; the STEP program is evaluated on the pair (state,
 *          successor) BEFORE the walker moves; the walker moves; the STATE program is evaluated on the state it now stands on; the built-in invariants
 *          are checked as in vsrmc_simulate.
 *   Without a stop every walker evaluates one state per iteration: n_states == steps + walks == 64 * rounds * n_walkers, and n_pairs == steps.
 * count_state[k] / count_step[k]: the states / pairs that satisfy exported predicate k of the state / step program — exact.
 * stop = 1: the run ends at the first state or pair with any bit set, or the first violated built-in invariant; found says which (of several in one
 *   iteration of one walker: the step program, then the state program, then the invariants), viol_mask the bits, ords[0 .. viol_steps) the walk — for
 *   found = 4 it INCLUDES the offending step; found = 3 with viol_steps == 0: Init itself satisfies the predicate.  vsrmc_model_replay gives the states.
 *   The counts are then those of the rounds up to and including the one that stopped (other walkers were cut short in it).
 * stop = 0: count only (the report mode); the built-in invariants are not a stop reason.  An evaluation / representation error on a walk ends
 *   the run in either mode (found = 2).
 * max_rounds > 0: the run ends after exactly that many launches and the clock is not consulted — every count is then the same in every run with the same
 *   seed, each walker's path depending on its own generator only.  max_rounds = 0: launches until max_seconds have passed, as vsrmc_simulate.
 * Refused with VSRMC_E_ARG before any device is looked at: both programs NULL; a step program as state_prog or a state program as step_prog; a program
 * "compiled for another model"; max_depth outside 1..512.
 * Where this departs from the stored-level scans: a walk has no VIEW representative — the aux variables a state program reads are the walk's own. */
typedef struct vsrmc_sim_where_result {
  int32_t found;            /* 0 none, 1 built-in invariant, 2 error, 3 state predicate, 4 step predicate */
  int32_t viol_mask;        /* found 1/2: as vsrmc_sim_result; found 3/4: the predicate bits of the hit */
  int32_t viol_steps;
  uint64_t steps, walks, rounds;
  uint64_t n_states, n_pairs;              /* evaluations of each program */
  uint64_t count_state[8], count_step[8];
  double seconds;
  uint32_t ords[512];
} vsrmc_sim_where_result;
int32_t vsrmc_simulate_where(const vsrmc_model* m, int32_t device, const vsrmc_where* state_prog, const vsrmc_where* step_prog,
                             int32_t stop, uint32_t n_walkers, int32_t max_depth, uint64_t seed,
                             double max_seconds, uint64_t max_rounds, vsrmc_sim_where_result* out);

/* ---- simulation mode under a state constraint and / or an action constraint (csrc/vsr_sim_constrain.hpp: k_simulate_constrained) -----
 * [TLC-RECALLED] TLC's simulator honours CONSTRAINT and ACTION_CONSTRAINT: a walk moves only along permitted transitions into in-model states.  The
 * constrained BFS (vsrmc_checker_constrain_attach, vsrmc_checker_action_constrain_attach) ends with the stored levels; walks go to any depth.
 * vsrmc_simulate and vsrmc_simulate_where are unchanged.
 * state_prog (vsrmc_predicates_compile, may be NULL): its export state_constraint (an index, or -1 for none) is the state constraint, every other
 *   export is a query as in vsrmc_simulate_where.  step_prog (vsrmc_step_predicates_compile, may be NULL) / step_constraint: the same for the action
 *   constraint.  At least one of the two constraints must be given.  The constraint exports are counted like the others and never stop a run.
 * Every walker keeps a TRIED SET: the enabled instances of the state it stands on, by position in ordinal order, that it has drawn and was refused.  It
 *   is cleared when the walker moves or starts and kept between launches.  It holds 256 positions; a state with more enabled instances ends the run
 *   with found = 2, viol_mask = VSRMC_SIM_ERR_TRIED_WIDTH.
 * THE ITERATION CONTRACT.  A launch ("round") is 64 iterations of every walker.  In one iteration a walker does exactly one of four things:
 *   start    it has no walk yet, or its depth equals max_depth, or its state has no enabled instance, or every enabled instance has been tried (counted
 *            in `stuck`: the state is terminal in the constrained model): Init goes into its record, the tried set is cleared.  The state program is
 *            evaluated on Init and its bits are counted.  No random draw is taken.
 *   Otherwise it TRIES: one draw of the walker's generator (xorshift64* seeded as in vsrmc_simulate / vsrmc_simulate_where); pick = draw % (total -
 *            |tried|) over the UNTRIED enabled instances in ordinal order; the instance is generated (an evaluation error ends the run, found = 2); the
 *            step program is evaluated on the pair (state, successor) before any move.
 *   blocked  the step_constraint bit is false: the instance is marked tried, `blocked` + 1; nothing else is evaluated or counted, the walker stays.
 *   Otherwise the walker moves on trial and the state program is evaluated on the successor.
 *   pruned   the state_constraint bit is false: the walker is put back, the instance is marked tried, `pruned` + 1; its depth is unchanged and the bits of
 *            both programs are counted nowhere.  With stop = 1 the state bits in pruned_stop_mask (found = 3), then the built-in invariants of that
 *            successor (found = 1), end the run: ords[0 .. viol_steps) INCLUDES the step into the pruned state — the constrained BFS checks -invariant
 *            names and the built-in invariants on pruned states too.  pruned_stop_mask = 0: a pruned state's predicates stop nothing.
 *   step     the move stands: steps, n_pairs (a step program is present) and n_states (a state program is present) + 1, the bits of both programs are
 *            counted, the tried set is cleared.  With stop = 1: step queries (found = 4), state queries (3), built-in invariants (1), in this order.
 *   Drawing without replacement up to the first acceptance is uniform over the permitted transitions into in-model states, and a state is left, or
 *   found stuck, within `total` iterations.
 * Without a stop: steps + walks + blocked + pruned == 64 * rounds * n_walkers; n_states == steps + walks and count_state[state_constraint] == n_states
 *   (a state program is present); n_pairs == steps and count_step[step_constraint] == n_pairs (a step program is present).  With max_rounds > 0 every
 *   count is the same in every run with the same seed.
 * Init fails the state constraint: nothing is launched and no device is looked at — init_pruned = 1, walks = 0, found = 0, return code 0.
 * Refused with VSRMC_E_ARG before any device is looked at: neither constraint given; an index the program does not export (or no program to export it);
 *   a step program as state_prog or a state program as step_prog; a program "compiled for another model"; a constraint's program that reads aux_svc or
 *   aux_client_acked (the rule of vsrmc_checker_constrain_attach: the walk's model is the constrained search's); max_depth outside 1..512; no walkers. */
#define VSRMC_SIM_ERR_TRIED_WIDTH 40   /* found = 2: a state has more enabled instances than the tried set has positions (256) */
typedef struct vsrmc_sim_constrained_result {
  int32_t found;            /* 0 none, 1 built-in invariant, 2 error, 3 state predicate, 4 step predicate */
  int32_t viol_mask;        /* found 1/2: as vsrmc_sim_result; found 3/4: the predicate bits of the hit */
  int32_t viol_steps;
  uint64_t steps, walks, rounds;
  uint64_t n_states, n_pairs;              /* evaluations of each program that are counted: states stood on, pairs taken */
  uint64_t count_state[8], count_step[8];
  double seconds;
  uint32_t ords[512];
  uint64_t blocked, pruned, stuck;         /* tries the action constraint / the state constraint refused; starts out of a state with every instance tried */
  int32_t init_pruned;                     /* 1: Init fails the state constraint — nothing was walked */
  int32_t reserved0;
} vsrmc_sim_constrained_result;
int32_t vsrmc_simulate_constrained(const vsrmc_model* m, int32_t device, const vsrmc_where* state_prog, int32_t state_constraint,
                                   const vsrmc_where* step_prog, int32_t step_constraint, uint32_t pruned_stop_mask, int32_t stop, uint32_t n_walkers,
                                   int32_t max_depth, uint64_t seed, double max_seconds, uint64_t max_rounds, vsrmc_sim_constrained_result* out);

/* ---- sharded seen-set (≙ tlc2.tool.fp.MultiFPSet across GPUs): the phases of one BFS level -----------------------
 * world ranks, one per GPU; owner(fp) = ((fp >> 40) & 0xFFFFFF) % world.  The caller (vsr_tlaplus_amd/sharded.py over
 * torch.distributed / RCCL) owns the exchange buffers and moves them between ranks; every pointer is a device pointer.
 *   1. vsrmc_shard_expand       expand the local frontier; local-owner candidates are claimed at once, the others are
 *                               bucketed per owner as (fp, key) pairs in io->cand_send; returns the bucket sizes
 *   2. [all-to-all of the buckets]
 *   3. vsrmc_shard_claim        claim the received candidates in the local shard, then answer each with 1 = "won its slot"
 *   4. [all-to-all of the verdict bytes, back to the generators]
 *   5. vsrmc_shard_materialize  every winner (local owner or remote verdict) is rebuilt into THIS rank's next frontier:
 *                               records stay with their generator, only candidates and verdicts cross ranks
 *   6. vsrmc_shard_count        valid states / index range of the local next frontier; the caller compares the ranks and,
 *                               when they are out of balance, moves records in bulk:
 *      vsrmc_shard_export       copy the valid records of an index window into send streams and invalidate them here
 *      [all-to-all of the streams]
 *      vsrmc_shard_append       per received stream: copy into the next frontier, publish refs / fps
 *   7. vsrmc_shard_commit       swap the frontiers; local statistics (the caller all-reduces them)
 * With exact_ties = 0 (default) the levels are single-pass: in step 1 a successor owned by another rank that passes this
 * rank's sent-filter (exact repeats are dropped there) is written to the local next frontier SPECULATIVELY and announced;
 * in step 3 the candidate that inserts the fingerprint wins; step 5 only withdraws the announced successors that lost.
 * With exact_ties = 1 step 5 rebuilds the winners (k_materialize) and same-level ties follow the oracle's rule.
 *
 * Replicated phase: a sharded checker starts with Init on EVERY rank.  While the frontier is small the ranks explore whole
 * levels on their own, without any exchange (vsrmc_shard_local_step = vsrmc_checker_step on this rank's private copy;
 * every rank sees the same state sets, trace keys carry the local rank).  vsrmc_shard_partition ends that phase: each
 * rank keeps the states of the current frontier it owns and the sharded protocol above takes over.  (The early
 * fingerprints then sit in every rank's table, owners included, which is all the protocol needs.) */
int32_t vsrmc_shard_local_step(vsrmc_checker* c, vsrmc_level_info* info);
int32_t vsrmc_shard_partition(vsrmc_checker* c, uint64_t* n_kept);
/* after vsrmc_shard_commit / _local_step: the largest bag (vsrmc_level_info.max_bag) of the new level over ALL ranks, so that the next
 * expansion can size its LDS record slots for the level (optional; without it the format's worst case is used) */
int32_t vsrmc_shard_set_max_bag(vsrmc_checker* c, uint64_t max_bag);
typedef struct vsrmc_shard_io {
  uint64_t* cand_send;           /* [world][cand_cap][2]  (fp, key) */
  uint64_t cand_cap;             /* entries per owner */
} vsrmc_shard_io;
int32_t vsrmc_shard_expand(vsrmc_checker* c, const vsrmc_shard_io* io, uint64_t* cand_counts);
int32_t vsrmc_shard_claim(vsrmc_checker* c, const uint64_t* d_cand_recv, uint64_t n, uint8_t* d_verdict);
int32_t vsrmc_shard_materialize(vsrmc_checker* c, const vsrmc_shard_io* io, const uint8_t* d_verdict_in /* [world][cand_cap] */);
int32_t vsrmc_shard_count(vsrmc_checker* c, uint64_t* n_valid, uint64_t* n_range);
/* streams: d_words (device layout records, contiguous), d_off (ref = word offset in d_words << 8 | length), d_fp */
int32_t vsrmc_shard_export(vsrmc_checker* c, uint64_t first, uint64_t n, uint64_t* d_words, uint64_t words_cap, uint64_t* d_off,
                           uint64_t* d_fp, uint64_t cap, uint64_t* n_out, uint64_t* words_out);
int32_t vsrmc_shard_append(vsrmc_checker* c, const uint64_t* d_words, uint64_t n_words, const uint64_t* d_off,
                           const uint64_t* d_fp, uint64_t n);
int32_t vsrmc_shard_commit(vsrmc_checker* c, vsrmc_level_info* info);

/* ---- the level loop of a sharded run, natively (csrc/vsr_shard_loop.hpp) ≙ TLC's distributed mode (TLCServer / TLCWorker / FPSet servers)
 * The loop sequences the phases above on one rank and talks to the other ranks through a vsrmc_comm: two functions and a flag.
 *   alltoallv  element p of every array = peer p; `send + send_offs[p] * elem_bytes` holds send_counts[p] elements for p, what p sends
 *              arrives at `recv + recv_offs[p] * elem_bytes` (recv_counts[p] elements, known to the caller); nothing is ever addressed to
 *              oneself.  host_buffers = 0: the pointers are DEVICE memory and `stream` is the hipStream_t to order the transfer on (the
 *              function returns when it has completed); host_buffers = 1: HOST memory, stream = NULL (the loop stages the buckets).
 *   allgather  `bytes` of host memory from every rank, rank order, blocking.
 * Return 0, or non-zero on failure.  vsrmc_comm_rccl_* is the RCCL transport (grouped ncclSend / ncclRecv over xGMI; librccl is
 * dlopen'ed on first use): rank 0 makes the 128-byte id, the caller's bootstrap (torch.distributed, MPI, a file) hands it to every rank. */
typedef struct vsrmc_comm {
  void* ctx;
  int32_t rank, world;
  int32_t host_buffers;
  int32_t reserved0;
  int32_t (*alltoallv)(void* ctx, const void* send, const uint64_t* send_counts, const uint64_t* send_offs, void* recv,
                       const uint64_t* recv_counts, const uint64_t* recv_offs, uint32_t elem_bytes, void* stream);
  int32_t (*allgather)(void* ctx, const void* send, void* recv, uint32_t bytes);
} vsrmc_comm;
int32_t vsrmc_comm_rccl_unique_id(uint8_t* id128);
int32_t vsrmc_comm_rccl_create(const uint8_t* id128, int32_t rank, int32_t world, int32_t device, vsrmc_comm** out);
void vsrmc_comm_rccl_destroy(vsrmc_comm* comm);

typedef struct vsrmc_shard_loop vsrmc_shard_loop;
/* c: a sharded checker (vsrmc_options.world / rank, exact_ties = 0) in its initial state; cand_cap: (fp, key) candidates per peer and
 * level; rec_cap / rec_words_cap: records / words one rebalancing round may move; replicate_below: levels with fewer new states are
 * explored by every rank on its own (0 / 1: sharded from Init on).  The comm struct is copied; its ctx must outlive the loop. */
int32_t vsrmc_shard_loop_create(vsrmc_checker* c, const vsrmc_comm* comm, uint64_t cand_cap, uint64_t rec_cap, uint64_t rec_words_cap,
                                uint64_t replicate_below, vsrmc_shard_loop** out);
void vsrmc_shard_loop_destroy(vsrmc_shard_loop* l);
/* one BFS level on every rank (collective): global = the level's figures over all ranks (viol_fp = smallest violating fingerprint of
 * any rank, ~0 if none; n_new == 0: exhausted), local = this rank's own */
int32_t vsrmc_shard_loop_step(vsrmc_shard_loop* l, vsrmc_level_info* global, vsrmc_level_info* local);
/* ≙ vsrmc_check: stop_reason 0 exhausted, 1 invariant violated, 2 max_depth */
int32_t vsrmc_shard_loop_run(vsrmc_shard_loop* l, int32_t max_depth, int32_t stop_on_violation, int32_t* stop_reason, vsrmc_level_info* last);
/* the seen-set shards before the next vsrmc_shard_loop_advance (collective once the run is sharded): *state = 0 room on every rank, 2 = some rank's shard
 * is more than 85 % full — every rank learns it in the same call and all of them stop together ("incomplete at depth N"); loops over
 * vsrmc_shard_loop_advance ask before every call, vsrmc_shard_loop_run does.  Round 6: the winner set of a sharded deep search counts too — it is re-hashed
 * into twice the slots here when the next level is expected to take it past 60 % (while the device has the memory) and answers 2 when that level cannot fit;
 * after an answer of 2 vsrmc_last_error() names the set and its fill on this rank (the call itself returns 0) */
int32_t vsrmc_shard_loop_room(vsrmc_shard_loop* l, int32_t* state);
/* Since round 6 a sharded level of 2^20 states per rank or more runs in SLICES with the exchange overlapped: the all-to-all of slice k's (fp, key)
 * candidates, the owners' claims, the verdict bytes and the withdrawal of the losers run on a second stream and a second set of buckets while k_expand of
 * slice k + 1 runs (VSRMC_OVERLAP=0: the sequential level of rounds 2-5; VSRMC_OVERLAP_MIN_STATES / _MIN_SLICES: when and how finely).  What a level
 * leaves does not depend on the slicing.  *levels / *slices: how many levels ran that way so far, in how many slices. */
int32_t vsrmc_shard_loop_overlap_stats(vsrmc_shard_loop* l, uint64_t* levels, uint64_t* slices);
/* ≙ TLC's checkpoints for a sharded run (collective; between two vsrmc_shard_loop_advance calls — also once the search has gone beyond the ranks' record
 * buffers: the seen-set-only levels' descriptors and each rank's winner set travel in its shard file).  Every rank writes <prefix>.rank<r>of<w> (its checker:
 * vsrmc_checker_save) and <prefix>.rank<r>of<w>.loop (the loop's own state), in two phases: a failure on any rank leaves the previous checkpoint whole.
 * Recover: vsrmc_checker_load of the rank's own shard file, then vsrmc_shard_loop_restore over it (every rank must have loaded the same depth). */
int32_t vsrmc_shard_loop_save(vsrmc_shard_loop* l, const char* prefix);
int32_t vsrmc_shard_loop_restore(vsrmc_checker* c, const vsrmc_comm* comm, uint64_t cand_cap, uint64_t rec_cap, uint64_t rec_words_cap, const char* prefix,
                                 vsrmc_shard_loop** out);
/* vsrmc_checker_deepen / vsrmc_checker_advance for a sharded run (collective; figures over all ranks): levels beyond the ranks' record
 * buffers live in the ranks' seen-sets only and are regenerated from the newest stored level; every pass of the descent is the
 * protocol of a sharded level with other sources and targets (csrc/vsr_shard_loop.hpp).  advance: an ordinary sharded level while EVERY
 * rank predicts that its part of the next one fits, else deepen.  vsrmc_shard_loop_run is the loop over advance (stop_reason 4: a
 * rank's seen-set is 85 % full). */
int32_t vsrmc_shard_loop_deepen(vsrmc_shard_loop* l, vsrmc_level_info* inserted, vsrmc_level_info* probed);
int32_t vsrmc_shard_loop_advance(vsrmc_shard_loop* l, vsrmc_level_info* a, vsrmc_level_info* b, int32_t* what);
/* the fingerprints of the counter-example of a violation a probe pass found (collective), Init first; *n = its length */
int32_t vsrmc_shard_loop_probe_trace_fps(vsrmc_shard_loop* l, uint64_t* fps, int32_t cap, int32_t* n);
int32_t vsrmc_shard_loop_status(vsrmc_shard_loop* l, int32_t* level, uint64_t* distinct, uint64_t* n_frontier, int32_t* replicated,
                                uint64_t* viol_fp, int32_t* viol_mask, int32_t* viol_level, uint64_t* moved, uint64_t* bytes_sent);
/* TLCTrace.getTrace across ranks (collective): fps[0 .. level) = fingerprints of the path Init -> the level-`level` state `fp`;
 * vsrmc_model_replay_fps re-executes it on one GPU */
int32_t vsrmc_shard_loop_trace_fps(vsrmc_shard_loop* l, int32_t level, uint64_t fp, uint64_t* fps);

#ifdef __cplusplus
}
#endif
#endif
