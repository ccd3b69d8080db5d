"""Host-side mirror of the TLC interfaces this path replaces, over the C ABI (include/vsrmc.h):

    Model         tlc2.tool.impl.Tool / ModelConfig   — (VSR.tla, VSR.cfg) lowered; getNextStates(batch)
    FPSet         tlc2.tool.fp.FPSet                  — put / contains / putBlock / containsBlock / size / close
    ModelChecker  tlc2.tool.ModelChecker + Worker.run + StateQueue + TLCTrace — level-synchronous BFS on the GPU

Everything below is plumbing: all model semantics, hashing and set operations run in the HIP kernels.
"""
import ctypes as C
import os

import numpy as np

from . import capi
from .capi import VsrmcError, check

ACTION_NAMES = ["Initial predicate", "TimerSendSVC", "ReceiveHigherSVC", "ReceiveMatchingSVC", "SendDVC",
                "ReceiveHigherDVC", "ReceiveMatchingDVC", "SendSV", "ReceiveSV", "ReceiveClientRequest",
                "ReceivePrepareMsg", "ReceivePrepareOkMsg", "ExecuteOp", "SendGetState", "ReceiveGetState",
                "ReceiveNewState"]          # Next order, VSR.tla:896-913

INV_ACK_NOT_LOST = 1           # AcknowledgedWriteNotLost           VSR.tla:945-950
INV_ACK_ON_MAJORITY = 2        # AcknowledgedWritesExistOnMajority  VSR.tla:937-943


def _p(a):
    return C.c_void_p(a.ctypes.data)


class Where:
    """State predicates compiled for one model (Model.compile_where), or step predicates (Model.compile_step: `step` is True; they run over
    (state, successor) pairs): `names[k]` is the exported predicate of bit k."""

    def __init__(self, handle, model):
        self._h = handle
        self.model = model                                            # (keeps the model alive)
        d = self.describe()
        self.names, self.step = d["names"], d["step"]

    def describe(self):
        """-> dict(names, n_ops, depth, msg_loops, n_bodies, step): the exported names, program length, operand-stack depth, nesting of the message
        quantifiers that remain as loops, quantifier bodies after unfolding, whether it is a step program."""
        d = capi.WhereDesc()
        check(capi.load().vsrmc_where_describe(self._h, C.byref(d)))
        return dict(names=[d.names[k].value.decode() for k in range(d.n_names)], n_ops=d.n_ops, depth=d.depth, msg_loops=d.msg_loops, n_bodies=d.n_bodies,
                    step=bool(d.step))

    def close(self):
        if self._h:
            capi.load().vsrmc_where_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Model:
    """The lowered (VSR.tla, VSR.cfg) pair."""

    def __init__(self, handle):
        self._h = handle
        lay = capi.Layout()
        check(capi.load().vsrmc_model_info(self._h, C.byref(lay)))
        self.layout = lay

    @classmethod
    def load(cls, cfg_path, tla_path=None):
        """≙ `tlc2.TLC -config VSR.cfg VSR.tla`: reads the cfg grammar of VSR.cfg:1-39."""
        h = C.c_void_p()
        check(capi.load().vsrmc_model_load(tla_path.encode() if tla_path else None, cfg_path.encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def from_constants(cls, R=3, C_=1, n=2, L=2, restart_limit=0, symmetry=True, invariant_mask=1,
                       assume_commit_number=False):
        h = C.c_void_p()
        check(capi.load().vsrmc_model_from_constants(R, C_, n, L, restart_limit, int(symmetry), invariant_mask,
                                                     int(assume_commit_number), C.byref(h)))
        return cls(h)

    @classmethod
    def second_model(cls, R=3, n=2, L=2, no_progress_limit=0, symmetry=False, invariant_mask=14):
        """analysis/03-state-transfer/VR_STATE_TRANSFER.tla under the constants of its cfg (the shipped one: 3, {v1,v2}, 2, 0;
        INVARIANT AcknowledgedWritesExistOnMajority, NoLogDivergence, CommitNumberNeverHigherThanOpNumber = mask 14)."""
        h = C.c_void_p()
        check(capi.load().vsrmc_model2_from_constants(R, n, L, no_progress_limit, int(symmetry), invariant_mask, C.byref(h)))
        return cls(h)

    @classmethod
    def third_model(cls, R=3, n=2, L=2, no_progress_limit=0, symmetry=False, invariant_mask=30):
        """analysis/04-application-state/VR_APP_STATE.tla under the constants of its cfg (the shipped one: 3, {a,b}, 2, 0; INVARIANT
        AcknowledgedWritesExistOnMajority, NoLogDivergence, NoAppStateDivergence, CommitNumberNeverHigherThanOpNumber = mask 30)."""
        h = C.c_void_p()
        check(capi.load().vsrmc_model3_from_constants(R, n, L, no_progress_limit, int(symmetry), invariant_mask, C.byref(h)))
        return cls(h)

    def set_fp_seed(self, seed):
        """Second-hash audit (TLC: a rerun under another -fp N): `seed` is xor-ed into every salt of the view hash.  Seed 0 is the
        function of the committed fixtures; under any other seed fingerprints and checksums change, counts must not.  Checkers
        created afterwards see it (a checker copies the model).  Returns self."""
        check(capi.load().vsrmc_model_set_fp_seed(self._h, C.c_uint64(int(seed) & (2 ** 64 - 1))))
        return self

    @property
    def fp_seed(self):
        return int(capi.load().vsrmc_model_fp_seed(self._h))

    def init_state(self):
        out = np.zeros(256, dtype=np.uint64)
        n = C.c_int32()
        check(capi.load().vsrmc_model_init_state(self._h, _p(out), 256, C.byref(n)))
        return out[: n.value].copy()

    def format_state(self, rec):
        rec = np.ascontiguousarray(rec, dtype=np.uint64)
        n = C.c_int64()
        check(capi.load().vsrmc_model_format_state(self._h, _p(rec), None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        check(capi.load().vsrmc_model_format_state(self._h, _p(rec), buf, n.value, C.byref(n)))
        return buf.value.decode()

    def get_next_states(self, words, off, device=0, cap_succ=None, cap_words=None):
        """Tool.getNextStates over all actions for a batch of states.
        -> list of dict(parent, ordinal, action, fp, auxkey, inv, err, words)."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        cap_succ = cap_succ or max(64, 48 * n)
        cap_words = cap_words or cap_succ * int(self.layout.max_record_words)
        ow = np.zeros(cap_words, dtype=np.uint64)
        om = np.zeros(8 * cap_succ, dtype=np.uint64)
        n_out, w_out = C.c_uint64(), C.c_uint64()
        check(capi.load().vsrmc_expand_batch(self._h, device, _p(words), _p(off), n, _p(ow), cap_words, _p(om), cap_succ,
                                             C.byref(n_out), C.byref(w_out)))
        out = []
        offs = [int(om[8 * k + 7]) for k in range(n_out.value)] + [w_out.value]
        for k in range(n_out.value):
            m = om[8 * k: 8 * k + 8]
            out.append(dict(parent=int(m[0]), ordinal=int(m[1]), action=int(m[2]), fp=int(m[3]), auxkey=int(m[4]),
                            inv=int(m[5]), err=int(m[6]), words=ow[offs[k]: offs[k + 1]].copy()))
        return out

    def fingerprints(self, words, off, device=0):
        """TLCState.fingerPrint (VIEW + SYMMETRY) of a batch of states -> (fps, auxkeys)."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        fps = np.zeros(n, dtype=np.uint64)
        aks = np.zeros(n, dtype=np.uint32)
        check(capi.load().vsrmc_fingerprint_batch(self._h, device, _p(words), _p(off), n, _p(fps), _p(aks)))
        return fps, aks

    def terminal_flags(self, words, off, device=0):
        """One flag byte per state of a batch (k_terminal, guards only): bit 0 = terminal — no (action, binding) instance is enabled (TLC's
        deadlock); bit 1 = unsettled — AllReplicasMoveToSameView (VSR.tla:958-962) is false."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        flags = np.zeros(max(1, n), dtype=np.uint8)
        check(capi.load().vsrmc_terminal_batch(self._h, device, _p(words), _p(off), n, _p(flags)))
        return flags[:n]

    def compile_where(self, text):
        """State predicates (csrc/vsr_where_parse.hpp: one expression or `Name == expr` definitions in TLA+ syntax) -> Where.  Needs no device.
        Raises VsrmcError with "line:col: reason" for a text that is refused."""
        h = C.c_void_p()
        check(capi.load().vsrmc_where_compile(self._h, text.encode() if isinstance(text, str) else text, C.byref(h)))
        return Where(h, self)

    def compile_predicates(self, text):
        """State predicates for ANY model -> Where.  A VSR.tla model: exactly compile_where's program.  second_model / third_model: the same language
        over that spec's variables (csrc/vsr_where_parse.hpp).  Needs no device.  Raises VsrmcError with "line:col: reason" for a text that is refused."""
        h = C.c_void_p()
        check(capi.load().vsrmc_predicates_compile(self._h, text.encode() if isinstance(text, str) else text, C.byref(h)))
        return Where(h, self)

    def where_flags(self, w, words, off, device=0):
        """One byte per state of a batch (k_where): bit k = exported predicate k of `w` holds."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        flags = np.zeros(max(1, n), dtype=np.uint8)
        check(capi.load().vsrmc_where_batch(self._h, device, w._h, _p(words), _p(off), n, _p(flags)))
        return flags[:n]

    def compile_step(self, text):
        """Step predicates (csrc/vsr_where_parse.hpp: the language of compile_where plus primed variables, UNCHANGED and step_action) -> Where with
        step == True.  Needs no device.  Raises VsrmcError with "line:col: reason" for a text that is refused."""
        h = C.c_void_p()
        check(capi.load().vsrmc_step_compile(self._h, text.encode() if isinstance(text, str) else text, C.byref(h)))
        return Where(h, self)

    def compile_step_predicates(self, text):
        """Step predicates for ANY model -> Where with step == True.  A VSR.tla model: exactly compile_step's program.  second_model / third_model: the
        step language over that spec's variables (csrc/vsr_where_parse.hpp).  Needs no device.  Raises VsrmcError with "line:col: reason" for a text
        that is refused."""
        h = C.c_void_p()
        check(capi.load().vsrmc_step_predicates_compile(self._h, text.encode() if isinstance(text, str) else text, C.byref(h)))
        return Where(h, self)

    def step_flags(self, w, words, off, device=0):
        """The step predicates of `w` on every transition out of a batch of states (k_step_list, k_step_apply) -> an (n, 5) uint64 array, one row
        [parent, ordinal, action, bits, err] per generated successor in (parent, ordinal) order: the rows of get_next_states, row for row.  A row
        with err != 0 (the action raises an evaluation error) was not evaluated: bits 0."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        lib = capi.load()
        total = C.c_uint64()
        check(lib.vsrmc_step_batch(self._h, device, w._h, _p(words), _p(off), n, None, 0, C.byref(total)))
        rows = np.zeros((max(1, total.value), 5), dtype=np.uint64)
        check(lib.vsrmc_step_batch(self._h, device, w._h, _p(words), _p(off), n, _p(rows), len(rows), C.byref(total)))
        return rows[: total.value]

    def tlc_fingerprints(self, words, off, device=0):
        """TLC's own fingerprint (tlc2.util.FP64 over Value.fingerPrint of `view`; [TLC-RECALLED], csrc/vsr_tlcfp.hpp) of a batch of states,
        computed on the GPU.  With SYMMETRY: of the permuted state TLC picks (tlc_min_permutation)."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        fps = np.zeros(n, dtype=np.uint64)
        check(capi.load().vsrmc_tlc_fingerprint_batch(self._h, device, _p(words), _p(off), n, _p(fps)))
        return fps

    def tlc_min_permutation(self, record):
        """Number of the value permutation whose permuted state TLC fingerprints under SYMMETRY (host code)."""
        record = np.ascontiguousarray(record, dtype=np.uint64)
        perm = C.c_int32()
        check(capi.load().vsrmc_tlc_min_permutation(self._h, _p(record), C.byref(perm)))
        return perm.value

    def tlc_view_bytes(self, record, permutation=0):
        """The byte stream TLC's fingerprint of one wire record is taken over (host code, a diagnostic)."""
        record = np.ascontiguousarray(record, dtype=np.uint64)
        n = C.c_uint64()
        check(capi.load().vsrmc_tlc_view_bytes(self._h, _p(record), permutation, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        check(capi.load().vsrmc_tlc_view_bytes(self._h, _p(record), permutation, _p(out), len(out), C.byref(n)))
        return out.tobytes()

    def simulate(self, n_walkers=1 << 16, max_depth=100, seed=1, max_seconds=10.0, device=0):
        """≙ `tlc2.TLC -simulate -depth max_depth`: random walks on the GPU until an invariant fails or time runs out.
        -> dict(found, viol_mask, steps, walks, seconds, trace=[(action name, wire record)] or None)."""
        r = capi.SimResult()
        check(capi.load().vsrmc_simulate(self._h, device, n_walkers, max_depth, seed, max_seconds, C.byref(r)))
        out = dict(found=r.found, viol_mask=r.viol_mask, steps=r.steps, walks=r.walks, seconds=r.seconds, trace=None)
        if r.found == 1:
            ords = [int(r.ords[k]) for k in range(r.viol_steps)]
            out["ordinals"] = ords
            out["trace"] = self.replay(ords, device)
        return out

    def simulate_where(self, state=None, step=None, stop=True, n_walkers=1 << 16, max_depth=100, seed=1, max_seconds=10.0, max_rounds=0, device=0):
        """Random walks with the user's own predicates on every walk (k_simulate_where; the iteration contract: include/vsrmc.h).  `state`: a Where of
        compile_predicates, evaluated on every state a walker stands on; `step`: a Where of compile_step_predicates, on every pair it takes; one may be
        None.  stop=True ends the run at the first state / pair with any bit set (found 3 / 4) or violated built-in invariant (found 1); stop=False only
        counts.  max_rounds > 0: exactly that many launches of 64 iterations per walker, every count the same in every run with the same seed.
        -> dict(found, viol_mask, viol_steps, steps, walks, rounds, n_states, n_pairs, seconds, state_names, step_names, count_state={name: n},
        count_step={name: n}, hit=[names of the bits of viol_mask] for found 3 / 4, ordinals and trace=[(action name, wire record)] for found 1, 3, 4:
        for found 4 the last step of the trace is the pair that was hit)."""
        r = capi.SimWhereResult()
        check(capi.load().vsrmc_simulate_where(self._h, device, state._h if state is not None else None, step._h if step is not None else None,
                                               int(bool(stop)), n_walkers, max_depth, C.c_uint64(int(seed) & (2 ** 64 - 1)), max_seconds, max_rounds,
                                               C.byref(r)))
        sn = list(state.names) if state is not None else []
        pn = list(step.names) if step is not None else []
        out = dict(found=r.found, viol_mask=r.viol_mask, viol_steps=r.viol_steps, steps=r.steps, walks=r.walks, rounds=r.rounds, n_states=r.n_states,
                   n_pairs=r.n_pairs, seconds=r.seconds, state_names=sn, step_names=pn, count_state={nm: int(r.count_state[k]) for k, nm in enumerate(sn)},
                   count_step={nm: int(r.count_step[k]) for k, nm in enumerate(pn)}, hit=None, ordinals=None, trace=None)
        if r.found in (3, 4):
            out["hit"] = [nm for k, nm in enumerate(sn if r.found == 3 else pn) if (r.viol_mask >> k) & 1]
        if r.found in (1, 3, 4):
            out["ordinals"] = [int(r.ords[k]) for k in range(r.viol_steps)]
            out["trace"] = self.replay(out["ordinals"], device)
        return out

    def simulate_constrained(self, state=None, constraint=None, step=None, action_constraint=None, pruned_stop=(), stop=True, n_walkers=1 << 16,
                             max_depth=100, seed=1, max_seconds=10.0, max_rounds=0, device=0):
        """Random walks under a state constraint and / or an action constraint (k_simulate_constrained; the iteration contract: include/vsrmc.h): a walk
        moves only along permitted transitions into in-model states.  `state`: a Where of compile_predicates whose export `constraint` (a name or a
        number, as ModelChecker.constrain takes it; None: no state constraint) is the state constraint, every other export a query as in simulate_where;
        `step` / `action_constraint`: the same with a Where of compile_step_predicates.  At least one constraint.  `pruned_stop`: the exports of `state`
        (names or numbers, or a ready mask) that also end a stop=True run when they hold on a PRUNED successor (found 3; the walk includes the step
        into it).  -> the dict of simulate_where plus blocked, pruned, stuck, init_pruned (True: Init fails the constraint, nothing was walked)."""
        def index_of(where, name, what):
            if name is None:
                return -1
            if where is None:
                raise ValueError("%s=%r needs the program that exports it" % (what, name))
            return name if isinstance(name, int) else where.names.index(name)
        ks, kp = index_of(state, constraint, "constraint"), index_of(step, action_constraint, "action_constraint")
        mask = pruned_stop if isinstance(pruned_stop, int) else sum(1 << index_of(state, nm, "pruned_stop") for nm in pruned_stop)
        r = capi.SimConstrainedResult()
        check(capi.load().vsrmc_simulate_constrained(self._h, device, state._h if state is not None else None, ks, step._h if step is not None else None, kp,
                                                     mask, int(bool(stop)), n_walkers, max_depth, C.c_uint64(int(seed) & (2 ** 64 - 1)), max_seconds,
                                                     max_rounds, C.byref(r)))
        sn = list(state.names) if state is not None else []
        pn = list(step.names) if step is not None else []
        out = dict(found=r.found, viol_mask=r.viol_mask, viol_steps=r.viol_steps, steps=r.steps, walks=r.walks, rounds=r.rounds, n_states=r.n_states,
                   n_pairs=r.n_pairs, seconds=r.seconds, state_names=sn, step_names=pn, count_state={nm: int(r.count_state[k]) for k, nm in enumerate(sn)},
                   count_step={nm: int(r.count_step[k]) for k, nm in enumerate(pn)}, blocked=r.blocked, pruned=r.pruned, stuck=r.stuck,
                   init_pruned=bool(r.init_pruned), hit=None, ordinals=None, trace=None)
        if r.found in (3, 4):
            out["hit"] = [nm for k, nm in enumerate(sn if r.found == 3 else pn) if (r.viol_mask >> k) & 1]
        if r.found in (1, 3, 4):
            out["ordinals"] = [int(r.ords[k]) for k in range(r.viol_steps)]
            out["trace"] = self.replay(out["ordinals"], device)
        return out

    def replay(self, ords, device=0):
        """Re-execute a path of ordinals from Init on the GPU -> [(action name, wire record)]."""
        n = len(ords)
        cap_w = (n + 2) * int(self.layout.max_record_words)
        words = np.zeros(cap_w, dtype=np.uint64)
        off = np.zeros(n + 3, dtype=np.uint64)
        acts = np.zeros(n + 3, dtype=np.int32)
        o = np.array(list(ords) + [0], dtype=np.uint32)
        ns = C.c_uint64()
        check(capi.load().vsrmc_model_replay(self._h, device, _p(o), n, _p(words), cap_w, _p(off), _p(acts), len(off), C.byref(ns)))
        return [(ACTION_NAMES[acts[t]], words[int(off[t]): int(off[t + 1])].copy()) for t in range(ns.value)]

    def parse_states(self, text):
        """TLC's value syntax (trace expression, one state record, or console form) -> [(action name or None, wire record)];
        the inverse of format_state (≙ reading a TLC trace file)."""
        raw = text.encode() if isinstance(text, str) else text
        ns = C.c_uint64()
        check(capi.load().vsrmc_model_parse_states(self._h, raw, None, 0, None, None, 0, C.byref(ns)))
        n = ns.value
        cap_w = max(1, n) * int(self.layout.fixed_words + 255)
        words = np.zeros(cap_w, dtype=np.uint64)
        off = np.zeros(n + 1, dtype=np.uint64)
        acts = np.zeros(max(1, n), dtype=np.int32)
        check(capi.load().vsrmc_model_parse_states(self._h, raw, _p(words), cap_w, _p(off), _p(acts), n + 1, C.byref(ns)))
        return [(ACTION_NAMES[acts[t]] if acts[t] >= 0 else None, words[int(off[t]): int(off[t + 1])].copy()) for t in range(n)]

    def check_trace(self, records, device=0):
        """Is this list of wire records a behaviour of the model (Init, then successor after successor, as generated on the
        GPU)?  -> dict(ok, first_bad, ords, actions, inv_mask_last)."""
        n = len(records)
        off = np.zeros(n + 1, dtype=np.uint64)
        for t, r in enumerate(records):
            off[t + 1] = off[t] + np.uint64(len(r))
        words = np.concatenate([np.asarray(r, dtype=np.uint64) for r in records]) if n else np.zeros(1, dtype=np.uint64)
        ords = np.zeros(max(1, n), dtype=np.uint32)
        acts = np.full(max(1, n), -1, dtype=np.int32)
        bad, inv = C.c_int64(), C.c_int32()
        check(capi.load().vsrmc_model_check_trace(self._h, device, _p(words), _p(off), n, _p(ords), _p(acts), C.byref(bad), C.byref(inv)))
        good = n if bad.value < 0 else bad.value
        return dict(ok=bad.value < 0, first_bad=bad.value, ords=[int(x) for x in ords[: max(0, good - 1)]],
                    actions=[ACTION_NAMES[a] for a in acts[:good]], inv_mask_last=inv.value)

    def close(self):
        if self._h:
            capi.load().vsrmc_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FPSet:
    """≙ tlc2.tool.fp.FPSet: an open-addressing set of 64-bit fingerprints in HBM."""

    def __init__(self, log2_slots=20, device=0):
        self._h = C.c_void_p()
        check(capi.load().vsrmc_fpset_create(device, log2_slots, C.byref(self._h)))

    def put_block(self, fps):
        """-> uint8 array: 1 where the fingerprint was already present (FPSet.put's return value)."""
        fps = np.ascontiguousarray(fps, dtype=np.uint64)
        out = np.zeros(len(fps), dtype=np.uint8)
        check(capi.load().vsrmc_fpset_put_batch(self._h, _p(fps), len(fps), _p(out)))
        return out

    def contains_block(self, fps):
        fps = np.ascontiguousarray(fps, dtype=np.uint64)
        out = np.zeros(len(fps), dtype=np.uint8)
        check(capi.load().vsrmc_fpset_contains_batch(self._h, _p(fps), len(fps), _p(out)))
        return out

    def put(self, fp):
        return bool(self.put_block(np.array([fp], dtype=np.uint64))[0])

    def contains(self, fp):
        return bool(self.contains_block(np.array([fp], dtype=np.uint64))[0])

    def put_block_device(self, d_fps_ptr, n, d_out_ptr, stream=None):
        check(capi.load().vsrmc_fpset_put_batch_device(self._h, C.c_void_p(d_fps_ptr), n, C.c_void_p(d_out_ptr),
                                                       C.c_void_p(stream or 0)))

    def contains_block_device(self, d_fps_ptr, n, d_out_ptr, stream=None):
        check(capi.load().vsrmc_fpset_contains_batch_device(self._h, C.c_void_p(d_fps_ptr), n, C.c_void_p(d_out_ptr),
                                                            C.c_void_p(stream or 0)))

    def size(self):
        n = C.c_uint64()
        check(capi.load().vsrmc_fpset_size(self._h, C.byref(n)))
        return n.value

    def close(self):
        if self._h:
            capi.load().vsrmc_fpset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StateQueue:
    """≙ tlc2.tool.queue.StateQueue: a FIFO of state records in HBM (sEnqueue(TLCState[]) / sDequeue(int) / size)."""

    def __init__(self, capacity_words=1 << 24, capacity_states=1 << 20, device=0):
        self._h = C.c_void_p()
        check(capi.load().vsrmc_queue_create(device, capacity_words, capacity_states, C.byref(self._h)))

    def s_enqueue(self, words, off):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        check(capi.load().vsrmc_queue_enqueue_batch(self._h, _p(words), _p(off), len(off) - 1))

    def s_dequeue(self, max_states, cap_words=None):
        cap_words = cap_words or 256 * max_states
        words = np.zeros(cap_words, dtype=np.uint64)
        off = np.zeros(max_states + 1, dtype=np.uint64)
        n = C.c_uint64()
        check(capi.load().vsrmc_queue_dequeue_batch(self._h, max_states, _p(words), cap_words, _p(off), C.byref(n)))
        return words[: int(off[n.value])].copy(), off[: n.value + 1].copy()

    def size(self):
        n = C.c_uint64()
        check(capi.load().vsrmc_queue_size(self._h, C.byref(n)))
        return n.value

    def close(self):
        if self._h:
            capi.load().vsrmc_queue_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ModelChecker:
    """≙ tlc2.tool.ModelChecker: level-synchronous BFS; `step()` = every Worker draining one level of the StateQueue."""

    @classmethod
    def auto(cls, model, device=0, **kw):
        """every buffer sized from the free memory of the device (vsrmc_options with zeros): seen-set = the largest power of two of
        slots within 30 % of it, the rest in two equal record buffers; pass table_log2 / frontier_words / .. to pin one of them"""
        kw = dict(dict(table_log2=0, frontier_words=0, frontier_states=0, pending_entries=0), **kw)
        return cls(model, device=device, **kw)

    def __init__(self, model, device=0, table_log2=24, frontier_words=1 << 25, frontier_states=1 << 20,
                 pending_entries=1 << 21, keep_trace=True, trace_entries=0, exact_ties=False, recover=None, host_frontier=False, frontier_words_b=0):
        """recover: path of a checkpoint written by save() — continue that search (≙ `tlc2.TLC -recover`).
        table_log2 = 0 / frontier_words = 0 / frontier_states = 0 / pending_entries = 0: sized from the free device memory (auto())."""
        self.model = model
        self._deep = None                                            # (state Where, step Where) of deep_attach, or None
        self._deep_seen = set()                                      # (level, probed) pairs run(deep=True) has looked at
        self._constraint = None                                      # (Where, k) of constrain(), or None
        self._constraint_deep = False                                # constrain(.., deep=True): the constraint reaches the levels beyond the record buffers
        self._action_constraint = None                               # (step Where, k) of action_constrain(), or None
        self._action_constraint_deep = False                         # action_constrain(.., deep=True): the gate reaches the levels beyond the record buffers
        self.stopped = None                                          # the reason advance() gave for ("stopped", ..)
        self._pruned_checked = 0                                     # the newest filtered level run(never=..) has looked at
        o = capi.Options()
        capi.load().vsrmc_options_default(C.byref(o))
        o.device, o.table_log2 = device, table_log2
        o.frontier_words, o.frontier_states, o.pending_entries = frontier_words, frontier_states, pending_entries
        o.keep_trace = int(keep_trace)
        o.trace_entries = trace_entries
        o.exact_ties = int(exact_ties)
        o.frontier_words_b = frontier_words_b         # second record buffer (levels 2, 4, ...); 0 = frontier_words
        # bit mask: record buffer 0 (levels 1, 3, ...) / 1 (levels 2, 4, ...) in pinned host memory (≙ DiskStateQueue); True = both
        o.host_frontier = 3 if host_frontier is True else int(host_frontier)
        self.options = o
        self._h = C.c_void_p()
        if recover is None:
            check(capi.load().vsrmc_checker_create(model._h, C.byref(o), C.byref(self._h)))
            self._fresh()
        else:
            check(capi.load().vsrmc_checker_load(model._h, C.byref(o), os.fsencode(recover), C.byref(self._h)))
            info = capi.LevelInfo()
            check(capi.load().vsrmc_checker_status(self._h, C.byref(info)))
            self.level, self.n_frontier, self.distinct = info.level, info.n_new, info.distinct
            self.levels = [dict(level=info.level, n_new=info.n_new, generated=0, deadlocks=0, recovered=True)]
            self.violation = None
            self.rebased = []
            self.deadlock = None
            self.witness = None
            self.depth = self.level + info.reserved0               # a deep search: the levels beyond the stored one came along in the seen-set
        check(capi.load().vsrmc_checker_options(self._h, C.byref(o)))       # sizes left 0 were derived from the free device memory

    def save(self, path):
        """Checkpoint between two levels (≙ TLC's checkpoint of FPSet + StateQueue + TLCTrace): one file."""
        check(capi.load().vsrmc_checker_save(self._h, os.fsencode(path)))

    def _fresh(self):
        self.depth = 1
        self.level = 1
        self.n_frontier = 1
        self.distinct = 1
        self.levels = [dict(level=1, n_new=1, generated=0, deadlocks=0)]
        self.violation = None
        self.rebased = []
        self.deadlock = None
        self.witness = None
        self.stopped = None
        self._pruned_checked = 0

    def reset(self):
        """Back to Init with an empty seen-set; keeps the HBM allocations (a fresh TLC run on the same model).  A constraint stays attached: Init is
        evaluated again."""
        check(capi.load().vsrmc_checker_reset(self._h))
        self._fresh()
        self._after_init_filter()

    def _after_init_filter(self):
        if self._action_constraint is not None and self._action_constraint_deep:   # (a search that starts over keeps the attachment and the opt-in; asked for again: harmless)
            check(capi.load().vsrmc_checker_action_constrain_deep(self._h, 1))
        if self._constraint is not None:
            if self._constraint_deep:                                # (a search that starts over keeps the attachment; the opt-in is asked for again at level 1)
                check(capi.load().vsrmc_checker_constrain_deep(self._h, 1))
            st = capi.LevelInfo()
            check(capi.load().vsrmc_checker_status(self._h, C.byref(st)))
            self.n_frontier, self.distinct = st.n_new, st.distinct
            self.levels = [dict(level=1, n_new=st.n_new, generated=0, deadlocks=0)]

    def constrain(self, where, name=None, deep=False):
        """Attach a state constraint (TLC's CONSTRAINT; vsrmc_checker_constrain_attach): the exported predicate `name` (a name or a number; None: the
        program's only one) of the state program `where` (Model.compile_predicates).  A state that fails it is out of model: counted in `generated`,
        checked against the built-in invariants, but no distinct state, never expanded, never a parent in a trace.  At level 1 only (a fresh checker, or
        after reset()); Init is evaluated at once.  where=None detaches and starts over.  While attached, levels are stored only: advance() returns
        ("stopped", ..) and run() "constraint-out-of-room" when the next level does not fit the record buffers; deepen / probe / deep_attach / save
        are refused.
        deep=True (vsrmc_checker_constrain_deep): the constraint is applied on the levels beyond the record buffers as well — every scratch slice of a
        descent is filtered before anything reads it (k_constrain_slice) — so advance() / run() / check() / deepen() / probe() go on as on an unconstrained
        checker, filtered, and run() no longer ends "constraint-out-of-room".  constraint_results() gains rows for those levels, constraint_deep_results()
        says how each was filtered.  Not with an action constraint, exact_ties, deep_attach / deep_terminal_attach, save."""
        if where is None:
            check(capi.load().vsrmc_checker_constrain_attach(self._h, None, 0))
            self._constraint = None
            self._constraint_deep = False
            self._fresh()
            return
        if name is None:
            if len(where.names) != 1:
                raise ValueError("the program exports %d predicates: name the constraint" % len(where.names))
            name = 0
        k = name if isinstance(name, int) else where.names.index(name)
        check(capi.load().vsrmc_checker_constrain_attach(self._h, where._h, k))
        self._constraint = (where, k)
        self._constraint_deep = False
        if deep:
            try:
                check(capi.load().vsrmc_checker_constrain_deep(self._h, 1))
            except VsrmcError:
                capi.load().vsrmc_checker_constrain_attach(self._h, None, 0)     # nothing stays attached by a refused call
                self._constraint = None
                raise
            self._constraint_deep = True
        self._fresh()
        self._after_init_filter()

    def action_constrain(self, step_where, name=None, deep=False):
        """Attach an action constraint (TLC's ACTION_CONSTRAINT; vsrmc_checker_action_constrain_attach): the exported predicate `name` (a name or a number;
        None: the program's only one) of the STEP program `step_where` (Model.compile_step_predicates).  A transition that fails it is generated and
        counted but not taken: its successor is neither put into the seen-set nor stored, and may still be reached by a permitted transition.  Init is
        not subject to it.  At level 1 only (a fresh checker, or after reset()); step_where=None detaches, at any level, and starts over.  A state constraint
        (constrain) may be attached beside it.  While attached, levels are stored only (run(): "constraint-out-of-room" when the next one does not fit);
        deepen / probe / deep_attach / save are refused; every trace takes permitted steps only, and step_scan / step_never / step_reach judge the
        permitted transitions only (a blocked one is neither counted nor listed, and is never a witness).
        deep=True (vsrmc_checker_action_constrain_deep): the gate reaches the levels beyond the record buffers — the record-less first pass, the level a
        descent inserts and the probed level take permitted transitions only (k_step_expand's insert, stored and probe modes) — so advance() / run() /
        check() / deepen() / probe() go on as on an unconstrained checker and run() no longer ends "constraint-out-of-room".
        action_constraint_deep_results() has the figures of those levels.  Not beside a state constraint, and not with exact_ties, deep_attach /
        deep_terminal_attach, probe2 / probe3, save."""
        if step_where is None:
            check(capi.load().vsrmc_checker_action_constrain_attach(self._h, None, 0))
            self._action_constraint = None
            self._action_constraint_deep = False
            self._fresh()
            self._after_init_filter()
            return
        if name is None:
            if len(step_where.names) != 1:
                raise ValueError("the program exports %d predicates: name the action constraint" % len(step_where.names))
            name = 0
        k = name if isinstance(name, int) else step_where.names.index(name)
        check(capi.load().vsrmc_checker_action_constrain_attach(self._h, step_where._h, k))
        self._action_constraint = (step_where, k)
        self._action_constraint_deep = False
        if deep:
            try:
                check(capi.load().vsrmc_checker_action_constrain_deep(self._h, 1))
            except VsrmcError:
                self._action_constraint = None
                check(capi.load().vsrmc_checker_action_constrain_attach(self._h, None, 0))   # nothing stays attached by a refused call; the detaching call
                self._fresh()                                                                # starts the search over, and this object follows it
                self._after_init_filter()
                raise
            self._action_constraint_deep = True
        self._fresh()
        self._after_init_filter()

    def action_constraint_results(self, level=None):
        """The figures of the steps taken under the action constraint (vsrmc_checker_action_constraint_info) -> [dict(level, k, parents, pairs, permitted,
        blocked, blocked_act={action name: n}, blocked_violating, blocked_viol_mask, blocked_min_fp, blocked_viol_min_fp, n_new, slices, relisted,
        launches, list_ms, verdict_ms, expand_ms)], the step into level 2 first; level=L: the step into level L (0: the newest step, which may have
        found nothing).  Fingerprints are the PARENT's, None where there is no such pair."""
        if self._action_constraint is None:
            raise ValueError("no action constraint attached (action_constrain)")
        none = (1 << 64) - 1

        def one(lv):
            ai = capi.ActionConstraintInfo()
            check(capi.load().vsrmc_checker_action_constraint_info(self._h, lv, C.byref(ai)))
            d = {n: getattr(ai, n) for n, _ in ai._fields_ if n != "blocked_act"}
            d["blocked_act"] = {ACTION_NAMES[a]: int(ai.blocked_act[a]) for a in range(16) if ai.blocked_act[a]}
            for f in ("blocked_min_fp", "blocked_viol_min_fp"):
                d[f] = None if d[f] == none else int(d[f])
            return d
        if level is not None:
            return one(level)
        out, lv = [], 2
        while True:
            try:
                out.append(one(lv))
            except VsrmcError:
                # (with deep=True the levels beyond the buffers lie between stored ones — action_constraint_deep_results has those — up to the deepest level reached)
                if not self._action_constraint_deep or lv > max(self.level, self.depth) + 1:
                    return out
            lv += 1

    def action_constraint_deep_results(self, level=None):
        """The figures of the gated passes beyond the record buffers (vsrmc_checker_action_constraint_deep_info; action_constrain(.., deep=True)) ->
        [dict(level, kind in ("inserted-recordless", "inserted", "probed"), parents, pairs, permitted, blocked, blocked_act={action name: n},
        blocked_violating, blocked_viol_mask, blocked_min_fp, blocked_viol_min_fp, slices, relisted, launches, list_ms, verdict_ms, expand_ms)], ascending;
        level=L: the passes that led INTO level L.  A probed level is filed anew (kind "inserted") by the pass that inserts it, and its row goes when a stored
        step after a re-basing files the level in action_constraint_results() instead: the two lists never hold the same level."""
        if self._action_constraint is None:
            raise ValueError("no action constraint attached (action_constrain)")
        none = (1 << 64) - 1

        def one(lv):
            ai = capi.ActionConstraintDeepInfo()
            check(capi.load().vsrmc_checker_action_constraint_deep_info(self._h, lv, C.byref(ai)))
            d = {n: getattr(ai, n) for n, _ in ai._fields_ if n != "blocked_act"}
            d["kind"] = {1: "inserted-recordless", 2: "inserted", 3: "probed"}[d["kind"]]
            d["blocked_act"] = {ACTION_NAMES[a]: int(ai.blocked_act[a]) for a in range(16) if ai.blocked_act[a]}
            for f in ("blocked_min_fp", "blocked_viol_min_fp"):
                d[f] = None if d[f] == none else int(d[f])
            return d
        if level is not None:
            return one(level)
        out = []
        for lv in range(2, max(self.level, self.depth) + 3):
            try:
                out.append(one(lv))
            except VsrmcError as e:
                if e.code != -1:
                    raise
        return out

    def seen_set_load(self):
        """(occupied slots, slots) of the seen-set, counted from a copy of the table (vsrmc_checker_seen_set_load)."""
        occ, slots = C.c_uint64(), C.c_uint64()
        check(capi.load().vsrmc_checker_seen_set_load(self._h, C.byref(occ), C.byref(slots)))
        return occ.value, slots.value

    def constraint_results(self, level=None):
        """The figures of the filtered levels (vsrmc_checker_constraint_info) -> [dict(level, k, n_states, kept, pruned, kept_xor, kept_sum, kept_max_bag,
        kept_words, pruned_min_fp, pruned_count={name: n}, pruned_min_fp_k={name: fp or None}, kernel_ms)], level 1 (Init) first; level=L: that
        level's dict.  pruned_count / pruned_min_fp_k: the program's exported predicates over the PRUNED states of the level."""
        if self._constraint is None:
            raise ValueError("no constraint attached (constrain)")
        w = self._constraint[0]
        none = (1 << 64) - 1

        def one(lv):
            ci = capi.ConstraintInfo()
            check(capi.load().vsrmc_checker_constraint_info(self._h, lv, C.byref(ci)))
            d = {n: getattr(ci, n) for n, _ in ci._fields_ if n not in ("pruned_count", "pruned_min_fp_k")}
            d["pruned_min_fp"] = None if ci.pruned_min_fp == none else int(ci.pruned_min_fp)
            d["pruned_count"] = {nm: int(ci.pruned_count[p]) for p, nm in enumerate(w.names)}
            d["pruned_min_fp_k"] = {nm: (None if ci.pruned_min_fp_k[p] == none else int(ci.pruned_min_fp_k[p])) for p, nm in enumerate(w.names)}
            return d
        if level is not None:
            return one(level)
        out, lv = [], 1
        while True:
            try:
                out.append(one(lv))
            except VsrmcError:
                return out
            lv += 1

    def constraint_pruned(self, level=None):
        """The pruned states of the newest filtered level -> fingerprints ascending (vsrmc_checker_constraint_pruned).  More than the list holds:
        VsrmcError (-5) that names the true number; the counts and minima of constraint_results() are exact regardless.
        level=L (constrain(.., deep=True)): the list of level L, kept for the levels the last filtering descent recorded — the newest one and, when that
        descent met a level not judged yet, that level (vsrmc_checker_constraint_pruned_level)."""
        n = C.c_uint64()
        lib = capi.load()
        lv = 0 if level is None else int(level)
        rc = lib.vsrmc_checker_constraint_pruned_level(self._h, lv, None, 0, C.byref(n))
        if rc not in (0, -5):
            check(rc)
        fps = np.zeros(max(1, n.value), dtype=np.uint64)
        check(lib.vsrmc_checker_constraint_pruned_level(self._h, lv, _p(fps), len(fps), C.byref(n)))
        return fps[: n.value].copy()

    def constraint_deep_results(self, level=None):
        """How the levels beyond the record buffers were filtered (vsrmc_checker_constraint_deep_info; constrain(.., deep=True)) -> [dict(level, kind in
        ("regenerated", "inserted"), filtered, list_overflowed, slices, launches, regen_records, regen_pruned)], ascending; level=L: that level's dict.
        filtered False: the level is complete in the seen-set and not judged yet — the next descent regenerates and filters it, and constraint_results()
        has no row for it until then."""
        def one(lv):
            di = capi.ConstraintDeepInfo()
            check(capi.load().vsrmc_checker_constraint_deep_info(self._h, lv, C.byref(di)))
            d = {n: int(getattr(di, n)) for n, _ in di._fields_}
            d["kind"] = {1: "regenerated", 2: "inserted"}[d["kind"]]
            d["filtered"], d["list_overflowed"] = bool(d["filtered"]), bool(d["list_overflowed"])
            return d
        if level is not None:
            return one(level)
        out = []
        for lv in range(2, 512):
            try:
                out.append(one(lv))
            except VsrmcError as e:
                if e.code != -1:
                    raise
        return out

    def seed_records(self, words, off):
        """TEST HOOK (the hooks library only: csrc/host_test_seed.hpp): start the search from the wire records words[off[i] : off[i + 1]] instead of
        Init — they become level 1, the seen-set holds exactly them; step() / probe() / deepen() / terminal_scan() / select() then run as on any level.
        reset() goes back to Init."""
        fn = getattr(capi.load(), "vsrmc_test_checker_seed_records", None)
        if fn is None:
            raise RuntimeError("vsrmc_test_checker_seed_records is a test hook: load libvsrmc_hooks.so (VSRMC_LIB)")
        words = np.ascontiguousarray(words, dtype=np.uint64)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        check(fn(self._h, _p(words), _p(off), len(off) - 1))
        self._fresh()
        self.n_frontier = self.distinct = len(off) - 1
        self.levels = [dict(level=1, n_new=len(off) - 1, generated=0, deadlocks=0, seeded=True)]

    def extra_launches(self):
        """TEST HOOK (the hooks library only): the checker's running count of k_expand launches beyond a pass's first one — a stored step adds one per
        list of overflowed tiles it launches again."""
        fn = getattr(capi.load(), "vsrmc_test_checker_extra_launches", None)
        if fn is None:
            raise RuntimeError("vsrmc_test_checker_extra_launches is a test hook: load libvsrmc_hooks.so (VSRMC_LIB)")
        n = C.c_uint64()
        check(fn(self._h, C.byref(n)))
        return n.value

    def step(self):
        info = capi.LevelInfo()
        check(capi.load().vsrmc_checker_step(self._h, C.byref(info)))
        d = info.as_dict()
        self.level, self.n_frontier, self.distinct = d["level"], d["n_new"], d["distinct"]
        self.depth = self.level
        if d["n_new"]:
            self.levels.append(d)
        if d["viol_mask"] and self.violation is None:
            self.violation = dict(level=self._viol_level(d), index=d["viol_index"], fp=d["viol_fp"], mask=d["viol_mask"])
        return d

    def _viol_level(self, d):
        """the level of the violator a step reported.  With a constraint attached it is the newest FILTERED level: when every state of that level is out of
        model the checker steps back to the level before (d["level"]), the violator is a state of the level after it"""
        if self._constraint is None:
            return d["level"]
        return self.constraint_results(0)["level"]

    def check(self, max_depth=0, max_seconds=0.0):
        """≙ ModelChecker.runTLC in one native call (vsrmc_check: the automatic level scheme)
        -> "exhausted" | "violation" | "max-depth" | "max-seconds" | "seen-set-full" | "constraint-out-of-room" (a constraint is attached and the
        next level does not fit the record buffers: self.stopped = the reason)."""
        reason = C.c_int32()
        info = capi.LevelInfo()
        check(capi.load().vsrmc_check(self._h, max_depth, max_seconds, C.byref(reason), C.byref(info)))
        d = info.as_dict()
        self.depth = d["level"]                                           # the deepest level that is complete (stored or in the seen-set only)
        self.distinct = d["distinct"]
        st = capi.LevelInfo()
        check(capi.load().vsrmc_checker_status(self._h, C.byref(st)))     # the newest STORED level: what level_fps / frontier / trace(index) address
        self.level, self.n_frontier = st.level, st.n_new
        check(capi.load().vsrmc_checker_options(self._h, C.byref(self.options)))   # (the seen-set may have grown)
        if reason.value == 1:
            beyond = self._constraint_deep and d["level"] > st.level      # found in an inserted or a probed level: that info names its own level
            self.violation = dict(level=d["level"] if beyond else self._viol_level(d), index=d["viol_index"], fp=d["viol_fp"], mask=d["viol_mask"],
                                  probed=d["viol_index"] == (1 << 64) - 1)
        if reason.value == 5:
            self.stopped = capi.load().vsrmc_last_error().decode()
        return ["exhausted", "violation", "max-depth", "max-seconds", "seen-set-full", "constraint-out-of-room"][reason.value]

    def _deep_dict(self, info):
        d = info.as_dict()
        d["ancestor_index"] = d.pop("viol_index")
        if d["level"] and d["viol_mask"] and self.violation is None:
            self.violation = dict(level=d["level"], index=None, fp=d["viol_fp"], mask=d["viol_mask"], probed=True)
        return d

    def deepen(self):
        """One more level beyond the record buffers (vsrmc_checker_deepen): the next level is inserted into the seen-set only — counted,
        checked, checksummed, its records regenerated from the newest stored level whenever they are needed — and the level after it is
        probed.  -> (inserted dict, probed dict or None).  `self.depth` = the deepest level that is complete in the seen-set."""
        a, b = capi.LevelInfo(), capi.LevelInfo()
        check(capi.load().vsrmc_checker_deepen(self._h, C.byref(a), C.byref(b)))
        da, db = self._deep_dict(a), self._deep_dict(b)
        self.depth, self.distinct = da["level"], da["distinct"]
        return da, (db if db["level"] else None)

    def advance(self):
        """One unit of progress of the automatic level scheme (vsrmc_checker_advance): an ordinary level while the next one is
        predicted to fit the record buffers, else a deepen() pass.  -> ("level", dict, None) | ("deep", inserted dict, probed dict or None)."""
        a, b = capi.LevelInfo(), capi.LevelInfo()
        what = C.c_int32()
        check(capi.load().vsrmc_checker_advance(self._h, C.byref(a), C.byref(b), C.byref(what)))
        while what.value == 3:                       # re-based: the newest seen-set-only level became the stored base (no new level): go on
            self.level, self.n_frontier = a.level, a.n_new
            self.rebased.append(dict(level=a.level, n=a.n_new, seconds=a.seconds, launches=a.pending))
            check(capi.load().vsrmc_checker_advance(self._h, C.byref(a), C.byref(b), C.byref(what)))
        if what.value == 4:                          # a constraint is attached and the next level does not fit: nothing was done
            self.stopped = capi.load().vsrmc_last_error().decode()
            return "stopped", a.as_dict(), None
        if what.value == 1:
            d = a.as_dict()
            self.level, self.n_frontier, self.distinct = d["level"], d["n_new"], d["distinct"]
            self.depth = self.level
            if d["n_new"]:
                self.levels.append(d)
            if d["viol_mask"] and self.violation is None:
                self.violation = dict(level=self._viol_level(d), index=d["viol_index"], fp=d["viol_fp"], mask=d["viol_mask"])
            return "level", d, None
        da, db = self._deep_dict(a), self._deep_dict(b)
        self.depth, self.distinct = da["level"], da["distinct"]
        return "deep", da, (db if db["level"] else None)

    def room(self):
        """The seen-set before the next advance(): 0 = room enough, 1 = just re-hashed into a table of twice the slots (self.options.table_log2 is
        refreshed), 2 = more than 85 % full and no device memory to grow into: the search is incomplete at the depth reached."""
        st = C.c_int32()
        check(capi.load().vsrmc_checker_room(self._h, C.byref(st)))
        if st.value == 1:
            check(capi.load().vsrmc_checker_options(self._h, C.byref(self.options)))
        return st.value

    def run(self, max_depth=None, max_seconds=None, stop_on_violation=True, check_deadlock=False, reach=None, never=None, step_never=None, step_reach=None,
            deep=False):
        """Worker.run until the queue is empty, an invariant is violated, or a bound is hit — the automatic level scheme: levels are
        stored while they fit the record buffers, the search goes on beyond them through the seen-set alone (deepen).
        check_deadlock (TLC's default, off here): every stored level is scanned for terminal states before it is expanded; the first level
        that has one ends the run with "deadlock" — self.deadlock = the scan's result, deadlock_trace() the behaviour.
        With a constraint attached (constrain) the scans see the in-model states, and `never` is checked on the states each level prunes as well (Init
        included) — through the figures k_constrain keeps for every predicate its own program exports: that program must export every name of `never`
        (ValueError otherwise; that the two definitions of a name agree is the caller's business: compile both from one text).  self.witness then has
        pruned=True and index None.
        reach / never (a Where each, off by default): every stored level is scanned (k_where) before it is expanded, where check_deadlock scans.  The
        first level with a state that satisfies a predicate of `reach` ends the run with "reached"; one that satisfies a predicate of `never` (the
        negation of a user's invariant) ends it with "violation".  self.witness = dict(level, k, name, fp, index, kind); witness_trace() the behaviour.
        step_never / step_reach (a step Where each — Model.compile_step / compile_step_predicates — off by default): every stored level is step-scanned (step_scan: every
        transition out of it) before it is expanded, after the scans above.  A pair that satisfies a predicate of step_never ends the run with
        "violation", one that satisfies step_reach with "reached"; self.witness then names the PARENT (level, fp, index) and has `ordinal` and
        `action` besides; step_witness_trace() is the behaviour with the step at its end.
        deep=True: the predicates are also ATTACHED (deep_attach) — one state program (`never` or `reach`, not both) and one step program (`step_never` or
        `step_reach`) — so that the levels beyond the record buffers are examined as well; the run ends at the advance() that finds a hit.  The shallowest
        level wins; within a level a built-in violation, then never, reach, step_never, step_reach.  self.witness then has `kind_of_level` in
        ("regenerated", "inserted", "probed") and index None (a step hit: no ordinal either); deep_witness_trace() is the behaviour.
        check_deadlock=True with deep=True (valid without a predicate): the terminal attachment (deep_terminal_attach) looks for terminal states on the
        levels beyond the record buffers too, the probed level included; the run ends with "deadlock" at the advance() whose results hold one.
        self.deadlock then has `kind_of_level` and `exact` besides (min_index None); deadlock_trace() is the behaviour.  Within a level a deadlock comes
        after a built-in violation and before the predicates; the shallowest level wins, also against a built-in violation found deeper by the same pass."""
        import time
        t0 = time.time()
        if never is not None and self._constraint is not None:
            missing = [nm for nm in never.names if nm not in self._constraint[0].names]
            if missing:
                raise ValueError("run(never=..) with a constraint attached: the constraint's program does not export %s, so the states it prunes would not be "
                                 "checked against them — define the predicates of `never` in the text the constraint was compiled from as well" % ", ".join(missing))
        deep_state = deep_step = None
        if deep:
            if never is not None and reach is not None:
                raise ValueError("run(deep=True) attaches one state program: never or reach")
            if step_never is not None and step_reach is not None:
                raise ValueError("run(deep=True) attaches one step program: step_never or step_reach")
            deep_state = (never, "violation", 1) if never is not None else (reach, "reached", 2) if reach is not None else None
            deep_step = (step_never, "violation", 3) if step_never is not None else (step_reach, "reached", 4) if step_reach is not None else None
            if deep_state is None and deep_step is None and not check_deadlock:
                raise ValueError("run(deep=True) needs a predicate or check_deadlock=True")
            if deep_state is not None or deep_step is not None:
                self.deep_attach(deep_state[0] if deep_state else None, deep_step[0] if deep_step else None)
            if check_deadlock:
                self.deep_terminal_attach()
            self._deep_seen = set()
            self._deep_term_seen = set()
        while True:
            if max_depth is not None and self.depth >= max_depth:
                return "max-depth"
            if max_seconds is not None and time.time() - t0 > max_seconds:
                return "max-seconds"
            if self.room() == 2:
                return "seen-set-full"
            if check_deadlock and self.depth == self.level and self.n_frontier:
                t = self.terminal_scan()
                if t["n_terminal"]:
                    return "deadlock"
            if self.depth == self.level and self.n_frontier:
                for w, kind in ((never, "violation"), (reach, "reached")):
                    if w is None:
                        continue
                    t = self.where_scan(w)
                    hits = [k for k in range(len(w.names)) if t["count"][k]]
                    if hits:
                        k = hits[0]
                        self.witness = dict(level=t["level"], k=k, name=w.names[k], fp=t["min_fp"][k], index=t["min_index"][k], kind=kind)
                        return kind
                for w, kind in ((step_never, "violation"), (step_reach, "reached")):
                    if w is None:
                        continue
                    t = self.step_scan(w)
                    hits = [k for k in range(len(w.names)) if t["count"][k]]
                    if hits:
                        k = hits[0]
                        self.witness = dict(level=t["level"], k=k, name=w.names[k], fp=t["min_fp"][k], index=t["min_index"][k], kind=kind,
                                            ordinal=t["min_ordinal"][k], action=ACTION_NAMES[t["min_action"][k]])
                        return kind
            if never is not None and self._never_on_pruned(never):          # (Init, when it is out of model)
                return "violation"
            kind, d, p = self.advance()
            if kind == "stopped":
                return "constraint-out-of-room"
            if never is not None and self._never_on_pruned(never):
                return "violation"
            if deep and kind == "deep":
                hit = self._deep_first_hit(deep_state, deep_step, stop_on_violation, check_deadlock)
                if hit is not None:
                    return hit
            if d["n_new"] == 0:
                return "exhausted"
            if self.violation is not None and stop_on_violation:
                return "violation"

    def _never_on_pruned(self, never):
        """run(never=..) with a constraint attached: the user's invariant on the states the newest filtered level pruned, if that level has not been looked at
        yet (TLC checks an invariant before the constraint).  k_constrain evaluates its WHOLE program on every pruned state, so the figures exist for the
        predicates the constraint's program exports: run() has checked that it exports every name of `never`.  -> True: self.witness is set"""
        if self._constraint is None:
            return False
        r = self.constraint_results(0)
        if r["level"] <= self._pruned_checked:
            return False
        if self._constraint_deep and self._pruned_checked and r["level"] > self._pruned_checked + 1:
            # a descent recorded two levels (one that was inserted unfiltered, and the one it inserted): the shallower one first
            try:
                below = self.constraint_results(r["level"] - 1)
                if any(below["pruned_count"][nm] for nm in never.names):
                    r = below
            except VsrmcError:
                pass
        self._pruned_checked = max(self._pruned_checked, r["level"])
        hits = [nm for nm in never.names if r["pruned_count"][nm]]
        if not hits:
            return False
        self.witness = dict(level=r["level"], k=never.names.index(hits[0]), name=hits[0], fp=r["pruned_min_fp_k"][hits[0]], index=None, kind="violation", pruned=True)
        return True

    def _deep_first_hit(self, deep_state, deep_step, stop_on_violation, check_deadlock=False):
        """the results of the levels the last advance() examined for the first time -> the run's verdict, or None.  The shallowest level wins; within a
        level a built-in violation (0), a deadlock (0.5), then the predicates in their order (1 .. 4)."""
        best = None
        if self.violation is not None and stop_on_violation:
            best = (self.violation["level"], 0, None, "violation")
        deadlock = None
        for r in (self.deep_terminal_results() if check_deadlock else ()):
            key = (r["level"], r["kind"] == "probed")
            if key in self._deep_term_seen:
                continue
            self._deep_term_seen.add(key)
            if r["n_terminal"] and (best is None or (r["level"], 0.5) < best[:2]):
                deadlock = dict(level=r["level"], n_states=r["n_states"], n_terminal=r["n_terminal"], n_unsettled=r["n_unsettled"], min_fp=r["min_fp"],
                                min_index=None, min_fp_unsettled=r["min_fp_unsettled"], min_index_unsettled=None, kernel_ms=r["ms"],
                                kind_of_level=r["kind"], exact=r["exact"])
                best = (r["level"], 0.5, None, "deadlock")
        for r in (self.deep_results() if (deep_state is not None or deep_step is not None) else ()):
            key = (r["level"], r["kind"] == "probed")
            if key in self._deep_seen:
                continue
            self._deep_seen.add(key)
            for prog, part in ((deep_state, r["state"]), (deep_step, r["step"])):
                if prog is None or part is None:
                    continue
                w, verdict, order = prog
                hits = [k for k in range(len(w.names)) if part["count"][k]]
                if hits and (best is None or (r["level"], order) < best[:2]):
                    k = hits[0]
                    best = (r["level"], order, dict(level=r["level"], k=k, name=w.names[k], fp=part["min_fp"][k], index=None, kind=verdict,
                                                    kind_of_level=r["kind"], program="step" if w.step else "state", exact=r["exact"]), verdict)
        if best is None:
            return None
        if best[2] is not None:
            self.witness = best[2]
        if best[3] == "deadlock":
            self.deadlock = deadlock
        return best[3]

    def violation_trace(self):
        """the counter-example of the violation run() / advance() reported, wherever it was found"""
        v = self.violation
        if self._constraint_deep and v.get("probed"):    # found beyond the record buffers (an inserted or a probed level): walked from what the pass recorded
            try:
                return self.probe_trace()
            except VsrmcError:                       # (no pass beyond the buffers reported it: an out-of-model violator of a stored level, below)
                pass
        if self._constraint is not None:            # (the violator may be out of model: its index slot is withdrawn, its seen-set slot is not)
            return self.trace_fp(v["level"], v["fp"])
        return self.probe_trace() if v.get("probed") else self.trace(v["level"], v["index"])

    def terminal_scan(self):
        """Scan the newest stored level for terminal states (k_terminal: guards only, nothing applied, the seen-set untouched) -> dict(level,
        n_states, n_terminal, n_unsettled, min_fp, min_index, min_fp_unsettled, min_index_unsettled, kernel_ms); fingerprints / indices are
        None where there is no such state.  n_terminal == `deadlocks` of the step that expands this level.  Remembers the first level that
        has a terminal state as self.deadlock (the shallowest level, there the smallest fingerprint: the same state in every run)."""
        info = capi.TerminalInfo()
        check(capi.load().vsrmc_checker_terminal_scan(self._h, C.byref(info)))
        d = info.as_dict()
        for k in ("min_fp", "min_index", "min_fp_unsettled", "min_index_unsettled"):
            if d[k] == (1 << 64) - 1:
                d[k] = None
        if d["n_terminal"] and (self.deadlock is None or d["level"] < self.deadlock["level"]):
            self.deadlock = d
        return d

    def terminal_states(self):
        """The terminal states the last terminal_scan() found -> (fingerprints ascending, flag bytes: bit 0 set, bit 1 = unsettled)."""
        n = C.c_uint64()
        lib = capi.load()
        rc = lib.vsrmc_checker_terminal_states(self._h, None, None, 0, C.byref(n))
        if rc not in (0, -5):                                             # -5 (VSRMC_E_REP): more than the list holds — raised below, by the call that copies
            check(rc)
        fps = np.zeros(max(1, n.value), dtype=np.uint64)
        flags = np.zeros(max(1, n.value), dtype=np.uint8)
        check(lib.vsrmc_checker_terminal_states(self._h, _p(fps), _p(flags), len(fps), C.byref(n)))
        return fps[: n.value].copy(), flags[: n.value].copy()

    def where_scan(self, w):
        """Evaluate the predicates of `w` on the newest stored level (k_where; nothing applied, the seen-set untouched) -> dict(level, n_states,
        count[k], min_fp[k], min_index[k], kernel_ms), one entry per exported predicate; fingerprint / index None where no state satisfies it."""
        info = capi.WhereInfo()
        check(capi.load().vsrmc_checker_where_scan(self._h, w._h, C.byref(info)))
        none = (1 << 64) - 1
        n = len(w.names)
        self._where = (w, info.level, [None if info.min_fp[k] == none else int(info.min_fp[k]) for k in range(n)])
        return dict(level=info.level, n_states=info.n_states, count=[int(info.count[k]) for k in range(n)], min_fp=list(self._where[2]),
                    min_index=[None if info.min_index[k] == none else int(info.min_index[k]) for k in range(n)], kernel_ms=info.kernel_ms)

    def where_states(self):
        """The states of the last where_scan() that satisfy any predicate -> (fingerprints ascending, their bits)."""
        n = C.c_uint64()
        lib = capi.load()
        rc = lib.vsrmc_checker_where_states(self._h, None, None, 0, C.byref(n))
        if rc not in (0, -5):                                             # -5 (VSRMC_E_REP): more than the list holds — raised below, by the call that copies
            check(rc)
        fps = np.zeros(max(1, n.value), dtype=np.uint64)
        bits = np.zeros(max(1, n.value), dtype=np.uint8)
        check(lib.vsrmc_checker_where_states(self._h, _p(fps), _p(bits), len(fps), C.byref(n)))
        return fps[: n.value].copy(), bits[: n.value].copy()

    def witness_trace(self, k=None):
        """The behaviour from Init into the state with the smallest fingerprint that satisfies predicate k (a number or a name) in the level of the
        last where_scan(); k=None: the witness run(reach= / never=) stopped at.  [(action name, record)], the shape of violation_trace()."""
        if k is None:
            if self.witness is None:
                raise ValueError("run(reach=..) / run(never=..) has not stopped at a state")
            return self.trace_fp(self.witness["level"], self.witness["fp"])
        w, level, fps = getattr(self, "_where", (None, None, None))
        if w is None:
            raise ValueError("no where_scan() yet")
        if not isinstance(k, int):
            k = w.names.index(k)
        if fps[k] is None:
            raise ValueError("no state of level %d satisfies %s" % (level, w.names[k]))
        return self.trace_fp(level, fps[k])

    def step_scan(self, w):
        """Evaluate the step predicates of `w` on every transition out of the newest stored level (k_step_list / k_step_apply; no successor is
        written, the seen-set untouched) -> dict(level, n_states, n_pairs, n_err, count[k], min_fp[k], min_index[k], min_ordinal[k], min_action[k],
        kernel_ms, list_ms, apply_ms, slices).  min_fp[k] is the smallest PARENT fingerprint with a pair that satisfies predicate k, min_ordinal[k]
        that parent's smallest such ordinal; None where no pair satisfies it.  n_pairs + n_err == `generated` of the step that expands the level."""
        info = capi.StepInfo()
        check(capi.load().vsrmc_checker_step_scan(self._h, w._h, C.byref(info)))
        none = (1 << 64) - 1
        n = len(w.names)
        has = [info.count[k] != 0 for k in range(n)]
        return dict(level=info.level, n_states=info.n_states, n_pairs=info.n_pairs, n_err=info.n_err, count=[int(info.count[k]) for k in range(n)],
                    min_fp=[None if info.min_fp[k] == none else int(info.min_fp[k]) for k in range(n)],
                    min_index=[None if info.min_index[k] == none else int(info.min_index[k]) for k in range(n)],
                    min_ordinal=[int(info.min_ordinal[k]) if has[k] else None for k in range(n)],
                    min_action=[int(info.min_action[k]) if has[k] else None for k in range(n)],
                    kernel_ms=info.kernel_ms, list_ms=info.list_ms, apply_ms=info.apply_ms, slices=int(info.slices))

    def step_pairs(self):
        """The pairs of the last step_scan() that satisfy any predicate -> (parent fingerprints, ordinals, bits), by (fingerprint, ordinal)."""
        n = C.c_uint64()
        lib = capi.load()
        rc = lib.vsrmc_checker_step_pairs(self._h, None, None, None, 0, C.byref(n))
        if rc not in (0, -5):                                             # -5 (VSRMC_E_REP): more than the list holds — raised below, by the call that copies
            check(rc)
        fps = np.zeros(max(1, n.value), dtype=np.uint64)
        ords = np.zeros(max(1, n.value), dtype=np.uint32)
        bits = np.zeros(max(1, n.value), dtype=np.uint8)
        check(lib.vsrmc_checker_step_pairs(self._h, _p(fps), _p(ords), _p(bits), len(fps), C.byref(n)))
        return fps[: n.value].copy(), ords[: n.value].copy(), bits[: n.value].copy()

    def step_witness_trace(self):
        """The behaviour into the pair run(step_never= / step_reach=) stopped at: trace_fp(level, parent fingerprint) plus one entry (action name,
        successor record) — the successor as the action generated it."""
        wit = self.witness
        if wit is None or "ordinal" not in wit:
            raise ValueError("run(step_never=..) / run(step_reach=..) has not stopped at a pair")
        tr = self.trace_fp(wit["level"], wit["fp"])
        # (the ordinal names a position in the bag of the record as the level stores it; the traced record of that state may be another member of its
        # orbit: the library finds the same step — action and successor fingerprint — out of the traced record)
        words = np.zeros(int(self.model.layout.max_record_words), dtype=np.uint64)
        parent = np.ascontiguousarray(tr[-1][1], dtype=np.uint64)
        n, act = C.c_uint64(), C.c_int32()
        check(capi.load().vsrmc_checker_step_successor(self._h, wit["index"], wit["ordinal"], _p(parent), len(parent), _p(words), len(words), C.byref(n),
                                                       C.byref(act)))
        return tr + [(ACTION_NAMES[act.value], words[: n.value].copy())]

    def deadlock_trace(self):
        """The behaviour into the terminal state terminal_scan() / run(check_deadlock=True) reported (self.deadlock): [(action name, record)]
        from Init, the shape of violation_trace()."""
        d = self.deadlock
        if d is None:
            raise ValueError("no terminal state has been found (terminal_scan)")
        if "kind_of_level" in d:                     # found beyond the record buffers (run(check_deadlock=True, deep=True))
            return self.deep_terminal_trace(d["level"], probed=d["kind_of_level"] == "probed")
        return self.trace_fp(d["level"], d["min_fp"])

    def level_fps(self):
        out = np.zeros(max(1, self.n_frontier), dtype=np.uint64)
        n = C.c_uint64()
        check(capi.load().vsrmc_checker_level_fps(self._h, _p(out), len(out), C.byref(n)))
        return out[: n.value].copy()

    def tlc_level_fps(self, fetch=True):
        """FP64 (TLC's fingerprint, [TLC-RECALLED]) of every state of the newest level, from the frontier in HBM -> (sorted fps or None, kernel ms)."""
        out = np.zeros(max(1, self.n_frontier), dtype=np.uint64) if fetch else None
        n = C.c_uint64()
        ms = C.c_double()
        check(capi.load().vsrmc_checker_tlc_level_fps(self._h, _p(out) if fetch else None, len(out) if fetch else 0, C.byref(n), C.byref(ms)))
        return (out[: n.value].copy() if fetch else None), ms.value

    def frontier(self):
        """The newest level in wire layout -> (words, offsets)."""
        lay = self.model.layout
        cap_w = max(1, self.n_frontier) * int(lay.max_record_words)
        words = np.zeros(cap_w, dtype=np.uint64)
        off = np.zeros(self.n_frontier + 1, dtype=np.uint64)
        n = C.c_uint64()
        check(capi.load().vsrmc_checker_frontier(self._h, _p(words), cap_w, _p(off), len(off), C.byref(n)))
        return words[: int(off[n.value])].copy(), off[: n.value + 1].copy()

    def level_checksum(self):
        """(xor, sum mod 2^64, count) of the newest level's fingerprints, computed on the device."""
        x, s_, n = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(capi.load().vsrmc_checker_level_checksum(self._h, C.byref(x), C.byref(s_), C.byref(n)))
        return x.value, s_.value, n.value

    def select(self, action_mask, max_states=4096):
        """States of the newest level in which an action of `action_mask` (bit a = action id a) is enabled
        -> (words, off, n_matching): at most max_states wire records, and how many such states the level has."""
        cap_w = int(max_states) * int(self.model.layout.max_record_words) + 16
        words = np.zeros(cap_w, dtype=np.uint64)
        off = np.zeros(int(max_states) + 1, dtype=np.uint64)
        n, total = C.c_uint64(), C.c_uint64()
        check(capi.load().vsrmc_checker_select(self._h, int(action_mask), int(max_states), _p(words), cap_w, _p(off), C.byref(n),
                                               C.byref(total)))
        return words[: int(off[n.value])], off[: n.value + 1], total.value

    def find_fp(self, fp):
        """Index (in the newest level's index range) of the state with fingerprint `fp`, or None."""
        idx = C.c_uint64()
        check(capi.load().vsrmc_checker_find_fp(self._h, int(fp), C.byref(idx)))
        return None if idx.value == (1 << 64) - 1 else idx.value

    def trace_fp(self, level, fp):
        """TLCTrace.getTrace for the level-`level` state with fingerprint `fp` (any completed level)."""
        lay = self.model.layout
        cap_w = (level + 1) * int(lay.max_record_words)
        words = np.zeros(cap_w, dtype=np.uint64)
        off = np.zeros(level + 2, dtype=np.uint64)
        acts = np.zeros(level + 2, dtype=np.int32)
        n = C.c_uint64()
        check(capi.load().vsrmc_checker_trace_fp(self._h, level, int(fp), _p(words), cap_w, _p(off), _p(acts), len(off), C.byref(n)))
        return [(ACTION_NAMES[acts[t]], words[int(off[t]): int(off[t + 1])].copy()) for t in range(n.value)]

    def lookup(self, key, level=0, by_low_bits=False):
        """one step of a trace walk through the seen-set -> (fingerprint, meta) or None; by_low_bits: a third element = the number
        of states of that level whose fingerprint ends in those 45 bits (> 1: the predecessor pointer is ambiguous)"""
        found, fp, meta = C.c_int32(), C.c_uint64(), C.c_uint64()
        check(capi.load().vsrmc_checker_lookup(self._h, int(key), int(level), int(by_low_bits), C.byref(found), C.byref(fp), C.byref(meta)))
        if not found.value:
            return None
        return (fp.value, meta.value, found.value) if by_low_bits else (fp.value, meta.value)

    def trace(self, level, index):
        """TLCTrace.getTrace -> list of (action name, record words) from Init to state `index` of the newest level."""
        lay = self.model.layout
        cap_w = (level + 1) * int(lay.max_record_words)
        words = np.zeros(cap_w, dtype=np.uint64)
        off = np.zeros(level + 2, dtype=np.uint64)
        acts = np.zeros(level + 2, dtype=np.int32)
        n = C.c_uint64()
        check(capi.load().vsrmc_checker_trace(self._h, level, index, _p(words), cap_w, _p(off), _p(acts), len(off),
                                              C.byref(n)))
        return [(ACTION_NAMES[acts[t]], words[int(off[t]): int(off[t + 1])].copy()) for t in range(n.value)]

    DEEP_KINDS = ("regenerated", "inserted", "probed")

    def deep_attach(self, state=None, step=None):
        """Attach a state Where and / or a step Where to the search beyond the record buffers (vsrmc_checker_deep_attach): every deepen() — and every
        deepen inside advance() / run() / check() — then evaluates them on the levels that exist in the seen-set only, each level once, and the state
        program on the probed level as well (k_probe_where).  Both None detaches.  Results: deep_results()."""
        check(capi.load().vsrmc_checker_deep_attach(self._h, state._h if state is not None else None, step._h if step is not None else None))
        self._deep = (state, step) if (state is not None or step is not None) else None

    def deep_results(self):
        """The per-level results of the attached programs, ascending by (level, probed) -> [dict(level, kind in DEEP_KINDS, exact, slices, n_hit_states,
        n_hit_pairs, where_ms, step_ms, state=dict(n_states, count[k], min_fp[k]) or None, step=dict(n_states, n_pairs, n_err, count[k], min_fp[k], slices)
        or None)].  kind "probed": count[k] = distinct states, lower bounds when exact is False."""
        lib = capi.load()
        n = C.c_uint64()
        check(lib.vsrmc_checker_deep_levels(self._h, None, None, 0, C.byref(n)))
        lv = np.zeros(max(1, n.value), dtype=np.int32)
        pr = np.zeros(max(1, n.value), dtype=np.int32)
        check(lib.vsrmc_checker_deep_levels(self._h, _p(lv), _p(pr), len(lv), C.byref(n)))
        if self._deep is None:
            raise ValueError("no predicates are attached (deep_attach)")
        state, step = self._deep
        none = (1 << 64) - 1
        out = []
        for i in range(n.value):
            d, w, s = capi.DeepInfo(), capi.WhereInfo(), capi.StepInfo()
            check(lib.vsrmc_checker_deep_result(self._h, int(lv[i]), int(pr[i]), C.byref(d), C.byref(w), C.byref(s)))
            r = dict(level=d.level, kind=self.DEEP_KINDS[d.kind], exact=bool(d.exact), slices=int(d.slices), n_hit_states=int(d.n_hit_states),
                     n_hit_pairs=int(d.n_hit_pairs), where_ms=d.where_ms, step_ms=d.step_ms, state=None, step=None)
            if d.has_state:
                ns = len(state.names)
                r["state"] = dict(n_states=int(w.n_states), count=[int(w.count[k]) for k in range(ns)],
                                  min_fp=[None if w.min_fp[k] == none else int(w.min_fp[k]) for k in range(ns)])
            if d.has_step:
                ns = len(step.names)
                r["step"] = dict(n_states=int(s.n_states), n_pairs=int(s.n_pairs), n_err=int(s.n_err), count=[int(s.count[k]) for k in range(ns)],
                                 min_fp=[None if s.min_fp[k] == none else int(s.min_fp[k]) for k in range(ns)], slices=int(s.slices))
            out.append(r)
        return out

    def deep_where_states(self, level, probed=False):
        """The states of a level deep_results() lists that satisfy any state predicate -> (fingerprints ascending, their bits); the contract of
        where_states() (VsrmcError -5 when the list overflowed)."""
        n = C.c_uint64()
        lib = capi.load()
        rc = lib.vsrmc_checker_deep_where_states(self._h, level, int(probed), None, None, 0, C.byref(n))
        if rc not in (0, -5):
            check(rc)
        fps = np.zeros(max(1, n.value), dtype=np.uint64)
        bits = np.zeros(max(1, n.value), dtype=np.uint8)
        check(lib.vsrmc_checker_deep_where_states(self._h, level, int(probed), _p(fps), _p(bits), len(fps), C.byref(n)))
        return fps[: n.value].copy(), bits[: n.value].copy()

    def deep_step_pairs(self, level):
        """The pairs out of a level deep_results() lists that satisfy any step predicate -> (parent fingerprints, ordinals, bits), by (fingerprint,
        ordinal); the ordinals are positions in the scratch records of the descent that scanned the level."""
        n = C.c_uint64()
        lib = capi.load()
        rc = lib.vsrmc_checker_deep_step_pairs(self._h, level, None, None, None, 0, C.byref(n))
        if rc not in (0, -5):
            check(rc)
        fps = np.zeros(max(1, n.value), dtype=np.uint64)
        ords = np.zeros(max(1, n.value), dtype=np.uint32)
        bits = np.zeros(max(1, n.value), dtype=np.uint8)
        check(lib.vsrmc_checker_deep_step_pairs(self._h, level, _p(fps), _p(ords), _p(bits), len(fps), C.byref(n)))
        return fps[: n.value].copy(), ords[: n.value].copy(), bits[: n.value].copy()

    def deep_witness_trace(self, level=None, program=None, k=None, probed=False):
        """The behaviour from Init into a hit of an attached program (vsrmc_checker_deep_witness), the same one in every run: [(action name, record)].
        No arguments: the witness run(deep=True) stopped at.  Otherwise program "state" (probed=True: the level as a probed level) or "step" (the
        behaviour into the parent plus the successor of the pair) and k, a number or a name."""
        if level is None:
            wit = self.witness
            if wit is None or "kind_of_level" not in wit:
                raise ValueError("run(deep=True) has not stopped at a hit beyond the record buffers")
            level, program, k, probed = wit["level"], wit["program"], wit["k"], wit["kind_of_level"] == "probed"
        if self._deep is None:
            raise ValueError("no predicates are attached (deep_attach)")
        w = self._deep[0 if program == "state" else 1]
        if w is None:
            raise ValueError("no %s program is attached" % program)
        if not isinstance(k, int):
            k = w.names.index(k)
        which = 1 if program == "step" else 2 if probed else 0
        lay = self.model.layout
        cap_w = (level + 3) * int(lay.max_record_words)
        words = np.zeros(cap_w, dtype=np.uint64)
        off = np.zeros(level + 4, dtype=np.uint64)
        acts = np.zeros(level + 4, dtype=np.int32)
        n = C.c_uint64()
        check(capi.load().vsrmc_checker_deep_witness(self._h, level, which, k, _p(words), cap_w, _p(off), _p(acts), len(off), C.byref(n)))
        return [(ACTION_NAMES[acts[t]], words[int(off[t]): int(off[t + 1])].copy()) for t in range(n.value)]

    def deep_terminal_attach(self):
        """Attach the deadlock check to the search beyond the record buffers (vsrmc_checker_deep_terminal_attach): every deepen() — and every deepen
        inside advance() / run() / check() — then scans the levels that exist in the seen-set only for terminal states (k_terminal on every scratch
        slice, each level once) and the probed level as well (k_probe_children writes its states chunk by chunk, k_terminal reads them).  A second call
        is a no-op.  Results: deep_terminal_results()."""
        check(capi.load().vsrmc_checker_deep_terminal_attach(self._h))

    def deep_terminal_results(self):
        """The per-level results of the terminal attachment, ascending by (level, probed) -> [dict(level, kind in DEEP_KINDS, exact, slices, chunks,
        n_states (kind "probed": the copies scanned), n_terminal, n_unsettled, min_fp, min_fp_unsettled, n_listed, bytes_written, ms, children_ms)];
        fingerprints None where there is no such state.  kind "probed": distinct states, lower bounds when exact is False."""
        lib = capi.load()
        n = C.c_uint64()
        check(lib.vsrmc_checker_deep_terminal_levels(self._h, None, None, 0, C.byref(n)))
        lv = np.zeros(max(1, n.value), dtype=np.int32)
        pr = np.zeros(max(1, n.value), dtype=np.int32)
        check(lib.vsrmc_checker_deep_terminal_levels(self._h, _p(lv), _p(pr), len(lv), C.byref(n)))
        none = (1 << 64) - 1
        out = []
        for i in range(n.value):
            d = capi.DeepTerminalInfo()
            check(lib.vsrmc_checker_deep_terminal_result(self._h, int(lv[i]), int(pr[i]), C.byref(d)))
            out.append(dict(level=d.level, kind=self.DEEP_KINDS[d.kind], exact=bool(d.exact), slices=int(d.slices), chunks=int(d.chunks), n_states=int(d.n_states),
                            n_terminal=int(d.n_terminal), n_unsettled=int(d.n_unsettled), min_fp=None if d.min_fp == none else int(d.min_fp),
                            min_fp_unsettled=None if d.min_fp_unsettled == none else int(d.min_fp_unsettled), n_listed=int(d.n_listed),
                            bytes_written=int(d.bytes_written), ms=d.ms, children_ms=d.children_ms))
        return out

    def deep_terminal_states(self, level, probed=False):
        """The terminal states of a level deep_terminal_results() lists -> (fingerprints ascending, flag bytes: bit 0 set, bit 1 = unsettled); the
        contract of terminal_states() (VsrmcError -5 when the list overflowed)."""
        n = C.c_uint64()
        lib = capi.load()
        rc = lib.vsrmc_checker_deep_terminal_states(self._h, level, int(probed), None, None, 0, C.byref(n))
        if rc not in (0, -5):
            check(rc)
        fps = np.zeros(max(1, n.value), dtype=np.uint64)
        flags = np.zeros(max(1, n.value), dtype=np.uint8)
        check(lib.vsrmc_checker_deep_terminal_states(self._h, level, int(probed), _p(fps), _p(flags), len(fps), C.byref(n)))
        return fps[: n.value].copy(), flags[: n.value].copy()

    def deep_terminal_trace(self, level=None, probed=False, unsettled=False):
        """The behaviour from Init into the terminal state (unsettled=True: the unsettled terminal state) with the smallest fingerprint of a level
        the terminal attachment examined (vsrmc_checker_deep_terminal_witness), the same one in every run: [(action name, record)].  level=None: the
        deadlock run(check_deadlock=True, deep=True) stopped at."""
        if level is None:
            d = self.deadlock
            if d is None or "kind_of_level" not in d:
                raise ValueError("run(check_deadlock=True, deep=True) has not stopped at a terminal state beyond the record buffers")
            level, probed = d["level"], d["kind_of_level"] == "probed"
        lay = self.model.layout
        cap_w = (level + 3) * int(lay.max_record_words)
        words = np.zeros(cap_w, dtype=np.uint64)
        off = np.zeros(level + 4, dtype=np.uint64)
        acts = np.zeros(level + 4, dtype=np.int32)
        n = C.c_uint64()
        check(capi.load().vsrmc_checker_deep_terminal_witness(self._h, level, int(probed), int(unsettled), _p(words), cap_w, _p(off), _p(acts), len(off), C.byref(n)))
        return [(ACTION_NAMES[acts[t]], words[int(off[t]): int(off[t + 1])].copy()) for t in range(n.value)]

    def probe(self):
        """Expand the newest level without storing it: invariants of every successor that is not an earlier-level state are
        checked, nothing is inserted or written (no frontier memory needed; the search cannot continue afterwards).  Also valid
        right after a step() that failed with "frontier full".  -> dict(level, generated, viol_fp, viol_mask, parent_index, ...)"""
        info = capi.LevelInfo()
        check(capi.load().vsrmc_checker_probe(self._h, C.byref(info)))
        d = info.as_dict()
        d["parent_index"] = d.pop("viol_index")
        if d["viol_mask"] and self.violation is None:
            self.violation = dict(level=d["level"], index=None, fp=d["viol_fp"], mask=d["viol_mask"], probed=True)
        return d

    def probe2(self):
        """Two levels beyond the newest one without storing either: level+1 as a virtual level (fingerprints claimed, exact count,
        invariants), level+2 as a probe over slices of regenerated level+1 states.  -> (virtual level dict, probe level dict)"""
        v, p = capi.LevelInfo(), capi.LevelInfo()
        check(capi.load().vsrmc_checker_probe2(self._h, C.byref(v), C.byref(p)))
        dv, dp = v.as_dict(), p.as_dict()
        for d in (dv, dp):
            d["ancestor_index"] = d.pop("viol_index")
            if d["viol_mask"] and self.violation is None:
                self.violation = dict(level=d["level"], index=None, fp=d["viol_fp"], mask=d["viol_mask"], probed=True)
        return dv, dp

    def probe3(self):
        """Three levels beyond the newest one without storing any: level+1 and level+2 as virtual levels, level+3 as a probe over
        regenerated sub-slices (level is expanded three times, level+1 twice).  -> (virtual dict, virtual dict, probe dict); a
        violation in a virtual level ends the call early (the later dicts then have level 0)."""
        v1, v2, p = capi.LevelInfo(), capi.LevelInfo(), capi.LevelInfo()
        check(capi.load().vsrmc_checker_probe3(self._h, C.byref(v1), C.byref(v2), C.byref(p)))
        out = [v1.as_dict(), v2.as_dict(), p.as_dict()]
        for d in out:
            d["ancestor_index"] = d.pop("viol_index")
            if d["viol_mask"] and self.violation is None:
                self.violation = dict(level=d["level"], index=None, fp=d["viol_fp"], mask=d["viol_mask"], probed=True)
        return tuple(out)

    def regen_launches(self):
        """Regenerating passes of the deep search this checker has run with the kernel of their own (csrc/vsr_regen_bits.hpp) since it was created."""
        n = C.c_uint64()
        check(capi.load().vsrmc_checker_regen_launches(self._h, C.byref(n)))
        return n.value

    def probe_violators(self):
        """fingerprints (ascending) of the distinct violating states of the level the last probe / deepen / advance call probed"""
        n = C.c_uint64()
        check(capi.load().vsrmc_checker_probe_violators(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), dtype=np.uint64)
        check(capi.load().vsrmc_checker_probe_violators(self._h, _p(out), len(out), C.byref(n)))
        return [int(x) for x in out[: n.value]]

    def probe_trace(self):
        """The counter-example of the violation probe() reported: [(action name, record)] from Init to the violator."""
        lay = self.model.layout
        n_max = max(self.level, self.depth) + 3                 # (the deepest level in the seen-set + the probed state beyond it)
        cap_w = (n_max + 1) * int(lay.max_record_words)
        words = np.zeros(cap_w, dtype=np.uint64)
        off = np.zeros(n_max + 2, dtype=np.uint64)
        acts = np.zeros(n_max + 2, dtype=np.int32)
        n = C.c_uint64()
        check(capi.load().vsrmc_checker_probe_trace(self._h, _p(words), cap_w, _p(off), _p(acts), len(off), C.byref(n)))
        return [(ACTION_NAMES[acts[t]], words[int(off[t]): int(off[t + 1])].copy()) for t in range(n.value)]

    def trace_to_violator(self, fp):
        """The counter-example that ends in the violating state `fp` of the last probed level (one of probe_violators()), as the search reached it:
        [(action name, record)] from Init.  probe_trace() is this for probe_violators()[0]."""
        lay = self.model.layout
        n_max = max(self.level, self.depth) + 3
        cap_w = (n_max + 1) * int(lay.max_record_words)
        words = np.zeros(cap_w, dtype=np.uint64)
        off = np.zeros(n_max + 2, dtype=np.uint64)
        acts = np.zeros(n_max + 2, dtype=np.int32)
        n = C.c_uint64()
        check(capi.load().vsrmc_checker_trace_to_violator(self._h, int(fp), _p(words), cap_w, _p(off), _p(acts), len(off), C.byref(n)))
        return [(ACTION_NAMES[acts[t]], words[int(off[t]): int(off[t + 1])].copy()) for t in range(n.value)]

    def close(self):
        if self._h:
            capi.load().vsrmc_checker_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
