"""Reference of test_constrained_seeded_cpu.py / test_constrained_seeded_gpu.py (constrained_seeded_worker.py): the constrained level step over HARVESTED states, CPU only.

A two-level restatement of action_constraint_reference.constrained_bfs that starts from a seed set instead of Init: the seeds are the 1500-state sample
(deep_predicates_reference.state_indices) of deep_harvest.space(orc, key) at (5,1,2,1), (4,1,2,1) and (3,2,3,1) under assume_commit_number.  THE SEEDS ARE LEVEL 1
AS GIVEN, SUBJECT TO NEITHER CONSTRAINT (as Init is not subject to an action constraint; unlike Init, they are not subject to the state constraint either: no
seed is pruned).  From there on the semantics are the checker's: a transition that fails the action constraint is generated and counted but
NOT TAKEN; a successor that arrives through a permitted transition and is not in an earlier level is new, holds a seen-set slot from then on, and is KEPT or
PRUNED by the state constraint; level 3 is stepped from the kept level-2 states, and the pruned ones count as "in an earlier level".

Every value comes from the C++ CPU oracle (orc.successors / fingerprint / invariants) and from the hand-written Python predicates of deep_predicates_reference.py
over pycodec.unpack: nothing here reads a predicate's text.  The constraints read what exists only at R >= 4 (the fourth word of a replica block, the appended
entries of a broadcast to R - 1 destinations) or only at C = 2 (the second row of a client table, client_id = 2 in a log entry).  A negated constraint is
`~(text)` beside `not f(..)`.  Each program exports two or three further predicates of the same set beside the constraint, so that pruned_count /
pruned_min_fp_k have something to count and the constraint's bit is not bit 0 everywhere.

A state is identified by the oracle's fingerprint (VIEW + SYMMETRY), so one state can arrive as two records that are value permutations of each other.  The
figures do not depend on which arrives (the predicates name no value); the RECORDS do, so a level-3 step expands every copy of a kept level-2 state that a
permitted producer of the smallest auxkey wrote: the figures are counted on the first copy (and asserted equal on the others), the candidate records of a new
state come from all of them."""
import collections

import deep_harvest as dh
import deep_predicates_reference as dp
from oracle import pycodec

M64 = (1 << 64) - 1
PFP_MASK = (1 << 45) - 1
SPACES = [(5, 1, 2, 1), (4, 1, 2, 1), (3, 2, 3, 1)]
IDS = ["%d-%d-%d-%d" % k for k in SPACES]


def _of(preds, name):
    return next(p for p in preds if p[0] == name)


def state_not(preds, name):
    n, t, f = _of(preds, name)
    return ("Not" + n, "~(%s)" % t, lambda s: not f(s))


def step_not(preds, name):
    n, t, f = _of(preds, name)
    return ("Not" + n, "~(%s)" % t, lambda p, c, a: not f(p, c, a))


def _program(preds, constraint):
    """(predicates in export order, index of the constraint among them)"""
    return dict(preds=preds, k=[p[0] for p in preds].index(constraint), name=constraint)


def _r4():
    return dict(
        action=_program([_of(dp.STEP, "DvcGrew"), _of(dp.STEP, "TailUnchanged"), _of(dp.STEP, "PeerTailMoves")], "TailUnchanged"),
        state=_program([_of(dp.STATE, "DvcHeld"), _of(dp.STATE, "SvcFour"), state_not(dp.STATE, "DvcQuorum"), _of(dp.STATE, "MsgTail")], "NotDvcQuorum"),
        second=_program([step_not(dp.STEP, "NewKeyForLast"), _of(dp.STEP, "DvcGrew"), _of(dp.STEP, "TailStatusView")], "NotNewKeyForLast"),
        e_state=None, step_set=dp.STEP)


PROGRAMS = {
    (5, 1, 2, 1): _r4(),
    (4, 1, 2, 1): _r4(),
    (3, 2, 3, 1): dict(
        action=_program([_of(dp.STEP_C2, "ExecutedRose"), _of(dp.STEP_C2, "Row1Unchanged"), _of(dp.STEP_C2, "LastClientEntryAppended")], "Row1Unchanged"),
        state=_program([_of(dp.STATE_C2, "Client2Pending"), _of(dp.STATE_C2, "Client2Committed"), _of(dp.STATE_C2, "RowsDiffer"), _of(dp.STATE_C2, "MsgOfClient2")],
                       "Client2Committed"),
        second=_program([step_not(dp.STEP_C2, "LastClientEntryAppended"), _of(dp.STEP_C2, "Row1RewrittenByClient2"), _of(dp.STEP_C2, "ExecutedRose")],
                        "NotLastClientEntryAppended"),
        e_state=_program([_of(dp.STATE_C2, "Client2Pending"), _of(dp.STATE_C2, "LaterClientLater"), state_not(dp.STATE_C2, "RowsDiffer")], "NotRowsDiffer"),
        step_set=dp.STEP_C2),
}
TRUE_STATE = _program([("True", "TRUE", lambda s: True)], "True")
TRUE_STEP = _program([("True", "TRUE", lambda p, c, a: True)], "True")

# What the oracle gives on the sample (measured when the cases were fixed; the sample is deterministic: test_constrained_seeded_cpu.py holds the reference to at
# least half of every figure, a margin against a deliberate change of the harvest, not against noise).  level2 / level3: the two steps of case (c), both
# constraints attached; rescued: new states, kept or pruned, with a blocked incoming edge (of the level-2 ones the state constraint keeps 1, 0 and 32; of the
# level-3 ones all); blocked_actions: the action ids with a blocked instance; all_blocked: seeds of which every instance is blocked (live parents that
# contribute nothing; `deadlocks` stays 0: no seed is terminal); second: the second action constraint alone, level 2; viol_*: the successors of the sample that
# fail AcknowledgedWritesExistOnMajority (invariant mask 3) — blocked by the first action constraint, or permitted and new under it / under the second one, and
# at two clients the permitted-new ones that ~RowsDiffer prunes.
MEASURED = {
    (5, 1, 2, 1): dict(level2=dict(generated=12745, blocked=3969, blocked_actions=9, new=8202, rescued=14, kept=4996, pruned=3206),
                       level3=dict(generated=63792, blocked=2640, new=32420, kept=31746, pruned=674, rescued=28),
                       second=dict(blocked=2548, blocked_actions=6, rescued=13), all_blocked=309,
                       viol_blocked=5, viol_new=0, viol_new_second=5, viol_pruned=0),
    (4, 1, 2, 1): dict(level2=dict(generated=7983, blocked=1510, blocked_actions=9, new=5633, rescued=26, kept=3775, pruned=1858),
                       level3=dict(generated=24555, blocked=109, new=10137, kept=9773, pruned=364, rescued=0),     # (3 rescued: not floored)
                       second=dict(blocked=940, blocked_actions=5, rescued=29), all_blocked=237,
                       viol_blocked=11, viol_new=0, viol_new_second=11, viol_pruned=0),
    (3, 2, 3, 1): dict(level2=dict(generated=6193, blocked=930, blocked_actions=3, new=4788, rescued=42, kept=3074, pruned=1714),
                       level3=dict(generated=10290, blocked=1681, new=6002, kept=6002, pruned=0, rescued=82),
                       second=dict(blocked=1098, blocked_actions=4, rescued=24), all_blocked=0,
                       viol_blocked=0, viol_new=9, viol_new_second=9, viol_pruned=6),
}


def floors(d):
    """half of every measured figure of a dict of MEASURED (0 = not a condition)"""
    return {k: (v + 1) // 2 for k, v in d.items() if isinstance(v, int) and v}


class Space:
    """the sample of one space: wire records, fingerprints, the oracle's parameters per invariant mask, the Python views"""

    def __init__(self, orc, key):
        self.orc, self.key = orc, key
        self.policy = dh.policy(key)
        h = dh.space(orc, key)
        idx = dp.state_indices(len(h))
        assert len(set(idx)) == dp.N_STATES
        self.recs = [h.records[i] for i in idx]
        self.fps = [h.fps[i] for i in idx]
        self.PM = dh.py_model(key)
        self.P = dh.params(orc, key)
        self._params = {1: self.P}
        self.perms = 1
        for k in range(2, key[2] + 1):
            self.perms *= k
        self._seed_expansion = None

    def params(self, inv_mask):
        if inv_mask not in self._params:
            self._params[inv_mask] = dh.params(self.orc, self.key, invariant_mask=inv_mask)
        return self._params[inv_mask]

    def view(self, words):
        return pycodec.unpack(self.PM, [int(x) for x in words])

    def norm(self, words):
        return tuple(int(x) for x in self.orc.normalise(self.P, words))

    def seeds(self):
        """the seeds as the parents of a step: [(fingerprint, [record])]"""
        return [(f, [r]) for f, r in zip(self.fps, self.recs)]

    def expansion(self, parents, cached=False):
        """per parent, per copy: (record, its view, the oracle's successors, their views).  cached: the seeds' (every case of a space steps them)"""
        if cached and self._seed_expansion is not None:
            return self._seed_expansion
        out = []
        for _fp, copies in parents:
            per = []
            for rec in copies:
                succ = self.orc.successors(self.P, rec)
                per.append((rec, self.view(rec), succ, [self.view(s["words"]) for s in succ]))
            out.append(per)
        if cached:
            self._seed_expansion = out
        return out

    def batch(self):
        import numpy as np
        return np.concatenate(self.recs), np.cumsum([0] + [len(r) for r in self.recs]).astype(np.uint64)


class Step:
    """what one constrained step yields (the module docstring of the tests lists the fields)"""

    def words_dev(self, sp, fp):
        """words of a new state in device layout: the wire record and one view hash per value permutation"""
        return len(self.record[fp]) + sp.perms

    def copies(self, sp, fp):
        """the distinct records (bag order aside) a permitted producer of the smallest auxkey wrote for the new state fp"""
        best = min(ak for ak, _i, _s, _a in self.producers[fp])
        seen, out = set(), []
        for ak, _i, s, _a in self.producers[fp]:
            n = sp.norm(s["words"])
            if ak == best and n not in seen:
                seen.add(n)
                out.append(s["words"])
        return out


def step(sp, parents, earlier, action=None, state=None, inv_mask=1, seeds=False):
    """One step from `parents` ([(fingerprint, [copies of the record])]; parent number = position) under the action constraint `action` and the state constraint
    `state` (programs of PROGRAMS, or None), `earlier` = the fingerprints of every earlier level, the pruned ones included -> Step:
      parents, generated, act[16], deadlocks (parents without any instance), live_blocked (parents with instances, all of them blocked)
      blocked, blocked_act {action id: n}, blocked_min_fp (the smallest PARENT fingerprint of a blocked pair, None without one), blocked_targets
      blocked_violating, blocked_viol_mask, blocked_viol_min_fp: the same over blocked pairs whose successor fails a built-in invariant of inv_mask
      permitted, permitted_pairs [(parent number, parent view, child view, action id, successor)] (first copies)
      producers {new fingerprint: [(auxkey, parent number, successor, action id)]}: the permitted edges into states of no earlier level (every copy)
      new (ascending), ties (new fingerprints under two auxkeys), record {fp: the record under the smallest auxkey}, max_bag, viol {fp: mask} over ALL new
      kept / pruned (ascending), kept_xor, kept_sum, kept_max_bag, kept_words (device layout), pruned_min_fp
      pruned_count / pruned_min_fp_k {exported name: ..} over the pruned states
      rescued: the new states with a blocked incoming edge from this step — what a seen-set claim made before the verdict would lose; rescued_kept: those of
      them the state constraint keeps (the ones the level's records must hold)"""
    orc, P = sp.orc, sp.params(inv_mask)
    act_f = action["preds"][action["k"]][2] if action else None
    st = Step()
    st.parents, st.generated, st.act, st.deadlocks, st.live_blocked = len(parents), 0, [0] * 16, 0, 0
    st.inv_mask, st.max_instances = inv_mask, 0                      # (max_instances: the most instances of one parent — what a list of 64 entries must hold)
    st.blocked, st.blocked_act, st.blocked_min_fp, st.blocked_targets = 0, collections.Counter(), None, set()
    st.blocked_from = collections.defaultdict(set)                   # successor fingerprint -> numbers of the parents with a blocked edge into it
    st.blocked_violating, st.blocked_viol_mask, st.blocked_viol_min_fp = 0, 0, None
    st.permitted_pairs, st.producers = [], collections.defaultdict(list)
    for i, ((pfp, _copies), per) in enumerate(zip(parents, sp.expansion(parents, cached=seeds))):
        shape0 = None
        for ci, (_rec, pv, succ, views) in enumerate(per):
            shape = sorted((s["action"], s["fp"], s["auxkey"]) for s in succ)
            if ci == 0:
                shape0 = shape
                st.deadlocks += not succ
                st.max_instances = max(st.max_instances, len(succ))
            else:
                assert shape == shape0, "two copies of one state differ in more than a value permutation"
            n_ok = 0
            for s, cv in zip(succ, views):
                a = s["action"]
                ok = act_f is None or bool(act_f(pv, cv, orc.ACTIONS[a]))
                if ci == 0:
                    st.generated += 1
                    st.act[a] += 1
                    if ok:
                        n_ok += 1
                        st.permitted_pairs.append((i, pv, cv, a, s))
                    else:
                        st.blocked += 1
                        st.blocked_act[a] += 1
                        st.blocked_targets.add(s["fp"])
                        st.blocked_from[s["fp"]].add(i)
                        st.blocked_min_fp = pfp if st.blocked_min_fp is None else min(st.blocked_min_fp, pfp)
                        bad = orc.invariants(P, s["words"])
                        if bad:
                            st.blocked_violating += 1
                            st.blocked_viol_mask |= bad
                            st.blocked_viol_min_fp = pfp if st.blocked_viol_min_fp is None else min(st.blocked_viol_min_fp, pfp)
                if ok and s["fp"] not in earlier:
                    st.producers[s["fp"]].append((s["auxkey"], i, s, a))
            if ci == 0 and succ and not n_ok:
                st.live_blocked += 1
    st.permitted = st.generated - st.blocked
    st.new = sorted(st.producers)
    st.ties = [f for f in st.new if len(set(ak for ak, _i, _s, _a in st.producers[f])) > 1]
    st.record, st.viol, st.kept, st.pruned, st.max_bag = {}, {}, [], [], 0
    st.kept_xor = st.kept_sum = st.kept_max_bag = st.kept_words = 0
    names = [p[0] for p in state["preds"]] if state else []
    st.pruned_count, st.pruned_min_fp_k = {nm: 0 for nm in names}, {nm: None for nm in names}
    for f in st.new:
        rec = min(st.producers[f], key=lambda t: t[0])[2]["words"]
        st.record[f] = rec
        st.max_bag = max(st.max_bag, dh.bag_size(rec))
        bad = orc.invariants(P, rec)
        if bad:
            st.viol[f] = bad
        v = sp.view(rec) if state else None
        if state is None or state["preds"][state["k"]][2](v):
            st.kept.append(f)
            st.kept_xor ^= f
            st.kept_sum = (st.kept_sum + f) & M64
            st.kept_max_bag = max(st.kept_max_bag, dh.bag_size(rec))
            st.kept_words += len(rec) + sp.perms
        else:
            st.pruned.append(f)
            for nm, _t, fn in state["preds"]:
                if fn(v):
                    st.pruned_count[nm] += 1
                    st.pruned_min_fp_k[nm] = f if st.pruned_min_fp_k[nm] is None else min(st.pruned_min_fp_k[nm], f)
    st.pruned_min_fp = min(st.pruned) if st.pruned else None
    st.rescued = [f for f in st.new if f in st.blocked_targets]
    kept = set(st.kept)
    st.rescued_kept = [f for f in st.rescued if f in kept]
    return st


def figures(st):
    """the figures of MEASURED's level2 / level3 rows of one Step"""
    return dict(generated=st.generated, blocked=st.blocked, blocked_actions=len(st.blocked_act), new=len(st.new), rescued=len(st.rescued), kept=len(st.kept),
                pruned=len(st.pruned), rescued_kept=len(st.rescued_kept))


def two_levels(sp, action, state, inv_mask=1):
    """case (c): the step into level 2 from the seeds, then into level 3 from the kept level-2 states (in fingerprint order) -> (Step, Step, level-3 parents)"""
    s2 = step(sp, sp.seeds(), set(sp.fps), action, state, inv_mask, seeds=True)
    assert not s2.ties, "level 2: ties among the permitted producers"
    parents3 = [(f, s2.copies(sp, f)) for f in s2.kept]
    s3 = step(sp, parents3, set(sp.fps) | set(s2.new), action, state, inv_mask)
    assert not s3.ties, "level 3: ties among the permitted producers"
    return s2, s3, parents3


def trace_parent(st, parents, fp):
    """number of the parent a behaviour into the new state fp goes through: the smallest (auxkey, low 45 bits of its fingerprint) among the PERMITTED producers"""
    return min(((ak, parents[i][0] & PFP_MASK), i) for ak, i, _s, _a in st.producers[fp])[1]
