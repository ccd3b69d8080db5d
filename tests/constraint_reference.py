"""Reference for the state-constraint tests (test_constraint_cpu.py, test_constraint_gpu.py): a Python BFS over the CPU oracles' successor function
(`orc.successors`; `orc2` / `orc3` for the analysis models) in which a successor that fails the constraint is OUT OF MODEL — generated and counted, but
no distinct state and never expanded.  The constraint is a hand-written Python function over `pycodec.unpack` (`pyoracle2.unpack` /
`pyoracle3.unpack`) of a record: nothing here reads a predicate's text.  States are identified by the oracle's fingerprint (VIEW + SYMMETRY), which is
what the checker's seen-set holds; a constraint is a function of the VIEW and symmetric, so every copy of a state gets the same verdict.

constrained_bfs(...) -> Result: per level (level 1 = Init) the fingerprint set of the in-model new states, the fingerprint set of the pruned states and
`generated` (the successors generated out of the level BEFORE, as the checker's level info counts them), the in-model total, and — from a second,
unconstrained search — the set "reachable without the constraint and satisfying it", of which `unreachable` are the states the constrained search
never reaches: what separates a constraint from filtering a finished search."""
import collections
import time

import numpy as np

Level = collections.namedtuple("Level", "level kept pruned generated")          # kept / pruned: {fingerprint: wire record}
Result = collections.namedtuple("Result", "levels in_model pruned_total depth satisfying unreachable seconds")
MASK = (1 << 64) - 1


# ---- the constraints, restated (the texts: tools/constraints_example.txt, tools/constraints_models_example.txt) -------------------------------
def narrow_network(s):
    """every two keys with count > 0 and the same dest agree in type, source, view_number and op_number (an absent op_number reads 0)"""
    by_dest = {}
    for m, c in s["messages"].items():
        if c > 0:
            d = dict(m)
            by_dest.setdefault(d["dest"], set()).add((d["type"], d["source"], d["view_number"], d.get("op_number", 0)))
    return all(len(v) == 1 for v in by_dest.values())


def replica3_normal(s):
    from oracle import pyoracle as po
    return s["rep_status"][2] == po.Normal


def views_below(k):
    return lambda s: all(v < k for v in s["rep_view_number"])


def not_all_in_view_change(s):
    """the invariant of test 6: the replicas are never all in ViewChange status at once.  Under Replica3Normal no in-model state can violate it; the
    states that do are successors of in-model states, pruned on arrival"""
    from oracle import pyoracle as po
    return not all(st == po.ViewChange for st in s["rep_status"])


def r3normal_commit_below2(s):
    """Replica3Normal and no commit number above 1: on (3,1,{v1,v2},1) the first state that violates AcknowledgedWritesExistOnMajority (level 19) has a
    commit number of 2 — it is generated from an in-model state and pruned on arrival"""
    return replica3_normal(s) and all(c < 2 for c in s["rep_commit_number"])


def no_state_transfer(s):
    from oracle import pyoracle2 as p2
    return all(st != p2.StateTransfer for st in s["rep_status"])


def init_only(s):
    """true of Init and of no successor of Init: nothing has been sent or timed out"""
    return len(s["messages"]) == 0 and all(v == 1 for v in s["rep_view_number"])


TEXTS = {
    "NarrowNetwork": r"""NarrowNetwork == \A m1 \in DOMAIN messages : \A m2 \in DOMAIN messages : (messages[m1] > 0 /\ messages[m2] > 0 /\ m1.dest = m2.dest) =>
        (m1.type = m2.type /\ m1.source = m2.source /\ m1.view_number = m2.view_number /\ m1.op_number = m2.op_number)""",
    "Replica3Normal": r"Replica3Normal == rep_status[3] = Normal",
    "R3NormalCommitBelow2": r"R3NormalCommitBelow2 == rep_status[3] = Normal /\ (\A r \in replicas : rep_commit_number[r] < 2)",
    "NotAllInViewChange": r"NotAllInViewChange == ~(\A r \in replicas : rep_status[r] = ViewChange)",
    "NoStateTransfer": r"NoStateTransfer == \A r \in replicas : rep_status[r] # StateTransfer",
    "InitOnly": r"InitOnly == (\A m \in DOMAIN messages : FALSE) /\ (\A r \in replicas : rep_view_number[r] = 1)",
    "True": r"True == TRUE",
    "False": r"False == FALSE",
}


def oracle_of(which):
    """which: "first" (VSR.tla), "second", "third" -> (orc module, unpack(PM, words), make PM)"""
    if which == "first":
        from oracle import orc, pycodec, pyoracle as po
        return orc, pycodec.unpack, lambda R, C, n, L: po.Model(R, C, tuple("v%d" % (i + 1) for i in range(n)), L)
    if which == "second":
        from oracle import orc2, pyoracle2
        return orc2, pyoracle2.unpack, lambda R, C, n, L: pyoracle2.Model(R, tuple("v%d" % (i + 1) for i in range(n)), L)
    from oracle import orc3, pyoracle3
    return orc3, pyoracle3.unpack, lambda R, C, n, L: pyoracle3.Model(R, tuple("abc"[:n]), L)


def params_of(which, R, C, n, L, invariant_mask=None):
    """invariant_mask (VSR.tla only): which built-in invariants the oracle evaluates (orc.invariants, `inv` of a successor); the search itself does not depend on it"""
    orc = oracle_of(which)[0]
    if which == "first":
        return orc.Params(R, C, n, L) if invariant_mask is None else orc.Params(R, C, n, L, invariant_mask=invariant_mask)
    return orc.Params(R, n, L)


def constrained_bfs(which, R, C, n, L, constraint, max_levels=None, with_unconstrained=True):
    """the constrained search, whole or to `max_levels` levels; with_unconstrained: also the plain search (to the same cap), for `satisfying` / `unreachable`"""
    t0 = time.time()
    orc, unpack, make_pm = oracle_of(which)
    P = params_of(which, R, C, n, L)
    PM = make_pm(R, C, n, L)
    verdict = {}                                                   # fingerprint -> constraint(state): one evaluation per state, shared by both searches

    def ok(fp, rec):
        if fp not in verdict:
            verdict[fp] = bool(constraint(unpack(PM, [int(x) for x in rec])))
        return verdict[fp]

    def search(constrained):
        init = orc.init_record(P)
        fp0 = orc.fingerprint(P, init)[0]
        seen = {fp0}
        first = Level(1, {fp0: init} if (not constrained or ok(fp0, init)) else {}, {} if (not constrained or ok(fp0, init)) else {fp0: init}, 0)
        levels = [first]
        while levels[-1].kept and (max_levels is None or len(levels) < max_levels):
            kept, pruned, generated = {}, {}, 0
            for rec in levels[-1].kept.values():
                for s in orc.successors(P, rec):
                    generated += 1
                    if s["fp"] in seen:
                        continue
                    seen.add(s["fp"])
                    (kept if (not constrained or ok(s["fp"], s["words"])) else pruned)[s["fp"]] = s["words"]
            if not kept and not pruned:
                break
            levels.append(Level(len(levels) + 1, kept, pruned, generated))
        return levels

    levels = search(True)
    reached = set(fp for lv in levels for fp in lv.kept)
    satisfying = unreachable = None
    if with_unconstrained:
        plain = search(False)
        satisfying = set(fp for lv in plain for fp, rec in lv.kept.items() if ok(fp, rec))
        unreachable = satisfying - reached
    depth = max([lv.level for lv in levels if lv.kept] or [1])     # the deepest level with an in-model state (an empty model: 1)
    return Result(levels, len(reached), sum(len(lv.pruned) for lv in levels), depth, satisfying, unreachable, time.time() - t0)


def fps_of(d):
    return np.array(sorted(d), dtype=np.uint64)


def xor_sum(d):
    x = s = 0
    for fp in d:
        x ^= fp
        s = (s + fp) & MASK
    return x, s
