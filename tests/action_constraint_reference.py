"""Reference for the action-constraint tests (test_action_constraint_cpu.py, test_action_constraint_gpu.py): a Python BFS over the CPU oracles' successor
function (`orc.successors`; `orc2` / `orc3` for the analysis models) in which a transition that fails the step predicate is NOT TAKEN — generated and
counted, but its successor is not added to `seen` and may still enter the model through a permitted transition, of the same level or a later one
(DESIGN.md §9i).  The predicate is a hand-written Python function f(parent, child, action name) over the unpacked records (tests/step_reference.py,
tests/step_models_reference.py): nothing here reads a predicate's text.  States are identified by the oracle's fingerprint (VIEW + SYMMETRY).

constrained_bfs(...) -> Result: per level (level 1 = Init, not subject to the action constraint) the new states, `generated` / `act_generated` /
`blocked` / `blocked_act` of the step that led into it (per action NAME), the states a state constraint pruned on arrival (with one attached: they keep
their place in `seen`, §9h), and the RESCUED states: the new in-model states with at least one blocked incoming edge from the level before — what a
per-state filter, or a seen-set claim made before the verdict, would lose.  The set of every level does not depend on the order parents are taken in: a
state is new in level l + 1 exactly if it is not in levels 1 .. l and some level-l state has a permitted transition to it."""
import collections
import time

import numpy as np

import constraint_reference as cr

Level = collections.namedtuple("Level", "level new pruned generated act_generated blocked blocked_act rescued")   # new / pruned: {fingerprint: wire record}
Result = collections.namedtuple("Result", "levels states generated blocked depth rescued seconds")
MASK = cr.MASK
oracle_of, params_of, fps_of, xor_sum = cr.oracle_of, cr.params_of, cr.fps_of, cr.xor_sum


# ---- the action constraints, restated (the texts: tools/action_constraints_example.txt) ---------------------------------------------------------
def quiet_client(p, c, a):
    """a client request is received only while no message is in flight: every key of the parent's bag has count 0"""
    return a != "ReceiveClientRequest" or all(n == 0 for n in p["messages"].values())


def commit_never_decreases(p, c, a):
    return all(cc >= pc for pc, cc in zip(p["rep_commit_number"], c["rep_commit_number"]))


def timers_in_view_1(p, c, a):
    """the view-change timer fires only while every replica is in view 1"""
    return a != "TimerSendSVC" or all(v == 1 for v in p["rep_view_number"])


def always(p, c, a):
    return True


def never(p, c, a):
    return False


def primed(state_pred):
    """a state predicate read in the successor: as an action constraint it keeps, from level 2 on, what the state constraint of the same text keeps"""
    return lambda p, c, a: state_pred(c)


TEXTS = {
    "QuietClient": r"QuietClient == step_action = ReceiveClientRequest => \A m \in DOMAIN messages : messages[m] = 0",
    "CommitNeverDecreases": r"CommitNeverDecreases == \A r \in replicas : rep_commit_number'[r] >= rep_commit_number[r]",
    "TimersInView1": r"TimersInView1 == step_action = TimerSendSVC => \A r \in replicas : rep_view_number[r] = 1",
    "True": r"True == TRUE",
    "False": r"False == FALSE",
    "NarrowNetworkPrimed": r"""NarrowNetworkPrimed == \A m1 \in DOMAIN messages' : \A m2 \in DOMAIN messages' : (messages'[m1] > 0 /\ messages'[m2] > 0 /\ m1.dest = m2.dest) =>
        (m1.type = m2.type /\ m1.source = m2.source /\ m1.view_number = m2.view_number /\ m1.op_number = m2.op_number)""",
}


def constrained_bfs(which, R, C, n, L, pred, max_levels=None, state_constraint=None, action_names=None):
    """the search that takes only the transitions `pred` permits, whole or to `max_levels` levels.  state_constraint (a function of one unpacked state):
    attached as well — a successor that arrives through a permitted transition and fails it is pruned on arrival (it stays in `seen`), Init included."""
    t0 = time.time()
    orc, unpack, make_pm = oracle_of(which)
    P = params_of(which, R, C, n, L)
    PM = make_pm(R, C, n, L)
    if action_names is None:
        import vsr_tlaplus_amd as vt
        action_names = vt.ACTION_NAMES
    views = {}

    def view(rec):
        key = tuple(int(x) for x in rec)
        if key not in views:
            views[key] = unpack(PM, list(key))
        return views[key]

    init = orc.init_record(P)
    fp0 = orc.fingerprint(P, init)[0]
    seen = {fp0}
    init_ok = state_constraint is None or bool(state_constraint(view(init)))
    levels = [Level(1, {fp0: init} if init_ok else {}, {} if init_ok else {fp0: init}, 0, {}, 0, {}, {})]
    while levels[-1].new and (max_levels is None or len(levels) < max_levels):
        new, pruned, generated, blocked = {}, {}, 0, 0
        act_generated, blocked_act = collections.Counter(), collections.Counter()
        blocked_targets = set()
        for rec in levels[-1].new.values():
            pv = view(rec)
            for s in orc.successors(P, rec):
                a = action_names[s["action"]]
                generated += 1
                act_generated[a] += 1
                if not pred(pv, view(s["words"]), a):
                    blocked += 1
                    blocked_act[a] += 1
                    blocked_targets.add(s["fp"])
                    continue
                if s["fp"] in seen:
                    continue
                seen.add(s["fp"])
                if state_constraint is None or state_constraint(view(s["words"])):
                    new[s["fp"]] = s["words"]
                else:
                    pruned[s["fp"]] = s["words"]
        views.clear()
        rescued = {fp: new[fp] for fp in blocked_targets if fp in new}
        levels.append(Level(len(levels) + 1, new, pruned, generated, dict(act_generated), blocked, dict(blocked_act), rescued))
        if not new:
            break
    depth = max([lv.level for lv in levels if lv.new] or [1])
    return Result(levels, sum(len(lv.new) for lv in levels), sum(lv.generated for lv in levels), sum(lv.blocked for lv in levels), depth,
                  sum(len(lv.rescued) for lv in levels), time.time() - t0)


def new_fps(lv):
    return np.array(sorted(lv.new), dtype=np.uint64)
