"""Deterministic guided harvest of reachable states deep in the view-change and state-transfer protocol (a helper module of
tests/test_deep_actions_cpu.py and tests/test_deep_actions_gpu.py, TEST INFRASTRUCTURE).

A plain BFS cannot reach these states at four or five replicas: on (5,1,1,1) level 12 already holds 5.1e6 states and the first state
with SendSV enabled is 15 steps from Init, the first with ReceiveSV 19.  So the walk is steered.  It uses the C++ CPU oracle only
(oracle/orc.py: successors, fingerprint); every state it returns is reached from Init by successor steps of that oracle, so every one
of them is a legitimate input of the model.

    restricted walk   level-synchronous; every successor is looked at, but only the successors of a chosen set of actions are
                      followed; de-duplicated by the oracle's fingerprint; successors that violate the invariant are dropped (their
                      parents are remembered: Harvest.violating_parents); a level larger than the beam is sorted by fingerprint and
                      thinned to an even stride - half of the beam is reserved for states whose replicas are in different views (what
                      ReceiveHigherDVC, VSR.tla:677-688, needs: a DoViewChange of a view above the receiver's).  No randomness: the same
                      states in every run.
    walk VC           follows the view-change actions (ids 1-8) from Init to exhaustion.
    walk ST           a VC walk in which "frozen" replicas are held back (a successor that changes the view number of a frozen replica is
                      discarded), so that a view change completes without them; from the states that then have a Normal replica in a
                      view above 1 and every frozen replica still in view 1, the actions 9-15 are followed with nobody frozen.
"""
import collections

import numpy as np

VC_ACTIONS = frozenset(range(1, 9))
ST_ACTIONS = frozenset(range(9, 16))
N_ACTIONS = 16

# the eight actions whose instances the tests count (ids in Next order, VSR.tla:896-913)
A_ReceiveHigherDVC, A_SendSV, A_ReceiveSV, A_ReceivePrepareOkMsg, A_ExecuteOp = 5, 7, 8, 11, 12
A_SendGetState, A_ReceiveGetState, A_ReceiveNewState = 13, 14, 15
COUNTED = (A_SendSV, A_ReceiveSV, A_ReceiveHigherDVC, A_ReceivePrepareOkMsg, A_ExecuteOp, A_SendGetState, A_ReceiveGetState,
           A_ReceiveNewState)


def views(P, rec):
    """view number of every replica of a wire record (A word of replica r: word 1 + (r - 1) * wpr, bits 2-4)"""
    w = P.wpr()
    return tuple((int(rec[1 + r * w]) >> 2) & 7 for r in range(P.R))


def statuses(P, rec):
    w = P.wpr()
    return tuple(int(rec[1 + r * w]) & 3 for r in range(P.R))


def bag_size(rec):
    return int(rec[0]) & 0xFF


class Harvest:
    """records: wire records (np.uint64 arrays) in ascending fingerprint order; fps: their fingerprints"""

    def __init__(self, orc, P, by_fp, violating_parents):
        self.orc, self.P = orc, P
        self.fps = sorted(by_fp)
        self.records = [by_fp[f] for f in self.fps]
        self.violating_parents = sorted(violating_parents)       # fingerprints of harvested states with a violating successor
        self._actions = {}

    def __len__(self):
        return len(self.records)

    def successors(self, i):
        """the oracle's successors of record i (not kept: 150 000 states' successor records are hundreds of MB)"""
        s = self.orc.successors(self.P, self.records[i])
        self._actions[i] = bytes(x["action"] for x in s)
        return s

    def actions(self, i):
        """action id of every successor of record i, in Next order (kept: one byte each)"""
        a = self._actions.get(i)
        if a is None:
            self.successors(i)
            a = self._actions[i]
        return a

    def enabled(self):
        """enabled instances per action id over all harvested states"""
        c = collections.Counter()
        for i in range(len(self)):
            c.update(self.actions(i))
        return c

    def summary(self):
        """what a drifting harvest would change: state count, xor of the fingerprints, largest bag"""
        x = 0
        for f in self.fps:
            x ^= f
        return dict(states=len(self), fp_xor=x, max_bag=max(bag_size(r) for r in self.records))

    def batch(self, lo, hi):
        """records lo .. hi - 1 as (words, offsets) of the C ABI"""
        recs = self.records[lo:hi]
        return np.concatenate(recs), np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64)


def _thin(P, level, beam):
    """level: {fp: record}; more than `beam` states -> an even stride of the fingerprint order, half of it among the states whose replicas
    are in different views (all of those when they are fewer)"""
    if len(level) <= beam:
        return level
    split = [f for f in sorted(level) if len(set(views(P, level[f]))) > 1]
    same = [f for f in sorted(level) if len(set(views(P, level[f]))) == 1]
    n_split = min(len(split), max(beam // 2, beam - len(same)))
    out = {}
    for fps, n in ((split, n_split), (same, beam - n_split)):
        for k in range(n):
            f = fps[(k * len(fps)) // n]
            out[f] = level[f]
    return out


def walk(orc, P, seeds, follow, beam, frozen=(), max_levels=64, seen=None, violating_parents=None):
    """the restricted walk -> {fp: record} of every state visited (the seeds included)"""
    seen = {} if seen is None else seen
    vp = set() if violating_parents is None else violating_parents
    level = {}
    for rec in seeds:
        fp = orc.fingerprint(P, rec)[0]
        if fp not in seen:
            seen[fp] = level[fp] = rec
    visited = dict(level)
    for _ in range(max_levels):
        if not level:
            break
        nxt = {}
        for fp in sorted(level):
            rec = level[fp]
            v0 = views(P, rec)
            for s in orc.successors(P, rec):
                if s["inv"]:
                    vp.add(fp)
                    continue
                if s["action"] not in follow or s["fp"] in seen or s["fp"] in nxt:
                    continue
                if frozen:
                    v1 = views(P, s["words"])
                    if any(v1[r - 1] != v0[r - 1] for r in frozen):
                        continue
                nxt[s["fp"]] = s["words"]
        level = _thin(P, nxt, beam)
        for fp, rec in level.items():
            seen[fp] = rec
        visited.update(level)
    return visited


def harvest_vc(orc, P, beam=1000, max_levels=64):
    vp = set()
    got = walk(orc, P, [orc.init_record(P)], VC_ACTIONS, beam, max_levels=max_levels, violating_parents=vp)
    return Harvest(orc, P, got, vp & set(got))


NORMAL_ACTIONS = frozenset((9, 10, 11, 12))


def harvest_st(orc, P, frozen, beam=1000, seed_cap=400, max_levels=64, prefix_levels=0):
    """-> Harvest of the second phase (the seeds included).  prefix_levels > 0: the view change starts not only from Init but from every state
    of that many levels of normal operation in view 1 (actions 9-12), so that the logs the view change merges are not all empty."""
    vp = set()
    start = [orc.init_record(P)]
    if prefix_levels:
        pre = walk(orc, P, start, NORMAL_ACTIONS, beam, max_levels=prefix_levels)
        start = [pre[f] for f in sorted(pre)]
    first = walk(orc, P, start, VC_ACTIONS, beam, frozen=frozen, max_levels=max_levels)
    seeds = []
    for fp in sorted(first):
        rec = first[fp]
        v, st = views(P, rec), statuses(P, rec)
        if all(v[r - 1] == 1 for r in frozen) and any(v[r] > 1 and st[r] == 0 for r in range(P.R)):
            seeds.append(rec)
    if len(seeds) > seed_cap:
        seeds = [seeds[(k * len(seeds)) // seed_cap] for k in range(seed_cap)]
    got = walk(orc, P, seeds, ST_ACTIONS, beam, max_levels=max_levels, violating_parents=vp)
    return Harvest(orc, P, got, vp & set(got))


# the spaces of the tests: (R, C, n, L) -> the walks whose union is harvested.  (5,1,2,1) runs k_expand's whole family of instantiations (SPEC 512),
# (4,1,2,1) a fused one (SPEC 412), the two L = 2 spaces the generic ones.
SPACES = {
    (5, 1, 2, 1): (("st", dict(prefix_levels=4)), ("vc", {})),
    (4, 1, 2, 1): (("st", dict(prefix_levels=4)), ("vc", {})),
    (5, 1, 1, 2): (("vc", {}),),
    (4, 1, 1, 2): (("vc", {}),),
}
FLOOR = {5: 1000, 4: 200}                                           # directly compared instances per counted action, per replica count
# the counted actions every space must itself contribute to (the floors are per replica count, over its two spaces).  The two spaces of ONE
# value cannot contribute the other five: ReceivePrepareOkMsg and ExecuteOp need an operation in a log, which these view-change walks never
# put there, and SendGetState needs m.op_number > op + 1 (VSR.tla:503), i.e. two operations - with one value there is at most one.
EXPECTED = {
    (5, 1, 2, 1): COUNTED,
    (4, 1, 2, 1): tuple(a for a in COUNTED if a != A_ReceiveHigherDVC),   # (one timer, L = 1: only 51 harvested states receive a DVC of a higher view)
    (5, 1, 1, 2): (A_SendSV, A_ReceiveSV, A_ReceiveHigherDVC),
    (4, 1, 1, 2): (A_SendSV, A_ReceiveSV, A_ReceiveHigherDVC),
}

# the TWO-CLIENT spaces (tests/test_two_clients_cpu.py, test_two_clients_gpu.py): three replicas, run under the documented policy assume_commit_number (the
# strict reading of VSR.tla:421 aborts on the first ReceivePrepareMsg at ClientCount = 2).  (3,2,3,1) and (3,2,3,2) are SPEC 323 - BASELINE configs[3]'s
# instantiation of k_expand - and (3,2,2,1) a generic one.  Five levels of normal operation before the view change put entries of both clients into the logs
# the view change merges.
A_ReceivePrepareMsg = 10
COUNTED_C2 = COUNTED + (A_ReceivePrepareMsg,)
SPACES_C2 = {
    (3, 2, 3, 1): (("st", dict(prefix_levels=5)), ("vc", {})),
    (3, 2, 3, 2): (("st", dict(prefix_levels=5)), ("vc", {})),
    (3, 2, 2, 1): (("st", dict(prefix_levels=5)), ("vc", {})),
}
FLOOR_C2 = 500                                                      # directly compared instances per action of COUNTED_C2, over the three spaces together
FLOOR_C2_FLIPS = 800                                                # (3,2,3,1): ReceivePrepareMsg flips the executed bit of a row it did not write, per client
FLOOR_C2_EXPAND = {a: 1000 for a in COUNTED_C2 if a not in (A_SendSV, A_ReceiveHigherDVC)}     # act_generated of the seeded level of (3,2,3,1) ...
FLOOR_C2_EXPAND[A_SendSV] = 150                                     # ... (ReceiveHigherDVC is not floored there: 5 instances at L = 1)
_cache = {}


def walks_of(key):
    return SPACES[key] if key in SPACES else SPACES_C2[key]


def expected(key):
    """the counted actions the space `key` must itself contribute to"""
    return EXPECTED[key] if key in EXPECTED else COUNTED_C2


def policy(key):
    """keyword arguments of the policy a space runs under, the same for orc.Params, pyoracle.Model and Model.from_constants"""
    return dict(assume_commit_number=True) if key in SPACES_C2 else {}


def params(orc, key, **kw):
    return orc.Params(*key, **dict(policy(key), **kw))


def py_model(key, **kw):
    from oracle import pyoracle as po
    return po.Model(key[0], key[1], tuple("v%d" % (i + 1) for i in range(key[2])), key[3], **dict(policy(key), **kw))


def product_model(vt, key, **kw):
    return vt.Model.from_constants(R=key[0], C_=key[1], n=key[2], L=key[3], **dict(policy(key), **kw))


def get(orc, key, kind, **kw):
    """one walk of the space `key` = (R, C, n, L), kind "vc" or "st" (frozen = the last two replicas at R = 5, the last one at R = 4 and R = 3); cached
    per process"""
    k = (key, kind, tuple(sorted(kw.items())), orc.fp_seed())
    if k not in _cache:
        P = params(orc, key)
        if kind == "vc":
            _cache[k] = harvest_vc(orc, P, **kw)
        else:
            _cache[k] = harvest_st(orc, P, frozen=(4, 5) if key[0] == 5 else (key[0],), **kw)
    return _cache[k]


def space(orc, key):
    """the harvest of one space of SPACES or SPACES_C2: the union of its walks (one state per fingerprint); cached per process"""
    k = (key, "space", orc.fp_seed())
    if k not in _cache:
        by_fp, vp = {}, set()
        for kind, kw in walks_of(key):
            h = get(orc, key, kind, **kw)
            by_fp.update(zip(h.fps, h.records))
            vp.update(h.violating_parents)
        _cache[k] = Harvest(orc, params(orc, key), by_fp, vp)
    return _cache[k]


def c2_facts(orc, key):
    """what makes a two-client harvest a test of the ClientCount = 2 code, from the oracle's successors unpacked by oracle/pycodec.py alone (cached per
    process).  A ReceivePrepareMsg instance "flips client c" when the executed bit of row c of the receiving replica's client table changes although the
    appended entry is the OTHER client's: the row the else branch of VSR.tla:414-421 recomputes.
      flip_states[c]    indices of the states with such an instance        flips[c]      such instances
      both_rows         ReceivePrepareMsg instances that change both rows   exec_rows[c]  ExecuteOp instances that change row c"""
    k = (key, "c2_facts", orc.fp_seed())
    if k in _cache:
        return _cache[k]
    from oracle import pycodec
    h, PM = space(orc, key), py_model(key)
    assert key[1] == 2
    out = dict(flip_states={1: [], 2: []}, flips={1: 0, 2: 0}, both_rows=0, exec_rows={1: 0, 2: 0})
    for i in range(len(h)):
        acts = h.actions(i)
        if A_ReceivePrepareMsg not in acts and A_ExecuteOp not in acts:
            continue
        p = pycodec.unpack(PM, [int(x) for x in h.records[i]])
        flipped = set()
        for s in h.successors(i):
            if s["action"] not in (A_ReceivePrepareMsg, A_ExecuteOp):
                continue
            c = pycodec.unpack(PM, [int(x) for x in s["words"]])
            changed = [(r, cl) for r in range(key[0]) for cl in (1, 2) if p["rep_client_table"][r][cl - 1] != c["rep_client_table"][r][cl - 1]]
            if s["action"] == A_ExecuteOp:
                for _r, cl in changed:
                    out["exec_rows"][cl] += 1
                continue
            (r,) = [r for r in range(key[0]) if len(c["rep_log"][r]) == len(p["rep_log"][r]) + 1]
            other = 3 - dict(c["rep_log"][r][-1])["client_id"]
            if len(changed) == 2:
                out["both_rows"] += 1
            if dict(p["rep_client_table"][r][other - 1])["executed"] != dict(c["rep_client_table"][r][other - 1])["executed"]:
                out["flips"][other] += 1
                flipped.add(other)
        for cl in flipped:
            out["flip_states"][cl].append(i)
    _cache[k] = out
    return out


def c2_state_facts(orc, key):
    """-> (states with a log that holds entries of both clients, states in which replica 1 holds a request, request_number > 0, of both clients)"""
    from oracle import pycodec
    h, PM = space(orc, key), py_model(key)
    both_logs = both_requests = 0
    for rec in h.records:
        p = pycodec.unpack(PM, [int(x) for x in rec])
        both_logs += any(len(set(dict(e)["client_id"] for e in lg)) == 2 for lg in p["rep_log"])
        both_requests += all(dict(row)["request_number"] > 0 for row in p["rep_client_table"][0])
    return both_logs, both_requests


C2_PY_SAMPLE = 60


def _stride(idx, k):
    k = min(k, len(idx))
    return [idx[(j * len(idx)) // k] for j in range(k)]


def c2_py_sample(orc, key):
    """indices of the states on which the Python restatement is compared: an even stride of 60 of the states that enable each counted action, and of the
    states in which ReceivePrepareMsg flips a row of client 1 / of client 2 -> (sorted indices, {action or ("flip", client): states taken})"""
    h, facts = space(orc, key), c2_facts(orc, key)
    states_of = collections.defaultdict(list)
    for i in range(len(h)):
        for a in set(h.actions(i)):
            if a in COUNTED_C2:
                states_of[a].append(i)
    for cl in (1, 2):
        states_of[("flip", cl)] = facts["flip_states"][cl]
    sample, taken = set(), {}
    for what, idx in states_of.items():
        mine = _stride(idx, C2_PY_SAMPLE)
        taken[what] = len(mine)
        sample.update(mine)
    return sorted(sample), taken


def max_bag_of_layout(P):
    """bag capacity of the device layout at R >= 4 (csrc/host_model.hpp: build_model): 95 words per staged record less the fixed ones (header,
    replica blocks, one view hash per value permutation)"""
    perms = 1
    for k in range(2, P.n + 1):
        perms *= k
    return 95 - (P.fixed_words() + perms)


# ---------------------------------------------------------------------------------------------------------------------
# hand-built records: HighestLog at f + 1 = 3 (VSR.tla:716-722), HighestCommitNumber (:729-733), state transfer with lagging replicas
# ---------------------------------------------------------------------------------------------------------------------
def hand_built(R):
    """-> (python states of (R,1,{v1,v2},1), checks): checks = [(state number, function(successor list [(action name, python state)]) asserting by
    value)]"""
    from oracle import pyoracle as po
    PM = po.Model(R, 1, ("v1", "v2"), 1)
    e = lambda view, v, req: po.rec(view_number=view, operation=v, client_id=1, request_number=req)   # noqa: E731
    e1, e2a, e2b, e3 = e(1, "v1", 1), e(2, "v2", 2), e(1, "v2", 2), e(2, "v1", 3)
    acked = {"v1": True, "v2": False}
    states, checks = [], []
    NEW, PRIM = 3, 3                                                  # the view being started and its primary (Primary(3) = 3 at R = 4 and R = 5)

    def dvc(source, lnv, log, commit):
        return po.rec(type=po.DoViewChangeMsg, view_number=NEW, log=tuple(log), last_normal_vn=lnv, op_number=len(log), commit_number=commit,
                      dest=PRIM, source=source)

    def view_change(dvcs, own_log=(), own_commit=0):
        """every replica in view NEW; the primary in ViewChange with `dvcs` received, its own log as given"""
        s = po.Init(PM)
        logs = [()] * R
        logs[PRIM - 1] = tuple(own_log)
        s = po.upd(s, rep_view_number=(NEW,) * R, rep_last_normal_view=(2,) * R, aux_svc=NEW - 1,
                   rep_status=tuple(po.ViewChange for _ in range(R)), rep_sent_dvc=(True,) * R,
                   rep_log=tuple(logs), rep_op_number=tuple(len(l) for l in logs),
                   rep_commit_number=tuple(own_commit if r == PRIM - 1 else 0 for r in range(R)),
                   rep_dvc_recv=tuple(frozenset(dvcs) if r == PRIM - 1 else frozenset() for r in range(R)), aux_client_acked=dict(acked))
        states.append(s)
        return len(states) - 1

    def installs(k, log, commit):
        def chk(succ):
            sv = [t for a, t in succ if a == "SendSV"]
            assert len(sv) == 1, (k, [a for a, _ in succ])
            t = sv[0]
            assert t["rep_log"][PRIM - 1] == tuple(log) and t["rep_op_number"][PRIM - 1] == len(log), (k, t["rep_log"][PRIM - 1])
            assert t["rep_commit_number"][PRIM - 1] == commit and t["rep_status"][PRIM - 1] == po.Normal, k
            assert t["rep_last_normal_view"][PRIM - 1] == NEW and t["rep_sent_sv"][PRIM - 1] is True
            svs = [m for m in t["messages"] if dict(m)["type"] == po.StartViewMsg]
            assert len(svs) == R - 1 and all(dict(m)["log"] == tuple(log) and dict(m)["commit_number"] == commit for m in svs), k
        checks.append((k, chk))

    # (a) three DVCs tie on (last_normal_vn, op_number) and differ in log, source and commit number: the CHOOSE of VSR.tla:716-722 takes the first of
    #     them in TLC's order of the records - the smallest commit number - whatever the source order is; HighestCommitNumber (:729-733) is the largest
    installs(view_change([dvc(1, 2, [e1, e2a], 1), dvc(2, 2, [e1, e2a], 2), dvc(4, 2, [e1, e2b], 0)]), [e1, e2b], 2)
    installs(view_change([dvc(1, 2, [e1, e2b], 0), dvc(2, 2, [e1, e2a], 2), dvc(4, 2, [e1, e2a], 1)]), [e1, e2b], 2)
    # (b) the same three with equal commit numbers: the smallest source decides
    installs(view_change([dvc(1, 2, [e1, e2a], 1), dvc(2, 2, [e1, e2b], 1), dvc(4, 2, [e1, e2b], 1)]), [e1, e2a], 1)
    installs(view_change([dvc(1, 2, [e1, e2b], 1), dvc(2, 2, [e1, e2a], 1), dvc(4, 2, [e1, e2a], 1)]), [e1, e2b], 1)
    # (c) the highest last_normal_vn has the SHORTER log: it wins over longer logs of an older view (:718-721)
    installs(view_change([dvc(1, 1, [e1, e2b, e3], 1), dvc(2, 2, [e1], 1), dvc(4, 1, [e1, e2b], 0)]), [e1], 1)
    installs(view_change([dvc(1, 1, [e1, e2b], 0), dvc(2, 1, [e1, e2b, e3], 1), dvc(4, 2, [], 0)]), [], 1)
    # (d) equal last_normal_vn: the longest log, wherever it sits; the commit number comes from another record
    installs(view_change([dvc(1, 2, [e1], 1), dvc(2, 2, [e1, e2a], 0), dvc(4, 2, [e1, e2a, e3], 0)]), [e1, e2a, e3], 1)
    installs(view_change([dvc(1, 2, [e1, e2a, e3], 0), dvc(2, 2, [e1], 0), dvc(4, 2, [e1, e2a], 2)]), [e1, e2a, e3], 2)
    # (e) more than a quorum, the primary's own record among them
    installs(view_change([dvc(1, 2, [e1], 1), dvc(2, 2, [e1, e2a], 1), dvc(3, 2, [e1, e2b], 0), dvc(4, 2, [e1, e2a], 2)], own_log=[e1, e2b]),
             [e1, e2b], 2)
    if R == 5:
        installs(view_change([dvc(1, 1, [e1, e2b, e3], 2), dvc(2, 2, [e1, e2a], 0), dvc(4, 2, [e1], 1), dvc(5, 2, [e1, e2b], 1)]), [e1, e2a], 2)
    # (f) one short of the quorum f + 1 = 3: SendSV is not enabled
    k = view_change([dvc(1, 2, [e1], 1), dvc(4, 2, [e1, e2a], 1)])

    def no_sv(succ, k=k):
        assert [a for a, _ in succ].count("SendSV") == 0, (k, "SendSV below the quorum")
    checks.append((k, no_sv))

    # ---- state transfer with lagging replicas (VSR.tla:496-516): the replicas from 4 on are still Normal in view 1, the primary of view 2
    #      (replica 2) has sent them a Prepare for op 3
    def prepare(dest):
        return po.rec(type=po.PrepareMsg, view_number=2, message=e3, op_number=3, commit_number=1, dest=dest, source=2)

    def getstate(dest, source, op):
        return po.rec(type=po.GetStateMsg, view_number=2, op_number=op, dest=dest, source=source)

    def lagging(extra, log, commit):
        lag = list(range(4, R + 1))
        s = po.Init(PM)
        s = po.upd(s, rep_view_number=tuple(1 if r + 1 in lag else 2 for r in range(R)),
                   rep_last_normal_view=tuple(1 if r + 1 in lag else 2 for r in range(R)), aux_svc=1,
                   rep_log=tuple(tuple(log) if r + 1 in lag else (e1, e2b, e3) for r in range(R)),
                   rep_op_number=tuple(len(log) if r + 1 in lag else 3 for r in range(R)),
                   rep_commit_number=tuple(commit if r + 1 in lag else 1 for r in range(R)),
                   messages=dict([(prepare(d), 1) for d in lag] + list(extra)), aux_client_acked=dict(acked))
        states.append(s)
        return len(states) - 1, len(lag)

    def sends(k, n, cut=None):
        def chk(succ):
            got = [t for a, t in succ if a == "SendGetState"]
            assert len(got) == n, (k, len(got), n)
            if cut is not None:                                       # MinVal, VSR.tla:504-507: the log is cut back to the commit number
                r = R - 1
                mine = [t for t in got if t["rep_view_number"][r] == 2]
                assert mine and all(t["rep_log"][r] == tuple(cut) and t["rep_op_number"][r] == len(cut) for t in mine), k
        checks.append((k, chk))

    k, nl = lagging([], [e1], 1)
    sends(k, nl * (R - 1), cut=[e1])                                  # every lagging replica may ask every other replica
    k, nl = lagging([], [e1], 0)
    sends(k, nl * (R - 1), cut=[])
    k, nl = lagging([(getstate(1, R, 1), 0)], [e1], 1)                # SendOnce (:250-252): the key towards replica 1 exists with count 0
    sends(k, nl * (R - 1) - 1)
    k, nl = lagging([(getstate(d, R, 1), 0) for d in range(1, R)], [e1], 1)    # every key of replica R exists: only the other lagging replicas send
    sends(k, (nl - 1) * (R - 1))
    k, nl = lagging([(getstate(1, R, 0), 0)], [e1], 1)                # a key for another op number does not block
    sends(k, nl * (R - 1))
    return states, checks
