"""Violating states for the invariant evaluators of the two analysis models (TEST INFRASTRUCTURE, NOT PRODUCT CODE).

The invariants of VR_STATE_TRANSFER and VR_APP_STATE hold in every reachable state, so no walk of a state space ever shows an
evaluator anything but "all clear".  This module makes the material on which they can be compared: reachable states of small spaces
(every state of the C++ oracle's BFS) with the replica variables edited at the level of the Python restatement's state
(pyoracle2 / pyoracle3: unpack -> edit -> pack), so that the codec keeps every record inside the representation:
op_number = Len(log), Len(app_state) = commit_number, values of the model only, every field within its bit width.  The bag and
rep_recv_dvc are never touched.  Deterministic: a fixed seed, no clock.

Classes (each aims at one edge of check_invariants_child / check_invariants):
  A  acked            aux_client_acked[v] = TRUE with v held by 0 .. R replicas (holders == 0, holders >= R/2 + 1)
  B  log divergence   two replicas with commit >= k whose logs differ at position k only, every k <= n and ordered pair (r1, r2);
                      near misses: one of the two commits at k - 1 (the bit stays clear: `expect`)
  C  app divergence   (third model) app states differ at k, every combination of the two log entries at k; the near misses of B
  D  commit > op      on one replica and no access outside a log (only where Len(log) = n: the quantifier stops at n)
  E  latent           a clean parent in which some enabled action makes the violation (found by the Python restatement's successors),
                      and its mirror: a violating replica that is in a view change or a state transfer, or about to start one
  F  out of the log   a committed position beyond Len(log): a single replica (only the pair r1 = r2 reads it), a pair, and for
                      the third model an app-state divergence at a position the first replica's log does not have
  N  naive            one replica's log, commit number (and app state), or one aux_client_acked entry, at random
"""
import collections
import functools
import itertools
import random

import numpy as np

from oracle import orc2, orc3, pyoracle2, pyoracle3

SEED = 1
MODELS = {2: (orc2, pyoracle2), 3: (orc3, pyoracle3)}
BITS = {2: (1, 2, 4, 8), 3: (1, 2, 4, 8, 16)}
CFG_MASK = {2: 14, 3: 30}
ALL_MASK = {2: 15, 3: 31}
NAMES = {1: "AcknowledgedWriteNotLost", 2: "AcknowledgedWritesExistOnMajority", 4: "NoLogDivergence",
         8: "CommitNumberNeverHigherThanOpNumber", 16: "NoAppStateDivergence"}
# label -> (R, Values, TimerLimit, levels of the BFS): the three-value space is the only one that uses log position 3 (bits 31-33),
# app-state position 3 (bits 38-39) and value index 2; depth 6 is what the Python restatement's BFS walks in about 10 s
SPACES = collections.OrderedDict([("r3v2", (3, ("a", "b"), 2, 7)), ("r2v2", (2, ("a", "b"), 2, 14)), ("r3v3", (3, ("a", "b", "c"), 3, 6))])
RAISES = "raises"

Mutant = collections.namedtuple("Mutant", "cls tag words expect")     # expect: {bit: verdict the parent must get}, from the construction


@functools.lru_cache(maxsize=None)
def base_records(model, space):
    """every state of the C++ oracle's BFS of the space, as packed records (tuples of ints), level by level"""
    orc, _po = MODELS[model]
    R, values, L, depth = SPACES[space]
    P = orc.Params(R, len(values), L)
    b = orc.Bfs(P)
    out = [tuple(int(x) for x in orc.init_record(P))]
    while b.info["depth"] < depth and b.step() > 0:
        words, off = b.frontier()
        out.extend(tuple(int(x) for x in words[int(off[i]): int(off[i + 1])]) for i in range(len(off) - 1))
    b.close()
    return out


# ---- the Python state ---------------------------------------------------------------------------------------------------------------
def logvals(po, s, r):
    return [po.get(e, "operation") for e in s["rep_log"][r - 1]]


def appvals(po, s, r):
    return [po.get(e, "operation") for e in s["rep_app_state"][r - 1]] if "rep_app_state" in s else None


def set_rep(po, M, s, r, log=None, commit=None, app=None):
    """replica r with this log (value names), commit number and app state; op_number follows the log, the app state is cut or
    filled (from the log, then with the first value) to the commit number"""
    log = logvals(po, s, r) if log is None else list(log)
    commit = s["rep_commit_number"][r - 1] if commit is None else commit
    kw = dict(rep_log=po.tset(s["rep_log"], r, tuple(po.rec(operation=v) for v in log)),
              rep_op_number=po.tset(s["rep_op_number"], r, len(log)),
              rep_commit_number=po.tset(s["rep_commit_number"], r, commit))
    if "rep_app_state" in s:
        app = list(appvals(po, s, r) if app is None else app)[:commit]
        while len(app) < commit:
            app.append(log[len(app)] if len(app) < len(log) else M.Values[0])
        kw["rep_app_state"] = po.tset(s["rep_app_state"], r, tuple(po.rec(operation=v) for v in app))
    return po.upd(s, **kw)


def set_acked(po, s, v, a):
    acked = dict(s["aux_client_acked"])
    acked[v] = a
    return po.upd(s, aux_client_acked=acked)


def encode(po, M, s):
    """-> the packed record; refuses what the layout cannot hold.  A primary whose log is full would append on a client request,
    which the record cannot hold: a state with a full log has every value requested already."""
    if any(len(l) == 3 for l in s["rep_log"]):
        for v in M.Values:
            if v not in s["aux_client_acked"]:
                s = set_acked(po, s, v, False)
    for i in range(M.R):
        assert 0 <= s["rep_commit_number"][i] <= 3 and len(s["rep_log"][i]) <= 3 and s["rep_op_number"][i] == len(s["rep_log"][i])
        assert all(po.get(e, "operation") in M.Values for e in s["rep_log"][i])
        if "rep_app_state" in s:
            assert len(s["rep_app_state"][i]) == s["rep_commit_number"][i]
            assert all(po.get(e, "operation") in M.Values for e in s["rep_app_state"][i])
    words = po.pack(M, s)
    assert po.pack(M, po.unpack(M, words)) == words and all(0 <= w < 1 << 64 for w in words)
    return tuple(words)


def other(M, v, step=1):
    return M.Values[(M.Values.index(v) + step) % len(M.Values)]


def grown(M, vals, k):
    """the log, continued to length >= k"""
    vals = list(vals)
    while len(vals) < k:
        vals.append(M.Values[len(vals) % len(M.Values)])
    return vals


# ---- the evaluators, bit by bit, from the Python restatement -----------------------------------------------------------------------
def py_bit(po, M, s, bit):
    """one invariant on a Python state: 0, the bit, or RAISES (an access outside a sequence: TLC's evaluation error)"""
    try:
        if bit == 1:                                                  # AcknowledgedWriteNotLost: not in the restatements' masks
            ok = all(a is False or any(po.ReplicaHasOp(s, r, v) for r in range(1, M.R + 1)) for v, a in s["aux_client_acked"].items())
        else:
            ok = getattr(po, NAMES[bit])(M, s)
    except IndexError:
        return RAISES
    return 0 if ok else bit


def py_verdicts(po, M, s, model):
    return {b: py_bit(po, M, s, b) for b in BITS[model]}


# ---- the classes ---------------------------------------------------------------------------------------------------------------------
def class_a(po, M, s, rng, model):
    for v in M.Values:
        for h in range(M.R + 1):
            holders = set(rng.sample(range(1, M.R + 1), h))
            t = s
            for r in range(1, M.R + 1):
                vals = logvals(po, t, r)
                if r in holders and v not in vals:
                    vals = vals + [v] if len(vals) < 3 else vals[:-1] + [v]
                if r not in holders and v in vals:
                    vals = [x for x in vals if x != v]
                t = set_rep(po, M, t, r, log=vals, commit=min(t["rep_commit_number"][r - 1], len(vals)))
            want = {1: 1, 2: 2} if h == 0 else {2: 2} if h < M.R // 2 + 1 else {}
            yield "v=%s holders=%d" % (v, h), set_acked(po, t, v, True), want


def _pair_frame(po, M, s, r1, r2, k, l1, l2, variant, app1=None, app2=None):
    """r1, r2 with these logs and commit k (near1 / near2: k - 1 on that one); every other replica at commit 0"""
    c1, c2 = (k - 1 if variant == "near1" else k), (k - 1 if variant == "near2" else k)
    t = set_rep(po, M, s, r1, log=l1, commit=c1, app=l1 if app1 is None else app1)
    t = set_rep(po, M, t, r2, log=l2, commit=c2, app=l1 if app2 is None else app2)
    for r in range(1, M.R + 1):
        if r not in (r1, r2):
            t = set_rep(po, M, t, r, commit=0)
    return t


def class_b(po, M, s, rng, model):
    n = len(M.Values)
    for k in range(1, n + 1):
        for r1, r2 in itertools.permutations(range(1, M.R + 1), 2):
            l1 = grown(M, logvals(po, s, r1), k)
            l2 = list(l1)
            l2[k - 1] = other(M, l1[k - 1], rng.randrange(1, n))
            for variant in ("both", "own", "near1", "near2"):
                # "both": the two app states agree (bit 16 clear); "own": each app state is the replica's own log (bit 16 too)
                t = _pair_frame(po, M, s, r1, r2, k, l1, l2, variant, app2=l2 if variant == "own" else None)
                want = {4: 0 if variant.startswith("near") else 4, 8: 0}
                if model == 3:
                    want[16] = 16 if variant == "own" else 0
                yield "k=%d r1=%d r2=%d %s" % (k, r1, r2, variant), t, want


def class_c(po, M, s, rng, model):
    n = len(M.Values)
    for k in range(1, n + 1):
        for r1, r2 in itertools.permutations(range(1, M.R + 1), 2):
            combos = [(g1, g2, a1, a2) for g1 in M.Values for g2 in M.Values for a1 in M.Values for a2 in M.Values if a1 != a2]
            if len(combos) > 8:
                combos = rng.sample(combos, 8)
            for g1, g2, a1, a2 in combos:                             # the entries at k: rep_log[r1], rep_log[r2], app[r1], app[r2]
                l1 = grown(M, logvals(po, s, r1), k)
                l1[k - 1] = g1
                l2 = list(l1)
                l2[k - 1] = g2
                ap1, ap2 = list(l1[:k]), list(l1[:k])
                ap1[k - 1], ap2[k - 1] = a1, a2
                for variant in ("both", "near1", "near2"):
                    t = _pair_frame(po, M, s, r1, r2, k, l1, l2, variant, app1=ap1, app2=ap2)
                    fires = variant == "both" and (g1 == a1 or g2 == a2)    # VRAS.tla:858 read from (r1, r2) and from (r2, r1)
                    yield "k=%d r1=%d r2=%d log=%s%s app=%s%s %s" % (k, r1, r2, g1, g2, a1, a2, variant), t, {16: 16 if fires else 0, 8: 0}


def class_d(po, M, s, rng, model):
    n = len(M.Values)
    if n + 1 > 3:
        return                                                        # commit > Len(log) = n needs commit 4: outside the field
    for r in range(1, M.R + 1):
        for low in (False, True):
            t = set_rep(po, M, s, r, log=grown(M, logvals(po, s, r), n)[:n], commit=n + 1)
            if low:
                for q in range(1, M.R + 1):
                    if q != r:
                        t = set_rep(po, M, t, q, commit=0)
            yield "r=%d%s" % (r, " others at 0" if low else ""), t, {8: 8}


def class_f(po, M, s, rng, model):
    n = len(M.Values)
    for r in range(1, M.R + 1):
        vals = logvals(po, s, r)
        for ln in range(0, min(n, len(vals) + 1)):
            for commit in range(ln + 1, 4):
                # a single replica: no other commit number reaches the missing position
                t = set_rep(po, M, s, r, log=vals[:ln], commit=commit)
                for q in range(1, M.R + 1):
                    if q != r:
                        t = set_rep(po, M, t, q, commit=min(t["rep_commit_number"][q - 1], ln))
                yield "single r=%d len=%d commit=%d" % (r, ln, commit), t, {8: 8}
                # a pair: a second replica that has the position and has committed it
                q = rng.choice([x for x in range(1, M.R + 1) if x != r])
                lq = grown(M, vals[:ln], ln + 1)
                t = set_rep(po, M, set_rep(po, M, s, r, log=vals[:ln], commit=commit), q, log=lq, commit=ln + 1)
                yield "pair r=%d q=%d len=%d commit=%d" % (r, q, ln, commit), t, {8: 8}
    if model == 3:                                                    # app states differ at k, rep_log[r1] ends before k
        for k in range(1, n + 1):
            for r1, r2 in itertools.permutations(range(1, M.R + 1), 2):
                l2 = grown(M, logvals(po, s, r2), k)
                ap1, ap2 = list(l2[:k]), list(l2[:k])
                ap1[k - 1] = other(M, ap2[k - 1], rng.randrange(1, n))
                t = set_rep(po, M, set_rep(po, M, s, r1, log=l2[:k - 1], commit=k, app=ap1), r2, log=l2, commit=k, app=ap2)
                yield "app k=%d r1=%d r2=%d" % (k, r1, r2), t, {8: 8}


def class_n(po, M, s, rng, model):
    if rng.random() < 0.25:
        v = rng.choice(M.Values)
        yield "acked %s" % v, set_acked(po, s, v, rng.choice((False, True))), {}
        return
    r = rng.randrange(1, M.R + 1)
    log = [rng.choice(M.Values) for _ in range(rng.randrange(0, 4))]
    commit = rng.randrange(0, 4)
    app = [rng.choice(M.Values) for _ in range(commit)]
    yield "r=%d log=%s commit=%d" % (r, "".join(log), commit), set_rep(po, M, s, r, log=log, commit=commit, app=app), {}


def unsettled(po, M, s):
    """replicas in a view change or a state transfer, or to which a StartView / NewState of the bag is addressed"""
    out = set(r for r in range(1, M.R + 1) if s["rep_status"][r - 1] != po.Normal)
    for m, c in s["messages"].items():
        if c > 0 and po.get(m, "type") in (po.StartViewMsg, po.NewStateMsg):
            out.update(r for r in range(1, M.R + 1) if po.get(m, "dest") in (r, po.Nil) and po.get(m, "source") != r)
    return sorted(out)


def class_e_candidates(po, M, s, rng, model, mirror=True):
    """edits that leave the state clean or nearly so, next to an action that may tip it; class_e keeps those that do"""
    n = len(M.Values)
    for r in range(1, M.R + 1):
        vals, commit = logvals(po, s, r), s["rep_commit_number"][r - 1]
        for p in range(commit + 1, len(vals) + 1):                    # diverged entries above the commit number
            w = list(vals)
            w[p - 1] = other(M, vals[p - 1], rng.randrange(1, n))
            yield "above commit r=%d p=%d" % (r, p), set_rep(po, M, s, r, log=w)
    for v, a in s["aux_client_acked"].items():                        # an acked value on a bare majority of logs
        holders = [r for r in range(1, M.R + 1) if v in logvals(po, s, r)]
        if len(holders) < M.R // 2 + 1:
            continue
        last = [r for r in holders if r in unsettled(po, M, s)] or holders
        for tag, keep in (("bare majority", set(rng.sample(holders, M.R // 2 + 1))), ("last holder", {rng.choice(last)})):
            t = s
            for r in holders:
                if r not in keep:
                    vals = [x for x in logvals(po, t, r) if x != v]
                    t = set_rep(po, M, t, r, log=vals, commit=min(t["rep_commit_number"][r - 1], len(vals)))
            yield "%s v=%s" % (tag, v), set_acked(po, t, v, True)
    for r in (unsettled(po, M, s) if mirror else ()):                 # the mirror: a violating replica about to be overwritten
        vals, commit = logvals(po, s, r), s["rep_commit_number"][r - 1]
        if len(vals) == n and n < 3:
            yield "unsettled commit>op r=%d" % r, set_rep(po, M, s, r, commit=n + 1)
        for v, a in s["aux_client_acked"].items():
            if v in vals:
                w = [x for x in vals if x != v]
                yield "unsettled loses %s r=%d" % (v, r), set_acked(po, set_rep(po, M, s, r, log=w, commit=min(commit, len(w))), v, True)
        for q in range(1, M.R + 1):
            k = s["rep_commit_number"][q - 1]
            if q != r and 1 <= k <= n:
                w = grown(M, vals, k)
                w[k - 1] = other(M, logvals(po, s, q)[k - 1], rng.randrange(1, n))
                yield "unsettled diverges r=%d q=%d k=%d" % (r, q, k), set_rep(po, M, s, r, log=w, commit=k, app=logvals(po, s, q)[:k])
                if model == 3:                                        # only (r, q) fires: rep_log[q][k] is not q's app state at k
                    aq = appvals(po, s, q)
                    x = other(M, aq[k - 1], rng.randrange(1, n))
                    w, wq = grown(M, vals, k), logvals(po, s, q)
                    w[k - 1] = wq[k - 1] = x
                    yield "unsettled app r=%d q=%d k=%d" % (r, q, k), set_rep(po, M, set_rep(po, M, s, q, log=wq), r, log=w, commit=k, app=aq[:k - 1] + [x])
        if len(vals) < 3:                                             # everything committed, and a shorter log on its way
            w = grown(M, vals, len(vals) + 1)
            yield "unsettled all committed r=%d" % r, set_rep(po, M, s, r, log=w, commit=len(w))


def class_e(po, M, s, rng, model, mirror=True):
    for tag, t in class_e_candidates(po, M, s, rng, model, mirror):
        before = py_verdicts(po, M, t, model)
        if RAISES in before.values() or (any(before.values()) and not mirror):
            continue
        try:
            children = [c for _a, c in po.successors(M, t)]
        except (po.EvalError, IndexError, ValueError, KeyError, AssertionError):
            continue
        moved = set()
        for c in children:
            after = py_verdicts(po, M, c, model)
            moved.update(("raised", b) for b in after if after[b] == b and before[b] == 0)
            moved.update(("cured", b) for b in after if after[b] == 0 and before[b] == b)
        if moved:
            yield "%s: %s" % (tag, ", ".join("%s %d" % x for x in sorted(moved))), t, dict(before)


CLASSES = collections.OrderedDict([("A", class_a), ("B", class_b), ("C", class_c), ("D", class_d), ("E", class_e), ("F", class_f), ("N", class_n)])
# base states taken per class and space (every class walks all its pairs / positions / values on each of them)
TAKE = {"A": 40, "B": 6, "C": 3, "D": 30, "E": 300, "F": 8, "N": 300}


@functools.lru_cache(maxsize=None)
def mutants(model, space):
    """-> list of Mutant for one model (2 | 3) and one space of SPACES, in a fixed order, every record distinct"""
    _orc, po = MODELS[model]
    R, values, L, _depth = SPACES[space]
    M = po.Model(R, values, L)
    base = base_records(model, space)
    out, seen = [], set(base)
    for cls, f in CLASSES.items():
        if cls == "C" and model != 3:
            continue
        rng = random.Random("%d %d %s %s" % (SEED, model, space, cls))
        picks = base if TAKE[cls] >= len(base) else rng.sample(base, TAKE[cls])
        for rec in picks:
            s = po.unpack(M, list(rec))
            for tag, t, expect in f(po, M, s, rng, model):
                words = encode(po, M, t)
                if words in seen:
                    continue
                seen.add(words)
                out.append(Mutant(cls, tag, np.array(words, dtype=np.uint64), expect))
    return out


@functools.lru_cache(maxsize=None)
def latent_parents(model, space, take):
    """the CLEAN parents of class E (no invariant violated, none raising) over `take` base states: seeds for a level of a checker"""
    _orc, po = MODELS[model]
    R, values, L, _depth = SPACES[space]
    M = po.Model(R, values, L)
    base = base_records(model, space)
    rng = random.Random("%d %d %s latent" % (SEED, model, space))
    out, seen = [], set(base)
    for rec in (base if take >= len(base) else rng.sample(base, take)):
        for tag, t, expect in class_e(po, M, po.unpack(M, list(rec)), rng, model, mirror=False):
            words = encode(po, M, t)
            if words not in seen and not any(expect.values()):
                seen.add(words)
                out.append(Mutant("E", tag, np.array(words, dtype=np.uint64), expect))
    return out


# ---- the C++ oracle's side: successors and verdicts, once per process ---------------------------------------------------------------
def oracle_params(model, space, mask):
    orc, _po = MODELS[model]
    R, values, L, _depth = SPACES[space]
    return orc.Params(R, len(values), L, invariant_mask=mask)


def orc_verdicts(model, space, words):
    """{bit: 0 | bit | RAISES}: every invariant alone (Params(invariant_mask = bit)), so that an evaluation error on one does not hide the others"""
    orc, _po = MODELS[model]
    out = {}
    for b in BITS[model]:
        try:
            out[b] = orc.invariants(oracle_params(model, space, b), words)
            assert out[b] in (0, b)
        except orc.OracleError:
            out[b] = RAISES
    return out


Family = collections.namedtuple("Family", "mutant verdicts children")   # children: the oracle's successors (mask 0), each with "verdicts"


@functools.lru_cache(maxsize=None)
def families(model, space):
    """-> ([Family], number of mutants the oracle refuses in `successors`: an action-level evaluation error on an unreachable state)"""
    orc, _po = MODELS[model]
    P0 = oracle_params(model, space, 0)
    out, refused = [], 0
    for m in mutants(model, space):
        try:
            succ = orc.successors(P0, m.words)
        except orc.OracleError:
            refused += 1
            continue
        for s in succ:
            s["verdicts"] = orc_verdicts(model, space, s["words"])
        out.append(Family(m, orc_verdicts(model, space, m.words), succ))
    return out, refused


def floors(model):
    """the counts of the issue's floors over all spaces, on the oracle's side -> dict"""
    c = dict(set=collections.Counter(), clear_beside=collections.Counter(), raised=collections.Counter(), cured=collections.Counter(),
             raises=collections.Counter(), parents=0, refused=0, children=0, by_class=collections.Counter())
    for space in SPACES:
        fams, refused = families(model, space)
        c["refused"] += refused
        c["parents"] += len(fams) + refused
        for f in fams:
            c["by_class"][f.mutant.cls] += 1
            for s in f.children:
                c["children"] += 1
                for b, v in s["verdicts"].items():
                    if v == b:
                        c["set"][b] += 1
                        if f.verdicts[b] == 0:
                            c["raised"][b] += 1
                    elif v == RAISES:
                        c["raises"][b] += 1
                    else:
                        if f.verdicts[b] == b:
                            c["cured"][b] += 1
                        if any(f.verdicts[o] == o for o in f.verdicts if o != b):
                            c["clear_beside"][b] += 1
    return c


def witnesses(po, M, s, bit):
    """the (r1, r2, k) at which NoLogDivergence (4) / NoAppStateDivergence (16) fails in a Python state: the ordered pairs and positions of
    VRST.tla:806-811, VRAS.tla:840-858 (an entry outside a log is no witness)"""
    out = set()
    for k in range(1, len(M.Values) + 1):
        for r1, r2 in itertools.permutations(range(1, M.R + 1), 2):
            if not (k <= s["rep_commit_number"][r1 - 1] and k <= s["rep_commit_number"][r2 - 1]):
                continue
            l1, l2 = s["rep_log"][r1 - 1], s["rep_log"][r2 - 1]
            if bit == 4 and len(l1) >= k and len(l2) >= k and l1[k - 1] != l2[k - 1]:
                out.add((r1, r2, k))
            if bit == 16 and len(l1) >= k and s["rep_app_state"][r1 - 1][k - 1] != s["rep_app_state"][r2 - 1][k - 1] \
                    and l1[k - 1] == s["rep_app_state"][r1 - 1][k - 1]:
                out.add((r1, r2, k))
    return out


# (model, bit, direction) the final generator never produces: no enabled action of these spaces empties the last log that holds an acked value
# without a majority having been lost before (bit 1 is raised by no step), and the second model's steps set the commit number only
# together with a log that reaches it (bit 8 is raised by no step of the second model)
NEVER = {(2, 1, "raised"), (3, 1, "raised"), (2, 8, "raised")}
FLOOR = 200
FLOOR_STEP = 5


def check_floors(model):
    """the floors, counted on the oracle's side and printed: per bit >= 200 children with the bit set and >= 200 with it clear beside another
    violated bit of the parent; >= 5 per (bit, raised / cured by the step) that occurs at all; every ordered pair and position k <= n among the
    violating children of classes B and C; <= 1 % of the parents refused by the oracle's `successors`"""
    _orc, po = MODELS[model]
    c = floors(model)
    print("model %d: %d parents (%s), %d refused by the oracle, %d children" % (model, c["parents"], dict(sorted(c["by_class"].items())), c["refused"], c["children"]))
    for b in BITS[model]:
        print("  bit %2d %-36s set %5d  clear beside another bit %5d  raises %5d  raised by the step %4d  cured by the step %4d"
              % (b, NAMES[b], c["set"][b], c["clear_beside"][b], c["raises"][b], c["raised"][b], c["cured"][b]))
    assert c["refused"] * 100 <= c["parents"]
    for b in BITS[model]:
        assert c["set"][b] >= FLOOR and c["clear_beside"][b] >= FLOOR, (model, b)
        for way in ("raised", "cured"):
            assert c[way][b] >= FLOOR_STEP or (c[way][b] == 0 and (model, b, way) in NEVER), (model, b, way, c[way][b])
    for space, (R, values, L, _depth) in SPACES.items():
        M = po.Model(R, values, L)
        seen = {4: set(), 16: set()}
        for f in families(model, space)[0]:
            if f.mutant.cls not in "BC":
                continue
            for s in f.children:
                for b in (4, 16):
                    if s["verdicts"].get(b) == b:
                        seen[b] |= witnesses(po, M, po.unpack(M, [int(x) for x in s["words"]]), b)
        want = set((r1, r2, k) for k in range(1, len(values) + 1) for r1, r2 in itertools.permutations(range(1, R + 1), 2))
        print("  %s: (r1, r2, k) among the violating children of classes B, C: bit 4 %d of %d%s" % (
            space, len(seen[4]), len(want), ", bit 16 %d of %d" % (len(seen[16]), len(want)) if model == 3 else ""))
        assert seen[4] == want and (model == 2 or seen[16] == want), (model, space)
    return c
