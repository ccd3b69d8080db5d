"""Reference evaluation for the state-predicate tests of the two analysis models (test_where_models_cpu.py, test_where_models_gpu.py): every
predicate's TEXT beside a hand-written Python function over `pyoracle2.unpack(...)` / `pyoracle3.unpack(...)` of a record.  The reference is never
the parser: nothing here reads the text.

Conventions of the language the functions restate (csrc/vsr_where_parse.hpp): an entry is its operation; an absent entry (outside a log's domain, m.message
of anything but a PrepareMsg) is None here and equals only another absent entry, its operation equals Nil; an absent message field reads 0; a replica index
out of range yields -1 (FALSE for a boolean, the absent entry for a log); AnyDest is the integer 7; Len(m.log) is the number of entries the message carries."""
import random

from oracle import pyoracle2 as p2

ANYDEST = 7
MODELS = ("second", "third")


def msgs(s):
    return [(dict(m), c) for m, c in s["messages"].items()]


def R_(s):
    return len(s["rep_status"])


def reps(s):
    return range(1, R_(s) + 1)


def ok(s, r):
    return isinstance(r, int) and 1 <= r <= R_(s)


def op_of(e):
    return dict(e)["operation"]


def mf(m, f):
    """integer field of a message; absent = 0, AnyDest = 7"""
    v = m.get(f, 0)
    return ANYDEST if v == p2.AnyDest else v


def mlog(m):
    """m.log as {position: operation}: a sequence for DoViewChangeMsg / StartViewMsg, the function on first_op..op_number for a NewStateMsg, else empty"""
    if m["type"] in (p2.DoViewChangeMsg, p2.StartViewMsg):
        return {i + 1: op_of(e) for i, e in enumerate(m["log"])}
    if m["type"] == p2.NewStateMsg:
        return {on: op_of(e) for on, e in m["log"]}
    return {}


def mmsg(m):
    return op_of(m["message"]) if m["type"] == p2.PrepareMsg else None


def rlog(s, r):
    return {i + 1: op_of(e) for i, e in enumerate(s["rep_log"][r - 1])} if ok(s, r) else {}


def rapp(s, r):
    return {i + 1: op_of(e) for i, e in enumerate(s["rep_app_state"][r - 1])} if ok(s, r) else {}


def held(s, r):
    """rep_recv_dvc[r] as dicts, by source"""
    return sorted((dict(d) for d in s["rep_recv_dvc"][r - 1]), key=lambda d: d["source"]) if ok(s, r) else []


def dlog(d):
    return {i + 1: op_of(e) for i, e in enumerate(d["log"])}


def rint(s, name, r):
    return s[name][r - 1] if ok(s, r) else -1


# ---- the ten predicates of the issue ---------------------------------------------------------------------------------------------------------
def in_state_transfer(s):
    return any(st == p2.StateTransfer for st in s["rep_status"])


def get_state_to_any(s):
    return any(m["type"] == p2.GetStateMsg and m["dest"] == p2.AnyDest and c >= 1 for m, c in msgs(s))


def dvc_log_below_commit(s):
    return any(m["type"] == p2.DoViewChangeMsg and any(cn > len(mlog(m)) for cn in s["rep_commit_number"]) for m, _ in msgs(s))


def sv_log_drops_entry(s):
    return any(m["type"] == p2.StartViewMsg and m["dest"] != p2.AnyDest and len(mlog(m)) < len(s["rep_log"][m["dest"] - 1]) for m, _ in msgs(s))


def log_divergence(s):
    for r1 in reps(s):
        for r2 in reps(s):
            a, b = rlog(s, r1), rlog(s, r2)
            if any(i in b and a[i] != b[i] for i in a):
                return True
    return False


def counted_dvc(s):
    return any(m["type"] == p2.DoViewChangeMsg and c == 0 for m, c in msgs(s))


def new_state_carries(v):
    return lambda s: any(m["type"] == p2.NewStateMsg and mlog(m).get(2) == v for m, _ in msgs(s))


def app_ahead_of_some_log(s):
    return any(len(a) > len(b) for a in s["rep_app_state"] for b in s["rep_log"])


def two_dvcs_held(s):
    return any(len(x) >= 2 for x in s["rep_recv_dvc"])


def held_dvc_shorter_log(s):
    return any(len(d["log"]) < len(s["rep_log"][r - 1]) for r in reps(s) for d in held(s, r))


LOG_DIVERGENCE = r"\E r1, r2 \in replicas : \E i \in DOMAIN rep_log[r1] : i \in DOMAIN rep_log[r2] /\ rep_log[r1][i] # rep_log[r2][i]"


def set_a(values):
    """the seven predicates both analysis models have; bit k = entry k.  `values`: the model's value names (the second is named in the last one)"""
    v2 = values[1] if len(values) > 1 else values[0]
    return [
        ("InStateTransfer", r"\E r \in replicas : rep_status[r] = StateTransfer", in_state_transfer),
        ("GetStateToAny", r"\E m \in DOMAIN messages : m.type = GetStateMsg /\ m.dest = AnyDest /\ messages[m] >= 1", get_state_to_any),
        ("DvcLogBelowCommit", r"\E m \in DOMAIN messages : m.type = DoViewChangeMsg /\ (\E r \in replicas : rep_commit_number[r] > Len(m.log))", dvc_log_below_commit),
        ("SvLogDropsEntry", r"\E m \in DOMAIN messages : m.type = StartViewMsg /\ m.dest # AnyDest /\ Len(m.log) < Len(rep_log[m.dest])", sv_log_drops_entry),
        ("LogDivergence", LOG_DIVERGENCE, log_divergence),
        ("CountedDvc", r"\E m \in DOMAIN messages : m.type = DoViewChangeMsg /\ messages[m] = 0", counted_dvc),
        ("NewStateCarriesV2", r"\E m \in DOMAIN messages : m.type = NewStateMsg /\ 2 \in DOMAIN m.log /\ m.log[2].operation = " + v2, new_state_carries(v2)),
    ]


# the three only VR_APP_STATE.tla has (a second compiled object there: seven and three are more than eight)
SET_A3 = [
    ("AppAheadOfSomeLog", r"\E r1, r2 \in replicas : Len(rep_app_state[r1]) > Len(rep_log[r2])", app_ahead_of_some_log),
    ("TwoDvcsHeld", r"\E r \in replicas : Cardinality(rep_recv_dvc[r]) >= 2", two_dvcs_held),
    ("HeldDvcShorterLog", r"\E r \in replicas : \E d \in rep_recv_dvc[r] : Len(d.log) < Len(rep_log[r])", held_dvc_shorter_log),
]


# ---- the remaining constructs -------------------------------------------------------------------------------------------------------------------
def no_progress_quiet(s):
    return s["no_progress_ctr"] == 0 and not any(s["no_progress"])


def peer_ahead(s):
    return any(s["rep_peer_op_number"][r - 1][p - 1] > s["rep_commit_number"][r - 1] for r in reps(s) for p in reps(s))


def aux_round(s):
    return s["aux_svc"] >= 1 and any(not a for a in s["aux_client_acked"].values())


def new_state_is_whole(s):
    return any(mf(m, "first_op") >= 1 and mf(m, "first_op") + len(mlog(m)) == mf(m, "op_number") + 1 for m, _ in msgs(s))


def dvc_behind(s):
    return any(m["type"] == p2.DoViewChangeMsg and mf(m, "last_normal_vn") < mf(m, "view_number") - 1 for m, _ in msgs(s))


def sv_log_is_senders(s):
    for m, _ in msgs(s):
        if m["type"] == p2.StartViewMsg and len(mlog(m)) >= 1:
            mine = rlog(s, m["source"])
            if all(mine.get(i) == v for i, v in mlog(m).items()):
                return True
    return False


def prepare_matches_log(s):
    for m, _ in msgs(s):
        if m["type"] == p2.PrepareMsg and mmsg(m) is not None and rlog(s, m["source"]).get(mf(m, "op_number")) == mmsg(m):
            return True
    return False


def any_dest_index(s):
    return any(rint(s, "rep_view_number", mf(m, "dest")) == -1 for m, _ in msgs(s))


SET_B = [
    ("NoProgressQuiet", r"no_progress_ctr = NoProgressChangeLimit /\ (\A r \in replicas : ~no_progress[r])", no_progress_quiet),
    ("PeerAhead", r"\E r, p \in replicas : rep_peer_op_number[r][p] > rep_commit_number[r]", peer_ahead),
    ("AuxRound", r"aux_svc >= 1 /\ (\E v \in Values : v \in DOMAIN aux_client_acked /\ ~aux_client_acked[v])", aux_round),
    ("NewStateIsWhole", r"\E m \in DOMAIN messages : m.first_op >= 1 /\ m.first_op + Len(m.log) = m.op_number + 1", new_state_is_whole),
    ("DvcBehind", r"\E m \in DOMAIN messages : m.type = DoViewChangeMsg /\ m.last_normal_vn < m.view_number - 1", dvc_behind),
    ("SvLogIsSenders", r"\E m \in DOMAIN messages : m.type = StartViewMsg /\ Len(m.log) >= 1 /\ (\A i \in DOMAIN m.log : m.log[i] = rep_log[m.source][i])", sv_log_is_senders),
    ("PrepareMatchesLog", r"\E m \in DOMAIN messages : m.type = PrepareMsg /\ m.message = rep_log[m.source][m.op_number] /\ m.message.operation # Nil", prepare_matches_log),
    ("AnyDestIndex", r"\E m \in DOMAIN messages : rep_view_number[m.dest] = 0 - 1", any_dest_index),
]


def app_is_log_prefix(s):
    return all(rapp(s, r)[i] == rlog(s, r).get(i) for r in reps(s) for i in rapp(s, r))


def app_differs(s):
    return any(rapp(s, r1)[i] != rapp(s, r2).get(i) for r1 in reps(s) for r2 in reps(s) for i in rapp(s, r1))


def held_dvc_fields(s):
    return any(d["type"] == p2.DoViewChangeMsg and d["dest"] == r and d["source"] != r and d["view_number"] == s["rep_view_number"][r - 1]
               for r in reps(s) for d in held(s, r))


def held_dvc_stale(s):
    return any(d["last_normal_vn"] < d["view_number"] - 1 or d["commit_number"] < d["op_number"] for r in reps(s) for d in held(s, r))


def held_dvc_log_differs(s):
    return any(v != rlog(s, r).get(i) for r in reps(s) for d in held(s, r) for i, v in dlog(d).items())


def held_own_dvc(s):
    return any(d["source"] == r and len(d["log"]) == d["op_number"] for r in reps(s) for d in held(s, r))


def app_behind_commit(s):
    return any(len(a) < cn for a in s["rep_app_state"] for cn in s["rep_commit_number"])


def svc_from_a_held_source(s):
    return any(m["type"] == p2.StartViewChangeMsg and any(d["source"] == m["source"] for d in held(s, mf(m, "dest"))) for m, _ in msgs(s))


SET_B3 = [
    ("AppIsLogPrefix", r"\A r \in replicas : \A i \in DOMAIN rep_app_state[r] : rep_app_state[r][i] = rep_log[r][i]", app_is_log_prefix),
    ("AppDiffers", r"\E r1, r2 \in replicas : \E i \in DOMAIN rep_app_state[r1] : rep_app_state[r1][i].operation # rep_app_state[r2][i].operation", app_differs),
    ("HeldDvcFields", r"\E r \in replicas : \E d \in rep_recv_dvc[r] : d.type = DoViewChangeMsg /\ d.dest = r /\ d.source # r /\ d.view_number = rep_view_number[r]",
     held_dvc_fields),
    ("HeldDvcStale", r"\E r \in replicas : \E d \in rep_recv_dvc[r] : d.last_normal_vn < d.view_number - 1 \/ d.commit_number < d.op_number", held_dvc_stale),
    ("HeldDvcLogDiffers", r"\E r \in replicas : \E d \in rep_recv_dvc[r] : \E i \in DOMAIN d.log : d.log[i] # rep_log[r][i]", held_dvc_log_differs),
    ("HeldOwnDvc", r"\E r \in replicas : \E d \in rep_recv_dvc[r] : d.source = r /\ Len(d.log) = d.op_number", held_own_dvc),
    ("AppBehindCommit", r"\E r1, r2 \in replicas : Len(rep_app_state[r1]) < rep_commit_number[r2]", app_behind_commit),
    ("SvcFromAHeldSource", r"\E m \in DOMAIN messages : m.type = StartViewChangeMsg /\ (\E d \in rep_recv_dvc[m.dest] : d.source = m.source)", svc_from_a_held_source),
]


def text_of(preds):
    return "\n".join("%s == %s" % (name, text) for name, text, _ in preds)


def bits_of(preds, s):
    return sum((1 << k) for k, (_, _, f) in enumerate(preds) if f(s))


# ---- random well-typed expressions: text and closure built together ----------------------------------------------------------------------------
STATUS = [p2.Normal, p2.ViewChange, p2.StateTransfer]
MTYPES = ["StartViewChangeMsg", "PrepareMsg", "PrepareOkMsg", "DoViewChangeMsg", "StartViewMsg", "GetStateMsg", "NewStateMsg"]
MFIELDS = ["view_number", "dest", "source", "op_number", "commit_number", "last_normal_vn", "first_op"]
CMP = {"=": lambda a, b: a == b, "#": lambda a, b: a != b, "<": lambda a, b: a < b, "<=": lambda a, b: a <= b, ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}


class Gen:
    """env: list of (name, kind) with kind 'r' (a replica number), 'i' (a position 1..3), 'm' (a message) or 'd' (a held DoViewChange, third model).  A
    closure takes (s, b) with b a dict name -> replica number / position / (message dict, count) / DoViewChange dict.  Atoms lean towards what varies
    in a small space (view numbers, statuses, message types, log lengths), so that most expressions are not constant there."""

    def __init__(self, seed, R, third, L):
        self.rnd = random.Random(seed)
        self.R = R
        self.L = L
        self.third = third
        self.n_var = 0

    def rep_index(self, env):
        cands = [(str(k), (lambda k: lambda s, b: k)(k)) for k in range(1, self.R + 1)]
        cands += [(n, (lambda n: lambda s, b: b[n])(n)) for n, k in env if k == "r"]
        for n, k in env:
            if k == "m":
                for f in ("dest", "source"):
                    cands.append(("%s.%s" % (n, f), (lambda n, f: lambda s, b: mf(b[n][0], f))(n, f)))
        return self.rnd.choice(cands[-6:] if len(cands) > 6 and self.rnd.random() < 0.7 else cands)

    def position(self, env):
        pos = [n for n, kk in env if kk == "i"]
        if pos and self.rnd.random() < 0.8:
            n = self.rnd.choice(pos)
            return n, (lambda s, b: b[n])
        c = self.rnd.randrange(1, 4)
        return str(c), (lambda s, b: c)

    def entry(self, env):
        """an entry: (text, closure -> operation or None)"""
        r = self.rnd
        it, itf = self.position(env)
        ms = [n for n, kk in env if kk == "m"]
        ds = [n for n, kk in env if kk == "d"]
        k = r.randrange(5)
        if k == 0 and ms:
            n = r.choice(ms)
            return "%s.message" % n, lambda s, b: mmsg(b[n][0])
        if k == 1 and ms:
            n = r.choice(ms)
            return "%s.log[%s]" % (n, it), lambda s, b: mlog(b[n][0]).get(itf(s, b))
        if k == 2 and ds:
            n = r.choice(ds)
            return "%s.log[%s]" % (n, it), lambda s, b: dlog(b[n]).get(itf(s, b))
        t, f = self.rep_index(env)
        if k == 3 and self.third:
            return "rep_app_state[%s][%s]" % (t, it), lambda s, b: rapp(s, f(s, b)).get(itf(s, b))
        return "rep_log[%s][%s]" % (t, it), lambda s, b: rlog(s, f(s, b)).get(itf(s, b))

    def integer(self, env, depth):
        r = self.rnd
        k = r.randrange(9 if depth > 0 else 7)
        if k == 0:
            v = r.randrange(0, 4)
            return str(v), lambda s, b: v
        if k == 1:
            t, f = self.rep_index(env)
            name = r.choice(["rep_view_number", "rep_op_number", "rep_commit_number", "rep_last_normal_view"])
            return "%s[%s]" % (name, t), lambda s, b: rint(s, name, f(s, b))
        if k == 2:
            t, f = self.rep_index(env)
            if self.third and r.random() < 0.4:
                if r.random() < 0.5:
                    return "Len(rep_app_state[%s])" % t, lambda s, b: len(rapp(s, f(s, b))) if ok(s, f(s, b)) else -1
                return "Cardinality(rep_recv_dvc[%s])" % t, lambda s, b: len(held(s, f(s, b))) if ok(s, f(s, b)) else -1
            return "Len(rep_log[%s])" % t, lambda s, b: len(rlog(s, f(s, b))) if ok(s, f(s, b)) else -1
        if k in (3, 4):
            ms = [n for n, kk in env if kk == "m"]
            ds = [n for n, kk in env if kk == "d"]
            if ds and r.random() < 0.5:
                n = r.choice(ds)
                fld = r.choice(["view_number", "dest", "source", "op_number", "commit_number", "last_normal_vn", "len"])
                if fld == "len":
                    return "Len(%s.log)" % n, lambda s, b: len(b[n]["log"])
                return "%s.%s" % (n, fld), lambda s, b: b[n][fld]
            if ms:
                n = r.choice(ms)
                fld = r.choice(MFIELDS + ["count", "len"])
                if fld == "count":
                    return "messages[%s]" % n, lambda s, b: b[n][1]
                if fld == "len":
                    return "Len(%s.log)" % n, lambda s, b: len(mlog(b[n][0]))
                return "%s.%s" % (n, fld), lambda s, b: mf(b[n][0], fld)
            return r.choice([("aux_svc", lambda s, b: s["aux_svc"]), ("no_progress_ctr", lambda s, b: s["no_progress_ctr"])])
        if k == 5:
            t1, f1 = self.rep_index(env)
            t2, f2 = self.rep_index(env)
            return ("rep_peer_op_number[%s][%s]" % (t1, t2),
                    lambda s, b: s["rep_peer_op_number"][f1(s, b) - 1][f2(s, b) - 1] if ok(s, f1(s, b)) and ok(s, f2(s, b)) else -1)
        if k == 6:
            return r.choice([("ReplicaCount", lambda s, b: R_(s)), ("AnyDest", lambda s, b: ANYDEST), ("StartViewOnTimerLimit", lambda s, b: self.L)])
        ta, fa = self.integer(env, depth - 1)
        tb, fb = self.integer(env, depth - 1)
        if k == 7:
            return "(%s + %s)" % (ta, tb), lambda s, b: fa(s, b) + fb(s, b)
        return "(%s - %s)" % (ta, tb), lambda s, b: fa(s, b) - fb(s, b)

    def boolean(self, env, depth):
        r = self.rnd
        k = r.randrange(11) if depth > 0 else r.randrange(4)
        if k == 0:
            op = r.choice(sorted(CMP))
            ta, fa = self.integer(env, 1)
            tb, fb = self.integer(env, 1)
            return "(%s %s %s)" % (ta, op, tb), lambda s, b: CMP[op](fa(s, b), fb(s, b))
        if k == 1:
            t, f = self.rep_index(env)
            st = r.choice(STATUS)
            return "(rep_status[%s] = %s)" % (t, st), lambda s, b: ok(s, f(s, b)) and s["rep_status"][f(s, b) - 1] == st
        if k == 2:
            ms = [n for n, kk in env if kk == "m"]
            if ms:
                n = r.choice(ms)
                ty = r.choice(MTYPES)
                return "(%s.type = %s)" % (n, ty), lambda s, b: b[n][0]["type"] == ty
            t, f = self.rep_index(env)
            name = r.choice(["rep_sent_dvc", "rep_sent_sv", "no_progress"])
            return "%s[%s]" % (name, t), lambda s, b: ok(s, f(s, b)) and bool(s[name][f(s, b) - 1])
        if k == 3:
            op = r.choice(["=", "#"])
            ta, fa = self.entry(env)
            if r.random() < 0.3:
                return "(%s.operation %s Nil)" % (ta, op), lambda s, b: CMP[op](fa(s, b), None)
            tb, fb = self.entry(env)
            return "(%s %s %s)" % (ta, op, tb), lambda s, b: CMP[op](fa(s, b), fb(s, b))
        if k == 4:
            t, f = self.boolean(env, depth - 1)
            return "~%s" % t if t.startswith("(") else "~(%s)" % t, lambda s, b: not f(s, b)
        if k in (5, 6):
            op = r.choice(["/\\", "\\/", "=>", "<=>"])
            ta, fa = self.boolean(env, depth - 1)
            tb, fb = self.boolean(env, depth - 1)
            fn = {"/\\": lambda x, y: x and y, "\\/": lambda x, y: x or y, "=>": lambda x, y: (not x) or y, "<=>": lambda x, y: bool(x) == bool(y)}[op]
            return "(%s %s %s)" % (ta, op, tb), lambda s, b: fn(fa(s, b), fb(s, b))
        self.n_var += 1
        q = r.choice(["\\A", "\\E"])
        agg = all if q == "\\A" else any
        if k == 7:
            n = "r%d" % self.n_var
            t, f = self.boolean(env + [(n, "r")], depth - 1)
            return "(%s %s \\in replicas : %s)" % (q, n, t), lambda s, b: agg(f(s, dict(b, **{n: x})) for x in range(1, self.R + 1))
        if k == 8 and sum(1 for _, kk in env if kk == "m") < 2:
            n = "m%d" % self.n_var
            t, f = self.boolean(env + [(n, "m")], depth - 1)
            return "(%s %s \\in DOMAIN messages : %s)" % (q, n, t), lambda s, b: agg(f(s, dict(b, **{n: mc})) for mc in msgs(s))
        if k == 9 and self.third:
            n = "d%d" % self.n_var
            rt, rf = self.rep_index(env)
            t, f = self.boolean(env + [(n, "d")], depth - 1)
            return ("(%s %s \\in rep_recv_dvc[%s] : %s)" % (q, n, rt, t), lambda s, b: agg(f(s, dict(b, **{n: d})) for d in held(s, rf(s, b))))
        n = "i%d" % self.n_var
        ms = [x for x, kk in env if kk == "m"]
        if ms and r.random() < 0.5:
            mn = r.choice(ms)
            t, f = self.boolean(env + [(n, "i")], depth - 1)
            return ("(%s %s \\in DOMAIN %s.log : %s)" % (q, n, mn, t), lambda s, b: agg(f(s, dict(b, **{n: x})) for x in sorted(mlog(b[mn][0]))))
        rt, rf = self.rep_index(env)
        t, f = self.boolean(env + [(n, "i")], depth - 1)
        if self.third and r.random() < 0.3:
            return ("(%s %s \\in DOMAIN rep_app_state[%s] : %s)" % (q, n, rt, t), lambda s, b: agg(f(s, dict(b, **{n: x})) for x in sorted(rapp(s, rf(s, b)))))
        return ("(%s %s \\in DOMAIN rep_log[%s] : %s)" % (q, n, rt, t), lambda s, b: agg(f(s, dict(b, **{n: x})) for x in sorted(rlog(s, rf(s, b)))))


def random_predicates(seed, R, L, count, third, depth=4):
    """-> [(text, function of the unpacked state)]"""
    g = Gen(seed, R, third, L)
    out = []
    for _ in range(count):
        t, f = g.boolean([], depth)
        out.append((t, (lambda f: lambda s: bool(f(s, {})))(f)))
    return out
