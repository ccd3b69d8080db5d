"""Reference evaluation for the state-predicate tests (test_where_cpu.py, test_where_gpu.py): every predicate's TEXT beside a hand-written Python
function over `pycodec.unpack(...)` of a record.  The reference is never the parser: nothing here reads the text.

Conventions of the language the functions restate (csrc/vsr_where_parse.hpp): an absent log entry or message field reads 0, m.message of anything
but a PrepareMsg is the absent entry, an absent entry's operation equals no value, aux_client_acked[v] outside its domain is FALSE, an index out
of range yields -1."""
import random

from oracle import pyoracle as po


def msgs(s):
    return [(dict(m), c) for m, c in s["messages"].items()]


def entries(s, r):
    """log of replica r (1-based) as dicts"""
    return [dict(e) for e in s["rep_log"][r - 1]]


def R_(s):
    return len(s["rep_status"])


def reps(s):
    return range(1, R_(s) + 1)


# ---- the predicates of the issue -------------------------------------------------------------------------------------------------------------
def stale_start_view(s):
    return any(m["type"] == po.StartViewMsg and c >= 1 and s["rep_view_number"][m["dest"] - 1] > m["view_number"] for m, c in msgs(s))


def log_divergence(s):
    for r1 in reps(s):
        for r2 in reps(s):
            a, b = s["rep_log"][r1 - 1], s["rep_log"][r2 - 1]
            if any(a[i] != b[i] for i in range(min(len(a), len(b)))):
                return True
    return False


def committed_divergence(s):
    for r1 in reps(s):
        for r2 in reps(s):
            a, b = s["rep_log"][r1 - 1], s["rep_log"][r2 - 1]
            top = min(len(a), len(b), s["rep_commit_number"][r1 - 1], s["rep_commit_number"][r2 - 1])
            if any(a[i] != b[i] for i in range(top)):
                return True
    return False


def two_normal_views(s):
    views = set(s["rep_view_number"][r - 1] for r in reps(s) if s["rep_status"][r - 1] == po.Normal)
    return len(views) > 1


def get_state_pending(s):
    return any(m["type"] == po.GetStateMsg and c >= 1 for m, c in msgs(s))


def unsettled(s):
    return not (all(st == po.Normal for st in s["rep_status"]) and len(set(s["rep_view_number"])) == 1)


def pending_request(s):
    return any((not dict(row)["executed"]) and dict(row)["request_number"] > 0 for r in reps(s) for row in s["rep_client_table"][r - 1])


def peer_lag(s):
    return any(s["rep_status"][r - 1] == po.Normal and s["rep_peer_op_number"][r - 1][p - 1] < s["rep_op_number"][p - 1] for r in reps(s) for p in reps(s))


def quorum_waiting(s):
    return any(len(s["rep_svc_recv"][r - 1]) + len(s["rep_dvc_recv"][r - 1]) >= 1 and not s["rep_sent_sv"][r - 1] for r in reps(s))


def has_op(s, r, v):
    return any(e["operation"] == v for e in entries(s, r))


def ack_not_lost(s):
    return all((not acked) or any(has_op(s, r, v) for r in reps(s)) for v, acked in s["aux_client_acked"].items())


def ack_on_majority(s):
    return all((not acked) or sum(1 for r in reps(s) if has_op(s, r, v)) >= R_(s) // 2 + 1 for v, acked in s["aux_client_acked"].items())


# ---- more constructs -------------------------------------------------------------------------------------------------------------------------
def prepare_for_old_view(s):
    return any(m["type"] == po.PrepareMsg and m["view_number"] < s["rep_view_number"][m["dest"] - 1] for m, c in msgs(s))


def same_type_two_sources(s):
    ms = msgs(s)
    return any(a["type"] == b["type"] and a["dest"] == b["dest"] and a["source"] != b["source"] for a, _ in ms for b, _ in ms)


def all_delivered(s):
    return all(c == 0 for _, c in msgs(s))


def acked_false_known(s):
    return any(not acked for acked in s["aux_client_acked"].values())


def prepare_of_acked(s):
    for m, c in msgs(s):
        if m["type"] == po.PrepareMsg:
            e = dict(m["message"])
            if e["request_number"] == 1 and s["aux_client_acked"].get(e["operation"], False):
                return True
    return False


def commit_lag(L):
    return lambda s: any(s["rep_op_number"][r - 1] - s["rep_commit_number"][r - 1] >= L // 2 + 1 for r in reps(s))


def svc_round(s):
    return (s["aux_svc"] >= 2) == any(v > 2 for v in s["rep_view_number"])


def last_normal_behind(s):
    return any(s["rep_last_normal_view"][r - 1] < s["rep_view_number"][r - 1] and s["rep_sent_dvc"][r - 1] for r in reps(s))


LOG_DIVERGENCE = r"""\E r1, r2 \in replicas : \E i \in DOMAIN rep_log[r1] :
    i \in DOMAIN rep_log[r2] /\ rep_log[r1][i] # rep_log[r2][i]"""

# the eight of set A in one compiled object: bit k = SET_A[k]
SET_A = [
    ("StaleStartView", r"\E m \in DOMAIN messages : m.type = StartViewMsg /\ messages[m] >= 1 /\ rep_view_number[m.dest] > m.view_number", stale_start_view),
    ("LogDivergence", LOG_DIVERGENCE, log_divergence),
    ("TwoNormalViews", r"\E r1, r2 \in replicas : rep_status[r1] = Normal /\ rep_status[r2] = Normal /\ rep_view_number[r1] # rep_view_number[r2]",
     two_normal_views),
    ("GetStatePending", r"\E m \in DOMAIN messages : (m.type = GetStateMsg /\ messages[m] >= 1)", get_state_pending),
    ("Unsettled", r"~((\A r \in replicas : rep_status[r] = Normal) /\ (\A r1, r2 \in replicas : rep_view_number[r1] = rep_view_number[r2]))", unsettled),
    ("PendingRequest", r"\E r \in replicas : \E c \in clients : ~rep_client_table[r][c].executed /\ rep_client_table[r][c].request_number > 0",
     pending_request),
    ("PeerLag", r"\E r, p \in replicas : rep_status[r] = Normal /\ rep_peer_op_number[r][p] < rep_op_number[p]", peer_lag),
    ("QuorumWaiting", r"\E r \in replicas : Cardinality(rep_svc_recv[r]) + Cardinality(rep_dvc_recv[r]) >= 1 /\ ~rep_sent_sv[r]", quorum_waiting),
]


def set_b(L):
    return [
        ("PrepareForOldView", r"\E m \in DOMAIN messages : m.type = PrepareMsg /\ m.view_number < rep_view_number[m.dest]", prepare_for_old_view),
        ("SameTypeTwoSources", r"\E m1, m2 \in DOMAIN messages : m1.type = m2.type /\ m1.dest = m2.dest /\ m1.source /= m2.source", same_type_two_sources),
        ("AllDelivered", r"\A m \in DOMAIN messages : messages[m] = 0", all_delivered),
        ("AckedFalseKnown", r"\E v \in Values : v \in DOMAIN aux_client_acked /\ ~aux_client_acked[v]", acked_false_known),
        ("PrepareOfAcked", r"\E m \in DOMAIN messages : m.type = PrepareMsg /\ m.message.request_number = 1 /\ aux_client_acked[m.message.operation]",
         prepare_of_acked),
        ("CommitLag", r"\E r \in replicas : rep_op_number[r] - rep_commit_number[r] >= StartViewOnTimerLimit \div 2 + 1", commit_lag(L)),
        ("SvcRound", r"(aux_svc >= 2) <=> (\E r \in replicas : rep_view_number[r] > 2)", svc_round),
        ("LastNormalBehind", r"\E r \in replicas : (rep_last_normal_view[r] =< rep_view_number[r] - 1) /\ rep_sent_dvc[r] = TRUE", last_normal_behind),
    ]


# the acknowledged-write invariants restated (TRUE = the invariant holds); the majority of 2 or 3 replicas is two distinct ones
ACK_TEXT = r"""
LOCAL Acked(* helper, not exported *) == TRUE
HasNotLost == \A v \in Values : aux_client_acked[v] =>
    (\E r \in replicas : \E i \in DOMAIN rep_log[r] : rep_log[r][i].operation = v)
OnMajority == \A v \in Values : aux_client_acked[v] =>
    (\E r1, r2 \in replicas : r1 < r2
        /\ (\E i \in DOMAIN rep_log[r1] : rep_log[r1][i].operation = v)
        /\ (\E j \in DOMAIN rep_log[r2] : rep_log[r2][j].operation = v))
CommittedDivergence == \E r1, r2 \in replicas : \E i \in 1..3 :
    i <= rep_commit_number[r1] /\ i <= rep_commit_number[r2] /\ i <= Len(rep_log[r1]) /\ i <= Len(rep_log[r2])
    /\ rep_log[r1][i] # rep_log[r2][i]
"""
ACK_FUNCS = [ack_not_lost, ack_on_majority, committed_divergence]


def text_of(preds):
    return "\n".join("%s == %s" % (name, text) for name, text, _ in preds)


def bits_of(preds, s):
    return sum((1 << k) for k, (_, _, f) in enumerate(preds) if f(s))


# ---- random well-typed expressions: text and closure built together ----------------------------------------------------------------------------
STATUS = [po.Normal, po.ViewChange, po.Recovering]
MTYPES = ["StartViewChangeMsg", "PrepareMsg", "PrepareOkMsg", "DoViewChangeMsg", "StartViewMsg", "GetStateMsg", "NewStateMsg"]
MFIELDS = ["view_number", "dest", "source", "op_number", "commit_number", "last_normal_vn", "first_op"]
CMP = {"=": lambda a, b: a == b, "#": lambda a, b: a != b, "<": lambda a, b: a < b, "<=": lambda a, b: a <= b, ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}


class Gen:
    """env: list of (name, kind) with kind 'r' (a replica number), 'i' (a log position 1..3) or 'm' (a message).  A closure takes (s, b) with b a dict
    name -> replica number / position / (message dict, count)."""

    def __init__(self, seed, R):
        self.rnd = random.Random(seed)
        self.R = R
        self.n_var = 0

    def rep_index(self, env):
        """an expression that denotes a replica: a constant, a bound replica, or (dynamic) a message's dest / source"""
        cands = [(str(k), (lambda k: lambda s, b: k)(k)) for k in range(1, self.R + 1)]
        cands += [(n, (lambda n: lambda s, b: b[n])(n)) for n, k in env if k == "r"]
        for n, k in env:
            if k == "m":
                for f in ("dest", "source"):
                    cands.append(("%s.%s" % (n, f), (lambda n, f: lambda s, b: b[n][0][f])(n, f)))
        return self.rnd.choice(cands[-6:] if len(cands) > 6 and self.rnd.random() < 0.7 else cands)

    def integer(self, env, depth):
        r = self.rnd
        k = r.randrange(8 if depth > 0 else 6)
        if k == 0:
            v = r.randrange(0, 4)
            return str(v), lambda s, b: v
        if k == 1:
            t, f = self.rep_index(env)
            name = r.choice(["rep_view_number", "rep_op_number", "rep_commit_number", "rep_last_normal_view"])
            return "%s[%s]" % (name, t), lambda s, b: s[name][f(s, b) - 1]
        if k == 2:
            t, f = self.rep_index(env)
            return "Len(rep_log[%s])" % t, lambda s, b: len(s["rep_log"][f(s, b) - 1])
        if k == 3:
            ms = [n for n, kk in env if kk == "m"]
            if ms:
                n = r.choice(ms)
                fld = r.choice(MFIELDS + ["count"])
                if fld == "count":
                    return "messages[%s]" % n, lambda s, b: b[n][1]
                return "%s.%s" % (n, fld), lambda s, b: b[n][0].get(fld, 0)
            return "aux_svc", lambda s, b: s["aux_svc"]
        if k == 4:
            t1, f1 = self.rep_index(env)
            t2, f2 = self.rep_index(env)
            return "rep_peer_op_number[%s][%s]" % (t1, t2), lambda s, b: s["rep_peer_op_number"][f1(s, b) - 1][f2(s, b) - 1]
        if k == 5:
            t, f = self.rep_index(env)
            pos = [n for n, kk in env if kk == "i"]
            if pos:
                n = r.choice(pos)
                it, itf = n, (lambda s, b: b[n])
            else:
                c = r.randrange(1, 4)
                it, itf = str(c), (lambda s, b: c)
            fld = r.choice(["view_number", "request_number", "client_id"])

            def ent(s, b):
                lg = s["rep_log"][f(s, b) - 1]
                i = itf(s, b)
                return dict(lg[i - 1])[fld] if 1 <= i <= len(lg) else 0
            return "rep_log[%s][%s].%s" % (t, it, fld), ent
        ta, fa = self.integer(env, depth - 1)
        tb, fb = self.integer(env, depth - 1)
        if k == 6:
            return "(%s + %s)" % (ta, tb), lambda s, b: fa(s, b) + fb(s, b)
        return "(%s - %s)" % (ta, tb), lambda s, b: fa(s, b) - fb(s, b)

    def boolean(self, env, depth):
        r = self.rnd
        k = r.randrange(9) if depth > 0 else r.randrange(3)
        if k == 0:
            op = r.choice(sorted(CMP))
            ta, fa = self.integer(env, 1)
            tb, fb = self.integer(env, 1)
            return "(%s %s %s)" % (ta, op, tb), lambda s, b: CMP[op](fa(s, b), fb(s, b))
        if k == 1:
            t, f = self.rep_index(env)
            st = r.choice(STATUS)
            return "(rep_status[%s] = %s)" % (t, st), lambda s, b: s["rep_status"][f(s, b) - 1] == st
        if k == 2:
            ms = [n for n, kk in env if kk == "m"]
            if ms:
                n = r.choice(ms)
                ty = r.choice(MTYPES)
                return "(%s.type = %s)" % (n, ty), lambda s, b: b[n][0]["type"] == ty
            t, f = self.rep_index(env)
            name = r.choice(["rep_sent_dvc", "rep_sent_sv"])
            return "%s[%s]" % (name, t), lambda s, b: bool(s[name][f(s, b) - 1])
        if k == 3:
            t, f = self.boolean(env, depth - 1)
            return "~%s" % t if t.startswith("(") else "~(%s)" % t, lambda s, b: not f(s, b)
        if k in (4, 5):
            op = r.choice(["/\\", "\\/", "=>", "<=>"])
            ta, fa = self.boolean(env, depth - 1)
            tb, fb = self.boolean(env, depth - 1)
            fn = {"/\\": lambda x, y: x and y, "\\/": lambda x, y: x or y, "=>": lambda x, y: (not x) or y, "<=>": lambda x, y: bool(x) == bool(y)}[op]
            return "(%s %s %s)" % (ta, op, tb), lambda s, b: fn(fa(s, b), fb(s, b))
        self.n_var += 1
        q = r.choice(["\\A", "\\E"])
        agg = all if q == "\\A" else any
        if k == 6:
            n = "r%d" % self.n_var
            t, f = self.boolean(env + [(n, "r")], depth - 1)
            return "(%s %s \\in replicas : %s)" % (q, n, t), lambda s, b: agg(f(s, dict(b, **{n: x})) for x in range(1, self.R + 1))
        if k == 7 and sum(1 for _, kk in env if kk == "m") < 2:
            n = "m%d" % self.n_var
            t, f = self.boolean(env + [(n, "m")], depth - 1)
            return "(%s %s \\in DOMAIN messages : %s)" % (q, n, t), lambda s, b: agg(f(s, dict(b, **{n: mc})) for mc in msgs(s))
        n = "i%d" % self.n_var
        rt, rf = self.rep_index(env)
        t, f = self.boolean(env + [(n, "i")], depth - 1)
        return ("(%s %s \\in DOMAIN rep_log[%s] : %s)" % (q, n, rt, t),
                lambda s, b: agg(f(s, dict(b, **{n: x})) for x in range(1, len(s["rep_log"][rf(s, b) - 1]) + 1)))


def random_predicates(seed, R, count, depth=4):
    """-> [(text, function of the unpacked state)]"""
    g = Gen(seed, R)
    out = []
    for _ in range(count):
        t, f = g.boolean([], depth)
        out.append((t, (lambda f: lambda s: bool(f(s, {})))(f)))
    return out
