"""Reference evaluation for the step-predicate tests (test_step_cpu.py, test_step_gpu.py): every predicate's TEXT beside a hand-written Python function
f(parent, child, action) over `pycodec.unpack(...)` of the two records; `action` is the name of the Next disjunct as traces print it.  The reference is
never the parser: nothing here reads the text.

Conventions restated (csrc/vsr_where_parse.hpp): an absent log entry or message field reads 0, aux_client_acked[v] outside its domain is FALSE; a primed
expression is the same expression over the child; bound variables and constants are what they are on both sides."""
from oracle import pyoracle as po

import where_reference as wr

reps, msgs = wr.reps, wr.msgs


def fld(m, name):
    return m.get(name, 0)


# ---- the five properties of the issue ----------------------------------------------------------------------------------------------------------
def view_monotonic(p, c, a):
    return all(c["rep_view_number"][r - 1] >= p["rep_view_number"][r - 1] for r in reps(p))


def commit_monotonic(p, c, a):
    return all(c["rep_commit_number"][r - 1] >= p["rep_commit_number"][r - 1] for r in reps(p))


def log_never_shrinks(p, c, a):
    return all(len(c["rep_log"][r - 1]) >= len(p["rep_log"][r - 1]) for r in reps(p))


def log_prefix_stable(p, c, a):
    """no existing entry is replaced: every position of the old log holds the same entry afterwards (a dropped entry reads as the absent one: replaced)"""
    for r in reps(p):
        old, new = p["rep_log"][r - 1], c["rep_log"][r - 1]
        if any(i >= len(new) or old[i] != new[i] for i in range(len(old))):
            return False
    return True


def committed_prefix_stable(p, c, a):
    """no entry at or below the commit number is replaced or dropped"""
    for r in reps(p):
        old, new = p["rep_log"][r - 1], c["rep_log"][r - 1]
        for i in range(min(len(old), p["rep_commit_number"][r - 1])):
            if i >= len(new) or new[i] != old[i]:
                return False
    return True


# ---- more constructs ----------------------------------------------------------------------------------------------------------------------------
def view_changed(p, c, a):
    return any(c["rep_view_number"][r - 1] != p["rep_view_number"][r - 1] for r in reps(p))


def became_normal(p, c, a):
    return any(p["rep_status"][r - 1] != po.Normal and c["rep_status"][r - 1] == po.Normal for r in reps(p))


KEYF = ("type", "dest", "source", "view_number", "op_number")


def bag_grew(p, c, a):
    """a message of the child's bag that no message of the parent's bag agrees with on (type, dest, source, view_number, op_number)"""
    return any(all(any(fld(m1, f) != fld(m2, f) for f in KEYF) for m1, _ in msgs(p)) for m2, _ in msgs(c))


def new_start_view(p, c, a):
    return any(m["type"] == po.StartViewMsg and n >= 1 and m["view_number"] > p["rep_view_number"][m["dest"] - 1] for m, n in msgs(c))


def delivered(p, c, a):
    return any(n == 0 for _, n in msgs(c))


def acked_flip(p, c, a):
    return any(c["aux_client_acked"].get(v, False) and not p["aux_client_acked"].get(v, False) for v in set(c["aux_client_acked"]) | set(p["aux_client_acked"]))


def svc_increment(p, c, a):
    return c["aux_svc"] == p["aux_svc"] + 1


def unchanged_log_1(p, c, a):
    return c["rep_log"][0] == p["rep_log"][0]


def dest_view_ahead(p, c, a):
    return any(n > 0 and c["rep_view_number"][m["dest"] - 1] > m["view_number"] for m, n in msgs(p))


def receive_sv_keeps_commit(p, c, a):
    return a != "ReceiveSV" or commit_monotonic(p, c, a)


def status_only(p, c, a):
    return c["rep_view_number"] == p["rep_view_number"] and c["rep_status"] != p["rep_status"]


def counts_kept(p, c, a):
    """every message of the parent's bag has one in the child's that agrees on (type, dest, source, view_number) and whose count is not smaller"""
    return all(any(all(fld(m1, f) == fld(m2, f) for f in KEYF[:4]) and n2 >= n1 for m2, n2 in msgs(c)) for m1, n1 in msgs(p))


def unchanged_aux_svc(p, c, a):
    return c["aux_svc"] == p["aux_svc"]


def not_timer(p, c, a):
    return a != "TimerSendSVC"


def unchanged_logs(p, c, a):
    return c["rep_log"] == p["rep_log"]


def op_sum_grows(p, c, a):
    return c["rep_op_number"][0] + len(c["rep_log"][1]) > p["rep_op_number"][0] + len(p["rep_log"][1])


def acked_domain_grows(p, c, a):
    return any(v in c["aux_client_acked"] and v not in p["aux_client_acked"] for v in c["aux_client_acked"])


def first_entry_kept(p, c, a):
    e0 = lambda s: s["rep_log"][0][0] if s["rep_log"][0] else None   # noqa: E731
    return e0(p) == e0(c)


def send_shrinks(p, c, a):
    return a in ("SendSV", "SendGetState") and not log_never_shrinks(p, c, a)


VIEW_MONOTONIC = r"\A r \in replicas : rep_view_number'[r] >= rep_view_number[r]"
COMMIT_MONOTONIC = r"\A r \in replicas : rep_commit_number'[r] >= rep_commit_number[r]"
LOG_NEVER_SHRINKS = r"\A r \in replicas : Len(rep_log[r])' >= Len(rep_log[r])"
LOG_PREFIX_STABLE = r"\A r \in replicas : \A i \in DOMAIN rep_log[r] : rep_log'[r][i] = rep_log[r][i]"
COMMITTED_PREFIX_STABLE = (r"\A r \in replicas : \A i \in DOMAIN rep_log[r] : i <= rep_commit_number[r] => "
                           r"(i \in DOMAIN rep_log'[r] /\ rep_log[r][i]' = rep_log[r][i])")

# set A: every predicate takes both verdicts on the spaces the GPU test walks
SET_A = [
    ("ViewChanged", r"\E r \in replicas : rep_view_number'[r] # rep_view_number[r]", view_changed),
    ("BecameNormal", r"\E r \in replicas : rep_status[r] # Normal /\ rep_status'[r] = Normal", became_normal),
    ("BagGrew", r"\E m2 \in DOMAIN messages' : \A m1 \in DOMAIN messages : m1.type # m2.type \/ m1.dest # m2.dest \/ m1.source # m2.source "
                r"\/ m1.view_number # m2.view_number \/ m1.op_number # m2.op_number", bag_grew),
    ("NewStartView", r"\E m \in DOMAIN messages' : m.type = StartViewMsg /\ messages'[m] >= 1 /\ m.view_number > rep_view_number[m.dest]", new_start_view),
    ("Delivered", r"\E m \in DOMAIN messages' : messages'[m] = 0", delivered),
    ("AckedFlip", r"\E v \in Values : aux_client_acked'[v] /\ ~aux_client_acked[v]", acked_flip),
    ("SvcIncrement", r"aux_svc' = aux_svc + 1", svc_increment),
    ("CommitMonotonic", COMMIT_MONOTONIC, commit_monotonic),
]

# set B: ViewMonotonic is TRUE on every pair of these spaces, the other seven take both verdicts
SET_B = [
    ("ViewMonotonic", VIEW_MONOTONIC, view_monotonic),
    ("LogNeverShrinks", LOG_NEVER_SHRINKS, log_never_shrinks),
    ("LogPrefixStable", LOG_PREFIX_STABLE, log_prefix_stable),
    ("UnchangedLog1", r"UNCHANGED rep_log[1]", unchanged_log_1),
    ("DestViewAhead", r"\E m \in DOMAIN messages : messages[m] > 0 /\ rep_view_number'[m.dest] > m.view_number", dest_view_ahead),
    ("ReceiveSVKeepsCommit", r"step_action = ReceiveSV => (\A r \in replicas : rep_commit_number[r]' >= rep_commit_number[r])", receive_sv_keeps_commit),
    ("StatusOnly", r"UNCHANGED rep_view_number /\ ~UNCHANGED rep_status", status_only),
    ("CountsKept", r"\A m1 \in DOMAIN messages : \E m2 \in DOMAIN messages' : m1.type = m2.type /\ m1.dest = m2.dest /\ m1.source = m2.source "
                   r"/\ m1.view_number = m2.view_number /\ messages'[m2] >= messages[m1]", counts_kept),
]

# set C: the fifth property (TRUE on every pair of these spaces, like ViewMonotonic: a set of eight may hold one such predicate) and further forms
SET_C = [
    ("CommittedPrefixStable", COMMITTED_PREFIX_STABLE, committed_prefix_stable),
    ("UnchangedAuxSvc", r"UNCHANGED aux_svc", unchanged_aux_svc),
    ("NotTimer", r"step_action # TimerSendSVC", not_timer),
    ("UnchangedLogs", r"UNCHANGED rep_log", unchanged_logs),
    ("OpSumGrows", r"(rep_op_number[1] + Len(rep_log[2]))' > rep_op_number[1] + Len(rep_log[2])", op_sum_grows),
    ("AckedDomainGrows", r"\E v \in Values : v \in DOMAIN aux_client_acked' /\ ~(v \in DOMAIN aux_client_acked)", acked_domain_grows),
    ("FirstEntryKept", r"UNCHANGED rep_log[1][1]", first_entry_kept),
    ("SendShrinks", r"(step_action = SendSV \/ step_action = SendGetState) /\ ~(" + LOG_NEVER_SHRINKS + ")", send_shrinks),
]

FIVE = [("ViewMonotonic", VIEW_MONOTONIC, view_monotonic), ("CommitMonotonic", COMMIT_MONOTONIC, commit_monotonic),
        ("LogNeverShrinks", LOG_NEVER_SHRINKS, log_never_shrinks), ("LogPrefixStable", LOG_PREFIX_STABLE, log_prefix_stable),
        ("CommittedPrefixStable", COMMITTED_PREFIX_STABLE, committed_prefix_stable)]

text_of = wr.text_of


def bits_of(preds, p, c, a):
    return sum((1 << k) for k, (_, _, f) in enumerate(preds) if f(p, c, a))
