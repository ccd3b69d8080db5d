"""Reference evaluation for the step-predicate tests of the two analysis models (test_step_models_cpu.py, test_step_models_gpu.py): every predicate's TEXT
beside a hand-written Python function f(parent, child, action) over `pyoracle2.unpack(...)` / `pyoracle3.unpack(...)` of the CPU oracles' records and
successors; `action` is the name of the Next disjunct as traces print it.  The reference is never the parser: nothing here reads the text.

Conventions restated (csrc/vsr_where_parse.hpp): those of tests/where_models_reference.py on either side of a pair; a primed expression is the same
expression over the child; bound variables and constants are what they are on both sides; a d bound over rep_recv_dvc'[r] is the child's."""
from oracle import pyoracle2 as p2

import where_models_reference as wm

MODELS = wm.MODELS
reps, msgs, rlog, rapp, held, mlog, mf, dlog = wm.reps, wm.msgs, wm.rlog, wm.rapp, wm.held, wm.mlog, wm.mf, wm.dlog
KEY = ("type", "view_number", "dest", "source", "op_number", "commit_number", "last_normal_vn", "first_op")


def same_key(m1, m2):
    """two bag keys agree on every field the language reads and on their logs"""
    return all(mf(m1, f) == mf(m2, f) if f != "type" else m1["type"] == m2["type"] for f in KEY) and mlog(m1) == mlog(m2) and wm.mmsg(m1) == wm.mmsg(m2)


SAME_KEY = (r"m1.type = m2.type /\ m1.view_number = m2.view_number /\ m1.dest = m2.dest /\ m1.source = m2.source /\ m1.op_number = m2.op_number "
            r"/\ m1.commit_number = m2.commit_number /\ m1.last_normal_vn = m2.last_normal_vn /\ m1.first_op = m2.first_op /\ m1.message = m2.message "
            r"/\ (\A i \in 1..3 : m1.log[i] = m2.log[i])")


def new_keys(p, c):
    """the messages of the child's bag whose key the parent's bag does not hold"""
    old = [m for m, _ in msgs(p)]
    return [m for m, _ in msgs(c) if not any(same_key(m1, m) for m1 in old)]


def actor(p, c):
    """the replicas whose own variables differ between the two states"""
    names = [k for k in p if k.startswith("rep_") or k == "no_progress"]
    return [r for r in reps(p) if any(p[k][r - 1] != c[k][r - 1] for k in names)]


# ---- the properties of the issue ---------------------------------------------------------------------------------------------------------------
def commit_monotonic(p, c, a):
    return all(c["rep_commit_number"][r - 1] >= p["rep_commit_number"][r - 1] for r in reps(p))


def log_never_shrinks(p, c, a):
    return all(len(c["rep_log"][r - 1]) >= len(p["rep_log"][r - 1]) for r in reps(p))


def op_monotonic(p, c, a):
    return all(c["rep_op_number"][r - 1] >= p["rep_op_number"][r - 1] for r in reps(p))


def view_monotonic(p, c, a):
    return all(c["rep_view_number"][r - 1] >= p["rep_view_number"][r - 1] for r in reps(p))


def committed_prefix_stable(p, c, a):
    """no entry at or below the commit number is replaced or dropped"""
    for r in reps(p):
        old, new = rlog(p, r), rlog(c, r)
        if any(i <= p["rep_commit_number"][r - 1] and new.get(i) != v for i, v in old.items()):
            return False
    return True


def enters_state_transfer(p, c, a):
    return any(p["rep_status"][r - 1] != p2.StateTransfer and c["rep_status"][r - 1] == p2.StateTransfer for r in reps(p))


def leaves_state_transfer(p, c, a):
    return any(p["rep_status"][r - 1] == p2.StateTransfer and c["rep_status"][r - 1] != p2.StateTransfer for r in reps(p))


def new_state_appears(p, c, a):
    return any(m["type"] == p2.NewStateMsg for m in new_keys(p, c))


def new_dvc_shorter_than_commit(p, c, a):
    return any(m["type"] == p2.DoViewChangeMsg and any(cn > len(mlog(m)) for cn in p["rep_commit_number"]) for m in new_keys(p, c))


def app_prefix_stable(p, c, a):
    """rep_app_state[r] never shrinks and never changes below its old length"""
    return all(rapp(c, r).get(i) == v for r in reps(p) for i, v in rapp(p, r).items())


def held_dvcs_dropped(p, c, a):
    return any(len(c["rep_recv_dvc"][r - 1]) < len(p["rep_recv_dvc"][r - 1]) for r in reps(p))


def held_unchanged(p, c, a):
    return all(c["rep_recv_dvc"][r - 1] == p["rep_recv_dvc"][r - 1] for r in reps(p))


def count_goes_down(p, c, a):
    """a key of both bags whose count is one less afterwards: the message the step received"""
    return any(same_key(m1, m2) and n2 == n1 - 1 for m2, n2 in msgs(c) for m1, n1 in msgs(p))


COMMIT_MONOTONIC = r"\A r \in replicas : rep_commit_number'[r] >= rep_commit_number[r]"
LOG_NEVER_SHRINKS = r"\A r \in replicas : Len(rep_log'[r]) >= Len(rep_log[r])"
OP_MONOTONIC = r"\A r \in replicas : rep_op_number[r]' >= rep_op_number[r]"
VIEW_MONOTONIC = r"\A r \in replicas : rep_view_number'[r] >= rep_view_number[r]"
COMMITTED_PREFIX_STABLE = (r"\A r \in replicas : \A i \in DOMAIN rep_log[r] : i <= rep_commit_number[r] => "
                           r"(i \in DOMAIN rep_log'[r] /\ rep_log[r][i]' = rep_log[r][i])")
ENTERS = r"\E r \in replicas : rep_status[r] # StateTransfer /\ rep_status'[r] = StateTransfer"
LEAVES = r"\E r \in replicas : rep_status[r] = StateTransfer /\ rep_status[r]' # StateTransfer"
NEW_STATE_APPEARS = r"\E m2 \in DOMAIN messages' : m2.type = NewStateMsg /\ (\A m1 \in DOMAIN messages : ~(" + SAME_KEY + "))"
NEW_DVC_SHORTER = (r"\E m2 \in DOMAIN messages' : m2.type = DoViewChangeMsg /\ (\E r \in replicas : rep_commit_number[r] > Len(m2.log)) "
                   r"/\ (\A m1 \in DOMAIN messages : ~(" + SAME_KEY + "))")
COUNT_GOES_DOWN = r"\E m2 \in DOMAIN messages' : \E m1 \in DOMAIN messages : " + SAME_KEY + r" /\ messages'[m2] = messages[m1] - 1"
APP_PREFIX_STABLE = r"\A r \in replicas : \A i \in DOMAIN rep_app_state[r] : i \in DOMAIN rep_app_state'[r] /\ rep_app_state'[r][i] = rep_app_state[r][i]"
HELD_DROPPED = r"\E r \in replicas : Cardinality(rep_recv_dvc[r])' < Cardinality(rep_recv_dvc[r])"
HELD_UNCHANGED = (r"\A r \in replicas : Cardinality(rep_recv_dvc[r])' = Cardinality(rep_recv_dvc[r]) /\ (\A d \in rep_recv_dvc'[r] : \E e \in rep_recv_dvc[r] : "
                  r"e.source = d.source /\ e.view_number = d.view_number /\ e.last_normal_vn = d.last_normal_vn /\ e.op_number = d.op_number "
                  r"/\ e.commit_number = d.commit_number /\ Len(e.log) = Len(d.log) /\ (\A i \in 1..3 : e.log[i] = d.log[i]))")

SIX = [
    ("LogNeverShrinks", LOG_NEVER_SHRINKS, log_never_shrinks),
    ("OpMonotonic", OP_MONOTONIC, op_monotonic),
    ("EntersStateTransfer", ENTERS, enters_state_transfer),
    ("LeavesStateTransfer", LEAVES, leaves_state_transfer),
    ("NewStateAppears", NEW_STATE_APPEARS, new_state_appears),
    ("NewDvcShorterThanCommit", NEW_DVC_SHORTER, new_dvc_shorter_than_commit),
]
# set A: every predicate takes both verdicts on the pairs the GPU tests 1 and 2 walk (CommitMonotonic is false on VR_STATE_TRANSFER.tla alone, and only on
# four pairs out of level 12 of (3, {v1,v2}, 1): the directed subset holds them)
SET_A = {
    "second": SIX + [("CommitMonotonic", COMMIT_MONOTONIC, commit_monotonic), ("CountGoesDown", COUNT_GOES_DOWN, count_goes_down)],
    "third": SIX + [("HeldDvcsDropped", HELD_DROPPED, held_dvcs_dropped), ("HeldUnchanged", HELD_UNCHANGED, held_unchanged)],
}


# ---- set B: at least seven of eight take both verdicts -----------------------------------------------------------------------------------------
def status_only(p, c, a):
    return c["rep_view_number"] == p["rep_view_number"] and c["rep_status"] != p["rep_status"]


def unchanged_logs(p, c, a):
    return c["rep_log"] == p["rep_log"]


def no_progress_kept(p, c, a):
    return c["no_progress"] == p["no_progress"] and c["no_progress_ctr"] == p["no_progress_ctr"]


def peer_op_grows(p, c, a):
    return any(c["rep_peer_op_number"][r - 1][q - 1] > p["rep_peer_op_number"][r - 1][q - 1] for r in reps(p) for q in reps(p))


def acked_flip(p, c, a):
    return any(c["aux_client_acked"].get(v, False) and not p["aux_client_acked"].get(v, False) for v in set(c["aux_client_acked"]) | set(p["aux_client_acked"]))


def svc_increment(p, c, a):
    return c["aux_svc"] == p["aux_svc"] + 1


def receive_sv_keeps_log(p, c, a):
    return a != "ReceiveSV" or log_never_shrinks(p, c, a)


def first_entry_kept(p, c, a):
    return rlog(p, 1).get(1) == rlog(c, 1).get(1)


SET_B = [
    ("StatusOnly", r"UNCHANGED rep_view_number /\ ~UNCHANGED rep_status", status_only),
    ("UnchangedLogs", r"UNCHANGED rep_log", unchanged_logs),
    ("NoProgressKept", r"UNCHANGED no_progress /\ no_progress_ctr' = no_progress_ctr", no_progress_kept),
    ("PeerOpGrows", r"\E r, q \in replicas : rep_peer_op_number'[r][q] > rep_peer_op_number[r][q]", peer_op_grows),
    ("AckedFlip", r"\E v \in Values : aux_client_acked'[v] /\ ~aux_client_acked[v]", acked_flip),
    ("SvcIncrement", r"aux_svc' = aux_svc + 1", svc_increment),
    ("ReceiveSVKeepsLog", r"step_action = ReceiveSV => (" + LOG_NEVER_SHRINKS + ")", receive_sv_keeps_log),
    ("FirstEntryKept", r"UNCHANGED rep_log[1][1]", first_entry_kept),
]


# ---- set C: properties that hold on every pair of these spaces, and further forms; no condition on the verdicts -----------------------------------------
def unchanged_log_2(p, c, a):
    return c["rep_log"][1] == p["rep_log"][1]


def timer_keeps(p, c, a):
    return a != "TimerSendSVC" or (c["rep_log"] == p["rep_log"] and c["rep_commit_number"] == p["rep_commit_number"] and c["aux_svc"] == p["aux_svc"] + 1)


def sv_carries_senders_log(p, c, a):
    """every new StartViewMsg carries the log its sender has afterwards"""
    return all(m["type"] != p2.StartViewMsg or mlog(m) == rlog(c, m["source"]) for m in new_keys(p, c))


def acked_domain_grows(p, c, a):
    return any(v not in p["aux_client_acked"] for v in c["aux_client_acked"])


def op_sum_grows(p, c, a):
    return c["rep_op_number"][0] + len(c["rep_log"][1]) > p["rep_op_number"][0] + len(p["rep_log"][1])


SET_C = [
    ("CommittedPrefixStable", COMMITTED_PREFIX_STABLE, committed_prefix_stable),
    ("ViewMonotonic", VIEW_MONOTONIC, view_monotonic),
    ("UnchangedLog2", r"UNCHANGED rep_log[2]", unchanged_log_2),
    ("TimerKeeps", r"step_action = TimerSendSVC => (UNCHANGED rep_log /\ UNCHANGED rep_commit_number /\ aux_svc' = aux_svc + 1)", timer_keeps),
    ("SvCarriesSendersLog", r"\A m2 \in DOMAIN messages' : (m2.type = StartViewMsg /\ (\A m1 \in DOMAIN messages : ~(" + SAME_KEY + r"))) => "
                            r"(Len(m2.log) = Len(rep_log'[m2.source]) /\ (\A i \in DOMAIN m2.log : m2.log[i] = rep_log'[m2.source][i]))", sv_carries_senders_log),
    ("AckedDomainGrows", r"\E v \in Values : v \in DOMAIN aux_client_acked' /\ ~(v \in DOMAIN aux_client_acked)", acked_domain_grows),
    ("OpSumGrows", r"(rep_op_number[1] + Len(rep_log[2]))' > rep_op_number[1] + Len(rep_log[2])", op_sum_grows),
    ("CommitMonotonic", COMMIT_MONOTONIC, commit_monotonic),
]


# ---- VR_APP_STATE.tla only: rep_app_state' and rep_recv_dvc' ---------------------------------------------------------------------------------------------
def app_grows(p, c, a):
    return any(len(c["rep_app_state"][r - 1]) > len(p["rep_app_state"][r - 1]) for r in reps(p))


def app_follows_log(p, c, a):
    return all(rlog(c, r).get(i) == v for r in reps(c) for i, v in rapp(c, r).items())


def unchanged_app(p, c, a):
    return c["rep_app_state"] == p["rep_app_state"]


def unchanged_app_2(p, c, a):
    return c["rep_app_state"][1] == p["rep_app_state"][1]


def held_grows(p, c, a):
    return any(len(c["rep_recv_dvc"][r - 1]) > len(p["rep_recv_dvc"][r - 1]) for r in reps(p))


def new_held_whole_log(p, c, a):
    return any(all(e["source"] != d["source"] for e in held(p, r)) and len(d["log"]) == d["op_number"] for r in reps(p) for d in held(c, r))


def held_log_differs(p, c, a):
    return any(v != rlog(c, r).get(i) for r in reps(c) for d in held(c, r) for i, v in dlog(d).items())


SET_3 = [
    ("AppPrefixStable", APP_PREFIX_STABLE, app_prefix_stable),
    ("AppGrows", r"\E r \in replicas : Len(rep_app_state'[r]) > Len(rep_app_state[r])", app_grows),
    ("AppFollowsLog", r"\A r \in replicas : \A i \in DOMAIN rep_app_state'[r] : rep_app_state'[r][i] = rep_log'[r][i]", app_follows_log),
    ("UnchangedApp", r"UNCHANGED rep_app_state", unchanged_app),
    ("UnchangedApp2", r"UNCHANGED rep_app_state[2]", unchanged_app_2),
    ("HeldGrows", r"\E r \in replicas : Cardinality(rep_recv_dvc'[r]) > Cardinality(rep_recv_dvc[r])", held_grows),
    ("NewHeldWholeLog", r"\E r \in replicas : \E d \in rep_recv_dvc'[r] : (\A e \in rep_recv_dvc[r] : e.source # d.source) /\ Len(d.log) = d.op_number", new_held_whole_log),
    ("HeldLogDiffers", r"(\E r \in replicas : \E d \in rep_recv_dvc[r] : \E i \in DOMAIN d.log : d.log[i].operation # rep_log[r][i].operation)'", held_log_differs),
]


# ---- the neighbour word: primed variables of every replica on steps that rewrite one block ---------------------------------------------------------------
def send_dvc_keeps_commit(p, c, a):
    return a != "SendDVC" or c["rep_commit_number"] == p["rep_commit_number"]


def sent_dvc_in_view_change(p, c, a):
    return a != "SendDVC" or all((not c["rep_sent_dvc"][r - 1]) or c["rep_status"][r - 1] == p2.ViewChange for r in reps(c))


def timer_keeps_logs(p, c, a):
    return a != "TimerSendSVC" or c["rep_log"] == p["rep_log"]


def lnv_below_view(p, c, a):
    return all(c["rep_last_normal_view"][r - 1] <= c["rep_view_number"][r - 1] for r in reps(c))


def one_view_raised(p, c, a):
    same = lambda q: all(c[k][q - 1] == p[k][q - 1] for k in ("rep_view_number", "rep_status", "rep_op_number"))   # noqa: E731
    return any(c["rep_view_number"][r - 1] > p["rep_view_number"][r - 1] and all(q == r or same(q) for q in reps(p)) for r in reps(p))


def peers_kept(p, c, a):
    return a == "ReceivePrepareOkMsg" or c["rep_peer_op_number"] == p["rep_peer_op_number"]


def one_held_changed(p, c, a):
    n = lambda s, r: len(s["rep_recv_dvc"][r - 1])   # noqa: E731
    return any(n(c, r) != n(p, r) and all(q == r or n(c, q) == n(p, q) for q in reps(p)) for r in reps(p))


def others_app_kept(p, c, a):
    return a in ("ExecuteOp", "ReceiveSV", "ReceivePrepareMsg", "ReceiveNewState") or c["rep_app_state"] == p["rep_app_state"]


NEIGHBOUR = [
    ("SendDvcKeepsCommit", r"step_action = SendDVC => UNCHANGED rep_commit_number", send_dvc_keeps_commit),
    ("SentDvcInViewChange", r"\A r \in replicas : step_action = SendDVC => (rep_sent_dvc'[r] => rep_status'[r] = ViewChange)", sent_dvc_in_view_change),
    ("TimerKeepsLogs", r"step_action = TimerSendSVC => UNCHANGED rep_log", timer_keeps_logs),
    ("LnvBelowView", r"\A r \in replicas : rep_last_normal_view'[r] <= rep_view_number'[r]", lnv_below_view),
    ("OneViewRaised", r"\E r \in replicas : rep_view_number'[r] > rep_view_number[r] /\ (\A q \in replicas : q = r \/ (rep_view_number'[q] = rep_view_number[q] "
                      r"/\ rep_status'[q] = rep_status[q] /\ rep_op_number'[q] = rep_op_number[q]))", one_view_raised),
    ("PeersKept", r"step_action = ReceivePrepareOkMsg \/ (\A r, q \in replicas : rep_peer_op_number'[r][q] = rep_peer_op_number[r][q])", peers_kept),
]
NEIGHBOUR_3 = [
    ("OneHeldChanged", r"\E r \in replicas : Cardinality(rep_recv_dvc[r])' # Cardinality(rep_recv_dvc[r]) /\ (\A q \in replicas : q = r "
                       r"\/ Cardinality(rep_recv_dvc[q])' = Cardinality(rep_recv_dvc[q]))", one_held_changed),
    ("OthersAppKept", r"step_action = ExecuteOp \/ step_action = ReceiveSV \/ step_action = ReceivePrepareMsg \/ step_action = ReceiveNewState \/ UNCHANGED rep_app_state",
     others_app_kept),
]

# the example files' properties, by name (tools/steps_model2_example.txt, tools/steps_model3_example.txt)
EXAMPLE = {"CommitMonotonic": commit_monotonic, "LogNeverShrinks": log_never_shrinks, "CommittedPrefixStable": committed_prefix_stable,
           "EntersStateTransfer": enters_state_transfer, "NewStateAppears": new_state_appears, "AppPrefixStable": app_prefix_stable,
           "HeldDvcsDropped": held_dvcs_dropped}


def sets(which):
    """[(tag, predicates)]: every set of a model — one compiled object each (at most eight names)"""
    out = [("A", SET_A[which]), ("B", SET_B), ("C", SET_C)]
    if which == "third":
        out.append(("T", SET_3))
    return out


def neighbour(which):
    return NEIGHBOUR + (NEIGHBOUR_3 if which == "third" else [])


text_of = wm.text_of


def bits_of(preds, p, c, a):
    return sum((1 << k) for k, (_, _, f) in enumerate(preds) if f(p, c, a))
