"""The R >= 4 predicate sets and the harvest sample of test_deep_predicates_cpu.py / test_deep_predicates_gpu.py (and of the five- and four-replica cases of
test_sim_where_gpu.py): every predicate's TEXT beside a hand-written Python function over `pycodec.unpack(...)`, in the style of where_reference.py and
step_reference.py.  The reference is never the parser: nothing here reads the text.

What these sets read exists only in a record of four or five replicas, where a replica block has a fourth word (wpr = 1 + (R + 2) / 2 = 4):
  * the DoViewChange slots of sources 4 and 5 (word 3 of the block: Cardinality(rep_dvc_recv[r]) unfolds to R one-bit loads, two of them there; in a
    pair view StepPair::word substitutes that word from the Delta);
  * bits 3-4 of the svc mask (Cardinality(rep_svc_recv[r]) >= 4), rep_peer_op_number[r][4] and [r][ReplicaCount] (A-word bits 25-28);
  * the fourth and fifth candidate of every select chain (rep_status[4], rep_view_number[ReplicaCount], rep_log[ReplicaCount], m.dest = ReplicaCount);
  * the appended bag entries of a broadcast to R - 1 destinations (StepPair::msg numbers them in patch-slot order; the last of them is for ReplicaCount).
ReplicaCount is the last replica: 5 or 4.  Every predicate must take both verdicts at R = 5 AND at R = 4 on the sample below (test_deep_predicates_cpu.py), so
a clause that can never hold at R = 4 (a message from replica 4 to itself) stands beside one that can."""
from oracle import pyoracle as po

import step_reference as sr
import where_reference as wr

reps, msgs, R_ = wr.reps, wr.msgs, wr.R_
fld = sr.fld


# ---- the sample: one definition for the CPU and the GPU leg ---------------------------------------------------------------------------------------
N_STATES, N_PARENTS, N_RANDOM = 1500, 150, 300


def state_indices(n):
    """indices of the sampled states of a harvest of n states (an even stride of the fingerprint order)"""
    return [(k * n) // N_STATES for k in range(N_STATES)]


def parent_indices(n):
    """indices of the sampled parents: every tenth sampled state ((k * n) // 150 == ((10 * k) * n) // 1500)"""
    return [(k * n) // N_PARENTS for k in range(N_PARENTS)]


def random_indices(n):
    """the sub-stride the random expressions run on"""
    return [(k * n) // N_RANDOM for k in range(N_RANDOM)]


# what the sample must keep holding, per space: half of the figures measured when the sample was fixed (a condition on a deterministic sample: the margin is
# against a deliberate change of the harvest, not against noise).  dvc45: sampled states in which a replica holds a DoViewChange from source 4 or 5;
# bag33: sampled states with more than 32 messages; word3: pairs (150 parents, all their successors) whose successor changes the fourth word of the
# acting replica's block; bcast: pairs that append R - 1 bag entries.  0 = not a condition.
MEASURED = {
    (5, 1, 2, 1): dict(dvc45=528, bag33=360, word3=24, bcast=299),
    (4, 1, 2, 1): dict(dvc45=435, bag33=0, word3=12, bcast=103),
    (5, 1, 1, 2): dict(dvc45=706, bag33=1143, word3=123, bcast=381),
    (4, 1, 1, 2): dict(dvc45=472, bag33=286, word3=75, bcast=253),
}


def floors(key):
    return {k: (v + 1) // 2 for k, v in MEASURED[key].items() if v}


def dvc_sources(s, r):
    return set(dict(d)["source"] for d in s["rep_dvc_recv"][r - 1])


def holds_dvc_from_4_or_5(s):
    return any(src >= 4 for r in reps(s) for src in dvc_sources(s, r))


def fourth_word_changes(p, c):
    """the fourth word of a block holds the DoViewChanges of sources 4 and 5 and nothing else"""
    return any(frozenset(d for d in p["rep_dvc_recv"][r - 1] if dict(d)["source"] >= 4) != frozenset(d for d in c["rep_dvc_recv"][r - 1] if dict(d)["source"] >= 4)
               for r in reps(p))


def appended(p, c):
    """bag entries the successor has more than the parent (keys are never removed: a delivered message stays with count 0)"""
    return len(c["messages"]) - len(p["messages"])


# ---- the state set --------------------------------------------------------------------------------------------------------------------------------
def n_dvc(s, r):
    return len(s["rep_dvc_recv"][r - 1])


def n_svc(s, r):
    return len(s["rep_svc_recv"][r - 1])


def dvc_held(s):
    return any(n_dvc(s, r) >= 1 for r in reps(s))


def dvc_quorum(s):
    return any(n_dvc(s, r) >= R_(s) // 2 + 1 for r in reps(s))


def dvc_all_but_one(s):
    return any(n_dvc(s, r) >= R_(s) - 1 for r in reps(s))


def svc_four(s):
    return any(n_svc(s, r) >= 4 or (n_svc(s, r) >= 3 and n_dvc(s, r) >= 1) for r in reps(s))


def tail_view(s):
    R = R_(s)
    return s["rep_status"][3] == po.ViewChange and s["rep_status"][R - 1] != po.Normal and s["rep_view_number"][R - 1] >= s["rep_view_number"][3] \
        and s["rep_view_number"][3] >= 2


def tail_log(s):
    R = R_(s)
    first = lambda lg: lg[0] if lg else None                      # noqa: E731   (an absent entry equals an absent entry)
    return len(s["rep_log"][3]) >= 1 and first(s["rep_log"][R - 1]) == first(s["rep_log"][0])


def peer_tail(s):
    R = R_(s)
    return any(s["rep_peer_op_number"][r - 1][3] >= 1 and s["rep_peer_op_number"][r - 1][R - 1] >= s["rep_peer_op_number"][r - 1][0] for r in reps(s))


def msg_tail(s):
    R = R_(s)
    return any((m["dest"] == R and m["source"] == 4) or (m["dest"] == 4 and m["source"] == R - 1 and m["type"] == po.StartViewMsg)
               for m, c in msgs(s))


STATE = [
    ("DvcHeld", r"\E r \in replicas : Cardinality(rep_dvc_recv[r]) >= 1", dvc_held),
    ("DvcQuorum", r"\E r \in replicas : Cardinality(rep_dvc_recv[r]) >= ReplicaCount \div 2 + 1", dvc_quorum),
    ("DvcAllButOne", r"\E r \in replicas : Cardinality(rep_dvc_recv[r]) >= ReplicaCount - 1", dvc_all_but_one),
    ("SvcFour", r"\E r \in replicas : Cardinality(rep_svc_recv[r]) >= 4 \/ (Cardinality(rep_svc_recv[r]) >= 3 /\ Cardinality(rep_dvc_recv[r]) >= 1)", svc_four),
    ("TailView", r"rep_status[4] = ViewChange /\ rep_status[ReplicaCount] # Normal /\ rep_view_number[ReplicaCount] >= rep_view_number[4] /\ rep_view_number[4] >= 2",
     tail_view),
    ("TailLog", r"Len(rep_log[4]) >= 1 /\ rep_log[ReplicaCount][1] = rep_log[1][1]", tail_log),
    ("PeerTail", r"\E r \in replicas : rep_peer_op_number[r][4] >= 1 /\ rep_peer_op_number[r][ReplicaCount] >= rep_peer_op_number[r][1]", peer_tail),
    ("MsgTail", r"\E m \in DOMAIN messages : (m.dest = ReplicaCount /\ m.source = 4) \/ (m.dest = 4 /\ m.source = ReplicaCount - 1 /\ m.type = StartViewMsg)", msg_tail),
]


# ---- the step set ---------------------------------------------------------------------------------------------------------------------------------
def dvc_grew(p, c, a):
    return any(n_dvc(c, r) > n_dvc(p, r) for r in reps(p))


def dvc_shrank(p, c, a):
    return any(n_dvc(c, r) < n_dvc(p, r) for r in reps(p))


def dvc_quorum_reached(p, c, a):
    q = R_(p) // 2 + 1
    return any(n_dvc(c, r) >= q and n_dvc(p, r) < q for r in reps(p))


def svc_four_reached(p, c, a):
    return any(n_svc(c, r) >= 4 and n_svc(p, r) < 4 for r in reps(p)) or any(n_svc(c, r) == 0 and n_svc(p, r) >= 3 for r in reps(p))


def tail_status_view(p, c, a):
    R = R_(p)
    return c["rep_status"][3] != p["rep_status"][3] or c["rep_view_number"][R - 1] > p["rep_view_number"][R - 1]


def tail_unchanged(p, c, a):
    R = R_(p)
    return c["rep_status"][R - 1] == p["rep_status"][R - 1] and c["rep_view_number"][3] == p["rep_view_number"][3] and c["rep_log"][3] == p["rep_log"][3] \
        and c["rep_log"][R - 1] == p["rep_log"][R - 1] and len(c["rep_log"][R - 1]) >= len(c["rep_log"][0])


def peer_tail_moves(p, c, a):
    R = R_(p)
    return any(c["rep_peer_op_number"][r - 1][3] > p["rep_peer_op_number"][r - 1][3] or c["rep_peer_op_number"][r - 1][R - 1] != p["rep_peer_op_number"][r - 1][R - 1]
               for r in reps(p))


KEY_FIELDS = ("type", "dest", "source", "view_number", "op_number", "commit_number", "last_normal_vn", "first_op", "message")


def new_key_for_last(p, c, a):
    """the text restated: a message of the child's bag for ReplicaCount with which no message of the parent's bag agrees on every field the language reads
    (all but the log a message carries).  test_deep_predicates_cpu.py checks that on the sample this is true exactly when the child's bag holds a KEY for
    ReplicaCount that the parent's does not (new_key_for_last_by_keys)."""
    R = R_(p)
    return any(m2["dest"] == R and all(any(fld(m1, f) != fld(m2, f) for f in KEY_FIELDS) for m1, _ in msgs(p)) for m2, _ in msgs(c))


def new_key_for_last_by_keys(p, c):
    R = R_(p)
    return any(dict(k)["dest"] == R for k in set(c["messages"]) - set(p["messages"]))


STEP = [
    ("DvcGrew", r"\E r \in replicas : Cardinality(rep_dvc_recv[r])' > Cardinality(rep_dvc_recv[r])", dvc_grew),
    ("DvcShrank", r"\E r \in replicas : Cardinality(rep_dvc_recv'[r]) < Cardinality(rep_dvc_recv[r])", dvc_shrank),
    ("DvcQuorumReached", r"\E r \in replicas : Cardinality(rep_dvc_recv[r])' >= ReplicaCount \div 2 + 1 /\ Cardinality(rep_dvc_recv[r]) < ReplicaCount \div 2 + 1",
     dvc_quorum_reached),
    ("SvcFourReached", r"(\E r \in replicas : Cardinality(rep_svc_recv[r])' >= 4 /\ Cardinality(rep_svc_recv[r]) < 4) \/ "
                       r"(\E r \in replicas : Cardinality(rep_svc_recv[r])' = 0 /\ Cardinality(rep_svc_recv[r]) >= 3)", svc_four_reached),
    ("TailStatusView", r"rep_status'[4] # rep_status[4] \/ rep_view_number[ReplicaCount]' > rep_view_number[ReplicaCount]", tail_status_view),
    ("TailUnchanged", r"UNCHANGED rep_status[ReplicaCount] /\ UNCHANGED rep_view_number[4] /\ UNCHANGED rep_log[4] /\ UNCHANGED rep_log[ReplicaCount] "
                      r"/\ Len(rep_log'[ReplicaCount]) >= Len(rep_log'[1])", tail_unchanged),
    ("PeerTailMoves", r"\E r \in replicas : rep_peer_op_number'[r][4] > rep_peer_op_number[r][4] \/ rep_peer_op_number[r][ReplicaCount]' # rep_peer_op_number[r][ReplicaCount]",
     peer_tail_moves),
    ("NewKeyForLast", r"\E m2 \in DOMAIN messages' : m2.dest = ReplicaCount /\ (\A m1 \in DOMAIN messages : m1.type # m2.type \/ m1.dest # m2.dest \/ m1.source # m2.source "
                      r"\/ m1.view_number # m2.view_number \/ m1.op_number # m2.op_number \/ m1.commit_number # m2.commit_number "
                      r"\/ m1.last_normal_vn # m2.last_normal_vn \/ m1.first_op # m2.first_op \/ m1.message # m2.message)", new_key_for_last),
]

# the two predicates the simulation test needs its walks to meet: "a DoViewChange is held", "the held set grew"
SIM_STATE_MUST_HIT, SIM_STEP_MUST_HIT = "DvcHeld", "DvcGrew"

text_of = wr.text_of
