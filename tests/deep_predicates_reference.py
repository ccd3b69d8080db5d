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


# =====================================================================================================================
# TWO CLIENTS: the sets of the two-client spaces (deep_harvest.SPACES_C2; three replicas, so the R >= 4 sets above do not apply).  What they read exists only in
# a record of ClientCount = 2: the second row of a replica's client table (A-word bits of row 2; `\E c \in clients` unfolds to two rows; a client index that
# is an expression becomes a select chain over two candidates), client_id = 2 inside log entries and inside the entry a PrepareMsg carries, the constant
# ClientCount, and - in a pair - the row that ReceivePrepareMsg rewrites although the appended entry is the other client's (VSR.tla:414-421).
# =====================================================================================================================
def row(s, r, c):
    return dict(s["rep_client_table"][r - 1][c - 1])


def C_(s):
    return len(s["rep_client_table"][0])


def clients(s):
    return range(1, C_(s) + 1)


def client2_pending(s):
    return any(row(s, r, 2)["request_number"] > 0 and not row(s, r, 2)["executed"] for r in reps(s))


def later_client_later(s):
    """the body differs between c = 1 and c = 2: client 2's request must sit at op number 2 or above"""
    return all(row(s, 1, c)["request_number"] > 0 and row(s, 1, c)["op_number"] >= c for c in clients(s))


def client2_committed(s):
    return any(i + 1 <= s["rep_commit_number"][r - 1] and e["client_id"] == 2 for r in reps(s) for i, e in enumerate(wr.entries(s, r)))


def msg_of_client2(s):
    return any(n >= 1 and m["type"] == po.PrepareMsg and dict(m["message"])["client_id"] == 2 for m, n in msgs(s))


def last_client_asked(s):
    return C_(s) == 2 and row(s, R_(s), C_(s))["request_number"] > 0


def rows_differ(s):
    return any(row(s, r, 1)["executed"] != row(s, r, 2)["executed"] for r in reps(s))


def row_of_prepare(s):
    """a client index that is an expression: the row of the client whose entry a PrepareMsg carries, at the destination"""
    return any(m["type"] == po.PrepareMsg and row(s, m["dest"], dict(m["message"])["client_id"])["op_number"] == m["op_number"] for m, n in msgs(s))


STATE_C2 = [
    ("Client2Pending", r"\E r \in replicas : rep_client_table[r][2].request_number > 0 /\ ~rep_client_table[r][2].executed", client2_pending),
    ("LaterClientLater", r"\A c \in clients : rep_client_table[1][c].request_number > 0 /\ rep_client_table[1][c].op_number >= c", later_client_later),
    ("Client2Committed", r"\E r \in replicas : \E i \in DOMAIN rep_log[r] : i <= rep_commit_number[r] /\ rep_log[r][i].client_id = 2", client2_committed),
    ("MsgOfClient2", r"\E m \in DOMAIN messages : messages[m] >= 1 /\ m.message.client_id = 2", msg_of_client2),
    ("LastClientAsked", r"ClientCount = 2 /\ rep_client_table[ReplicaCount][ClientCount].request_number > 0", last_client_asked),
    ("RowsDiffer", r"\E r \in replicas : rep_client_table[r][1].executed # rep_client_table[r][2].executed", rows_differ),
    ("RowOfPrepare", r"\E m \in DOMAIN messages : m.type = PrepareMsg /\ rep_client_table[m.dest][m.message.client_id].op_number = m.op_number", row_of_prepare),
]


def appended_entry_of(p, c, r, client):
    """replica r's log has a position in the child that the parent's has not, and the entry there is `client`'s"""
    return any(i >= len(p["rep_log"][r - 1]) and e["client_id"] == client for i, e in enumerate(wr.entries(c, r)))


def other_row_rewritten(mine, other):
    """the row of `other` differs at a replica whose log gained an entry of `mine`, under ReceivePrepareMsg: the row the else branch of VSR.tla:414-421 rewrites"""
    return lambda p, c, a: a == "ReceivePrepareMsg" and any(row(c, r, other) != row(p, r, other) and appended_entry_of(p, c, r, mine) for r in reps(p))


def row1_unchanged(p, c, a):
    return all(row(c, r, 1) == row(p, r, 1) for r in reps(p))


def executed_rose(p, c, a):
    return any(row(c, r, cl)["executed"] and not row(p, r, cl)["executed"] for r in reps(p) for cl in clients(p))


def executed_rises_only_on_execute_op(p, c, a):
    """"the executed bit of either client rises only on ExecuteOp or ReceivePrepareMsg" is TRUE on every pair of these spaces (the bit rose on 133 + 120 sampled
    pairs, all of them of those two actions), so it cannot take both verdicts.  This is the same implication with the second action left out: false exactly where
    ReceivePrepareMsg raises a bit (90 and 84 sampled pairs), among them the rows the else branch of VSR.tla:414-421 recomputes."""
    return (not executed_rose(p, c, a)) or a == "ExecuteOp"


def last_client_entry_appended(p, c, a):
    return any(appended_entry_of(p, c, r, C_(p)) for r in reps(p))


def _other_row_text(mine, other):
    t = "rep_client_table'[r][%d]" % other
    u = "rep_client_table[r][%d]" % other
    return (r"step_action = ReceivePrepareMsg /\ (\E r \in replicas : (%s.executed # %s.executed \/ %s.request_number # %s.request_number \/ %s.op_number # %s.op_number) "
            r"/\ (\E i \in DOMAIN rep_log'[r] : ~(i \in DOMAIN rep_log[r]) /\ rep_log'[r][i].client_id = %d))" % (t, u, t, u, t, u, mine))


STEP_C2 = [
    ("Row2RewrittenByClient1", _other_row_text(1, 2), other_row_rewritten(1, 2)),
    ("Row1RewrittenByClient2", _other_row_text(2, 1), other_row_rewritten(2, 1)),
    ("Row1Unchanged", r"\A r \in replicas : UNCHANGED rep_client_table[r][1].request_number /\ UNCHANGED rep_client_table[r][1].op_number "
                      r"/\ UNCHANGED rep_client_table[r][1].executed", row1_unchanged),
    ("ExecutedRose", r"\E r \in replicas : \E c \in clients : rep_client_table[r][c].executed' /\ ~rep_client_table[r][c].executed", executed_rose),
    ("ExecutedRisesOnlyOnExecuteOp", r"(\E r \in replicas : \E c \in clients : rep_client_table'[r][c].executed /\ ~rep_client_table[r][c].executed) "
                                     r"=> step_action = ExecuteOp", executed_rises_only_on_execute_op),
    ("LastClientEntryAppended", r"\E r \in replicas : \E i \in DOMAIN rep_log'[r] : ~(i \in DOMAIN rep_log[r]) /\ rep_log'[r][i].client_id = ClientCount",
     last_client_entry_appended),
]
N_C2_FLIP_PARENTS = 75
BOTH_VERDICTS = 20                                                  # every two-client predicate: true on at least 20 and false on at least 20 sampled items
SIM_C2_STATE_MUST_HIT, SIM_C2_STEP_MUST_HIT = "Client2Pending", "LastClientEntryAppended"


def c2_parent_indices(n, flip_states):
    """the 150 sampled parents of a two-client harvest of n states: an even stride of 75, and an even stride of 75 of the states in which ReceivePrepareMsg flips
    the executed bit of a row it did not write (deep_harvest.c2_facts: flip_states of client 1 and 2 together) - an even stride of the harvest alone holds about
    six such pairs"""
    first = [(k * n) // (N_PARENTS - N_C2_FLIP_PARENTS) for k in range(N_PARENTS - N_C2_FLIP_PARENTS)]
    rest = sorted(set(flip_states) - set(first))
    return sorted(first + [rest[(k * len(rest)) // N_C2_FLIP_PARENTS] for k in range(N_C2_FLIP_PARENTS)])


def state_sets(key):
    """(tag, predicates) of the state sets of a space"""
    return (("A", wr.SET_A), ("B", wr.set_b(key[3])), ("C2", STATE_C2) if key[1] == 2 else ("R4", STATE))


def step_sets(key):
    return (("A", sr.SET_A), ("B", sr.SET_B), ("C", sr.SET_C), ("C2", STEP_C2) if key[1] == 2 else ("R4", STEP))
