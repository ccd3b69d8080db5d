"""The action bodies and the predicate language at TWO CLIENTS, CPU leg (`-m "not gpu"`): what test_two_clients_gpu.py and the two-client cases of the
predicate tests rely on, checked without a device.

BASELINE configs[3] (3 replicas, 2 clients, {v1,v2,v3}, limit 3, policy assume_commit_number) was seen by the suite through level totals alone.  What runs only at
ClientCount = 2 — the else branch of ReceivePrepareMsg (VSR.tla:414-421: the executed bit of the OTHER client's row is recomputed), the guard bit of
ReceiveClientRequest per (client, value), the ordinal decoding over clients, log entries with client_id = 2 through every log copy, printer and reader — is
reached state by state on the three harvests of deep_harvest.SPACES_C2 (a deterministic guided walk on the C++ oracle under the policy).  Here:

  * the three harvests are pinned by literals (states, xor of the fingerprints, largest bag, enabled instances per action) and a second run gives the same;
  * the floors hold on the oracle alone, each measured value printed: per counted action >= 500 instances over the three spaces, on (3,2,3,1) >= 800
    ReceivePrepareMsg instances per client that flip the executed bit of a row they did not write, and the act_generated floors of the seeded level;
  * C++ oracle == Python restatement (successor multisets, invariant verdicts, fingerprint against canonical view) on every state of (2,2,1,1) and (2,2,2,1)
    and of levels 1-9 of (3,2,1,1), and on a sample of every harvest (60 states per counted action, 60 per client with a flipped row);
  * under the strict reading both oracles raise exactly on the states with a ReceivePrepareMsg instance;
  * printer and reader keep `clients`, both client-table rows and client_id = 2 inside logs and messages;
  * every two-client predicate of deep_predicates_reference.py takes each verdict on at least 20 sampled items.

Flips, measured by deep_harvest.c2_facts (a changed executed bit of the row of the client whose entry was NOT appended, parent against child by
oracle/pycodec.py): 828 / 838 on (3,2,3,1), 788 / 791 on (3,2,3,2), 128 / 128 on (3,2,2,1); they are exactly the instances that change both rows.
(892 / 903 on (3,2,3,1), quoted when the floor of 800 was set, came from a looser count of the same harvest; only a CHANGED executed bit counts here.)"""
import collections

import numpy as np
import pytest

import deep_harvest as dh
import deep_predicates_reference as dp
from oracle import orc, pycodec, pyoracle as po

SPACES = sorted(dh.SPACES_C2)
IDS = ["%d-%d-%d-%d" % k for k in SPACES]

# (states, xor of the fingerprints, largest bag, enabled instances of action 1 .. 15 in Next order)
PINNED = {
    (3, 2, 2, 1): (6252, 0xc4192d8d830ee91f, 17, [2, 2060, 1899, 783, 5, 612, 181, 5886, 3100, 2358, 2874, 2048, 412, 1022, 640]),
    (3, 2, 3, 1): (18787, 0x9bf0e2677e72cd5b, 22, [2, 8512, 1899, 783, 5, 612, 181, 18630, 6100, 8566, 10529, 7645, 6480, 4371, 2077]),
    (3, 2, 3, 2): (38609, 0x6b77cf284e401042, 22, [31853, 24816, 28460, 17004, 646, 9829, 3521, 26133, 51895, 8179, 10596, 7758, 4586, 3618, 2133]),
}


@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


# ---------------------------------------------------------------------------------------------------------------------
# 1. the harvests
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SPACES, ids=IDS)
def test_harvest_is_the_pinned_one_twice_and_fits_the_layout(key):
    h = dh.space(orc, key)
    assert h.P.arr[5] == 1 and dh.policy(key) == dict(assume_commit_number=True)
    got = h.summary()
    e = h.enabled()
    assert (got["states"], got["fp_xor"], got["max_bag"], [e[a] for a in range(1, 16)]) == PINNED[key]
    assert got["max_bag"] < dh.max_bag_of_layout(h.P) and h.violating_parents == []
    # a second run, past the cache: the same states
    by_fp = {}
    for kind, kw in dh.SPACES_C2[key]:
        again = dh.harvest_vc(orc, dh.params(orc, key), **kw) if kind == "vc" else dh.harvest_st(orc, dh.params(orc, key), frozen=(3,), **kw)
        by_fp.update(zip(again.fps, again.records))
    assert sorted(by_fp) == h.fps and all(np.array_equal(by_fp[f], r) for f, r in zip(h.fps, h.records))


def test_the_five_and_four_replica_spaces_are_what_they_were():
    assert sorted(dh.SPACES) == [(4, 1, 1, 2), (4, 1, 2, 1), (5, 1, 1, 2), (5, 1, 2, 1)] and dh.FLOOR == {5: 1000, 4: 200}
    assert all(dh.policy(k) == {} and dh.expected(k) == dh.EXPECTED[k] for k in dh.SPACES)
    assert dh.params(orc, (4, 1, 2, 1)).arr.tolist() == orc.Params(4, 1, 2, 1).arr.tolist()


def test_the_floors_hold_on_the_oracle_alone():
    total = collections.Counter()
    for key in SPACES:
        total.update(dh.space(orc, key).enabled())
    print("instances per counted action over the three spaces:", {orc.ACTIONS[a]: total[a] for a in dh.COUNTED_C2})
    assert len(dh.COUNTED_C2) == 9
    for a in dh.COUNTED_C2:
        assert total[a] >= dh.FLOOR_C2, (orc.ACTIONS[a], total[a])
    for key in SPACES:
        f = dh.c2_facts(orc, key)
        both_logs, both_requests = dh.c2_state_facts(orc, key)
        print(key, "ReceivePrepareMsg flips a row it did not write: client 1 %d, client 2 %d (in %d / %d states); changes both rows %d; ExecuteOp writes row 1 "
              "%d, row 2 %d; states with a log of both clients %d, with a request of both at replica 1 %d"
              % (f["flips"][1], f["flips"][2], len(f["flip_states"][1]), len(f["flip_states"][2]), f["both_rows"], f["exec_rows"][1], f["exec_rows"][2],
                 both_logs, both_requests))
        assert min(f["flips"].values()) >= 100 and min(f["exec_rows"].values()) >= 500 and both_logs >= 3000 and both_requests >= 2000
        if key == (3, 2, 3, 1):
            assert f["flips"][1] >= dh.FLOOR_C2_FLIPS and f["flips"][2] >= dh.FLOOR_C2_FLIPS, f["flips"]
            e = dh.space(orc, key).enabled()                     # act_generated of a step over the seeded level = the successors per action
            print(key, "act_generated of the seeded level:", {orc.ACTIONS[a]: e[a] for a in sorted(dh.FLOOR_C2_EXPAND)})
            for a, floor in dh.FLOOR_C2_EXPAND.items():
                assert e[a] >= floor, (orc.ACTIONS[a], e[a])


# ---------------------------------------------------------------------------------------------------------------------
# 2. C++ oracle against the Python restatement
# ---------------------------------------------------------------------------------------------------------------------
def _both_oracles_agree(P3, M, w, st):
    """successor multisets (action name, normalised record, verdicts of both invariants), the state's own verdict -> the restatement's successors"""
    psucc = po.successors(M, st)
    cs = sorted((orc.ACTIONS[x["action"]], tuple(pycodec.normalise(M, [int(v) for v in x["words"]])), orc.invariants(P3, x["words"])) for x in orc.successors(P3, w))
    ps = sorted((n, tuple(pycodec.normalise(M, pycodec.pack(M, t))),
                 (0 if po.AcknowledgedWriteNotLost(M, t) else 1) | (0 if po.AcknowledgedWritesExistOnMajority(M, t) else 2)) for n, t in psucc)
    assert cs == ps
    assert orc.invariants(P3, w) == (0 if po.AcknowledgedWriteNotLost(M, st) else 1) | (0 if po.AcknowledgedWritesExistOnMajority(M, st) else 2)
    return psucc


@pytest.mark.parametrize("key, levels, total, depth", [((2, 2, 1, 1), 99, 139, 14), ((2, 2, 2, 1), 99, 973, 18), ((3, 2, 1, 1), 9, 3768, 9)],
                         ids=["2-2-1-1", "2-2-2-1", "3-2-1-1-levels-1-9"])
def test_both_oracles_agree_on_every_state_of_a_two_client_space(key, levels, total, depth):
    """the shape of test_successor_sets_agree_on_every_state_of_a_small_space; the states are enumerated by the restatement's own successors, level by level,
    and the level sizes are the C++ BFS's"""
    M = po.Model(key[0], key[1], tuple("v%d" % (i + 1) for i in range(key[2])), key[3], assume_commit_number=True)
    P = orc.Params(*key, assume_commit_number=True)
    P3 = orc.Params(*key, assume_commit_number=True, invariant_mask=3)
    s0 = po.Init(M)
    level, seen, fp_of_view, sizes = [(s0, po.canonical_view(M, s0))], set(), {}, []
    seen.add(level[0][1])
    actions = collections.Counter()
    while level and len(sizes) < levels:
        sizes.append(len(level))
        nxt = []
        for st, cv in level:
            w = np.array(pycodec.pack(M, st), dtype=np.uint64)
            assert fp_of_view.setdefault(cv, orc.fingerprint(P, w)[0]) == orc.fingerprint(P, w)[0]
            for name, t in _both_oracles_agree(P3, M, w, st):
                actions[name] += 1
                cvt = po.canonical_view(M, t)
                if cvt not in seen:
                    seen.add(cvt)
                    nxt.append((t, cvt))
        level = nxt
    b = orc.Bfs(P)
    cpp = [1]
    while len(cpp) < len(sizes) and b.step():
        cpp.append(b.info["n_new"])
    b.close()
    print(key, "levels", len(sizes), "states", sum(sizes), dict(actions))
    assert sizes == cpp and (sum(sizes), len(sizes)) == (total, depth)
    assert len(set(fp_of_view.values())) == len(fp_of_view) == total  # the fingerprint separates exactly what the canonical view separates
    assert actions["ReceivePrepareMsg"] > 0 and actions["ReceiveClientRequest"] > 0


@pytest.mark.parametrize("key", SPACES, ids=IDS)
def test_both_oracles_agree_on_a_sample_of_every_harvest(key):
    h = dh.space(orc, key)
    M = dh.py_model(key)
    P3 = dh.params(orc, key, invariant_mask=3)
    sample, taken = dh.c2_py_sample(orc, key)
    print(key, len(sample), "states:", {(orc.ACTIONS[k] if isinstance(k, int) else "flips client %d" % k[1]): v for k, v in taken.items()})
    for a in dh.COUNTED_C2:
        assert taken[a] == min(60, sum(1 for i in range(len(h)) if a in h.actions(i)))      # (ReceiveHigherDVC at L = 1: 5 instances in 4 states)
    assert taken[("flip", 1)] == taken[("flip", 2)] == 60
    checked = collections.Counter()
    for i in sample:
        w = h.records[i]
        st = pycodec.unpack(M, [int(x) for x in w])
        assert pycodec.normalise(M, pycodec.pack(M, st)) == pycodec.normalise(M, [int(x) for x in w])
        _both_oracles_agree(P3, M, w, st)
        checked.update(set(h.actions(i)))
    for a in dh.COUNTED_C2:
        assert checked[a] >= taken[a]


def test_the_strict_reading_raises_exactly_where_a_prepare_is_received():
    """(3,2,2,1), every harvested state.  At ClientCount = 2 the loop of VSR.tla:414-421 always meets the other client, whose row reads `m.commit`."""
    key = (3, 2, 2, 1)
    h = dh.space(orc, key)
    strict, M = orc.Params(*key), po.Model(3, 2, ("v1", "v2"), 1)
    raised = 0
    for i in range(len(h)):
        has = dh.A_ReceivePrepareMsg in h.actions(i)
        try:
            got = orc.successors(strict, h.records[i])
            assert not has and bytes(x["action"] for x in got) == h.actions(i), i
        except orc.OracleError as e:
            assert has and "VSR.tla:421" in str(e), (i, str(e))
            raised += 1
        st = pycodec.unpack(M, [int(x) for x in h.records[i]])
        try:
            list(po.ReceivePrepareMsg(M, st))
            assert not has, i
        except po.EvalError:
            assert has, i
    print("strict reading: raised on %d of %d states" % (raised, len(h)))
    assert raised >= 1000 and len(h) - raised >= 1000


# ---------------------------------------------------------------------------------------------------------------------
# 3. printer and reader
# ---------------------------------------------------------------------------------------------------------------------
def test_printer_and_reader_keep_both_clients(vt):
    from oracle import tlcprint, tlcvalue
    key = (3, 2, 3, 1)
    h = dh.space(orc, key)
    M = dh.py_model(key)
    m = dh.product_model(vt, key)
    fixed = int(m.layout.fixed_words)
    idx = [(k * len(h)) // 500 for k in range(500)]
    n_both = n_log2 = n_msg2 = 0
    for i in idx:
        rec = h.records[i]
        st = pycodec.unpack(M, [int(x) for x in rec])
        both = any(len(set(dict(e)["client_id"] for e in lg)) == 2 for lg in st["rep_log"])
        n_both += both
        # the product's printer, then its trace reader: the same record (the reader returns the bag sorted)
        text = m.format_state(rec)
        back = m.parse_states(text)
        want = np.array(rec, dtype=np.uint64)
        want[fixed:] = np.sort(want[fixed:])
        assert len(back) == 1 and np.array_equal(back[0][1], want), i
        assert "clients |-> 1..2" in text
        rows = text.split("rep_client_table |-> ", 1)[1].split("\n", 1)[0]
        assert rows.count("request_number |-> ") == 2 * key[0], rows
        log_line = text.split("rep_log |-> ", 1)[1].split("\n", 1)[0]
        msg_line = text.split("messages |-> ", 1)[1].split("\n", 1)[0]
        assert both == ("client_id |-> 1" in log_line and "client_id |-> 2" in log_line), i
        n_log2 += "client_id |-> 2" in log_line
        n_msg2 += "client_id |-> 2" in msg_line
        # the product's text through the independent value parser: the Python state
        val = dict(tlcvalue.parse_value(text))
        assert po.canon(val["clients"]) == po.canon(st["clients"]) and po.canon(val["rep_client_table"]) == po.canon(st["rep_client_table"])
        assert po.canon(val["rep_log"]) == po.canon(st["rep_log"]), i
        # the independent printer, then the independent parser: the same Python state
        for var in po.VIEW_VARS + po.AUX_VARS + ["clients"]:
            got = tlcvalue.parse_value(tlcprint.fmt(st[var]))
            if got == () and st[var] == {}:                       # TLC prints the empty function as <<>>
                continue
            assert po.canon(got) == po.canon(st[var]), (i, var)
    m.close()
    print("printer and reader: %d states, %d with a log of both clients, client_id = 2 in a log of %d and in a message of %d" % (len(idx), n_both, n_log2, n_msg2))
    assert len(set(idx)) == 500 and n_both >= 250 and n_log2 >= 250 and n_msg2 >= 250


# ---------------------------------------------------------------------------------------------------------------------
# 4. the two-client predicates, by the compiler and the reference alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(3, 2, 3, 1), (3, 2, 2, 1)], ids=["3-2-3-1", "3-2-2-1"])
def test_every_two_client_predicate_compiles_and_takes_both_verdicts_twenty_times(vt, key):
    """the sample of the GPU leg (test_deep_predicates_gpu.py): 1 500 states; 150 parents — an even stride of 75 and 75 of the states in which ReceivePrepareMsg
    flips a row it did not write — with all their successors.  ExecutedRisesOnlyOnExecuteOp stands for "the executed bit rises only on ExecuteOp or
    ReceivePrepareMsg", which is true on every pair (deep_predicates_reference.executed_rises_only_on_execute_op says so with figures)."""
    h = dh.space(orc, key)
    PM = dh.py_model(key)
    m = dh.product_model(vt, key)
    for preds, step in ((dp.STATE_C2, False), (dp.STEP_C2, True)):
        w = (m.compile_step if step else m.compile_where)(dp.text_of(preds))
        d = w.describe()
        assert w.names == [p[0] for p in preds] and d["step"] is step and 0 < d["n_ops"] <= 4096 and 0 < d["depth"] <= 32, d
    assert dp.state_sets(key)[-1] == ("C2", dp.STATE_C2) and dp.step_sets(key)[-1] == ("C2", dp.STEP_C2)
    assert dp.state_sets((5, 1, 2, 1))[-1] == ("R4", dp.STATE) and dp.step_sets((4, 1, 1, 2))[-1] == ("R4", dp.STEP)
    m.close()
    flips = dh.c2_facts(orc, key)["flip_states"]
    si, pi = dp.state_indices(len(h)), dp.c2_parent_indices(len(h), flips[1] + flips[2])
    assert len(set(si)) == dp.N_STATES and len(set(pi)) == dp.N_PARENTS and len(set(pi) & set(flips[1] + flips[2])) >= dp.N_C2_FLIP_PARENTS
    states = [pycodec.unpack(PM, [int(x) for x in h.records[i]]) for i in si]
    pairs = []
    for i in pi:
        p = pycodec.unpack(PM, [int(x) for x in h.records[i]])
        pairs.extend((p, pycodec.unpack(PM, [int(x) for x in s["words"]]), orc.ACTIONS[s["action"]]) for s in h.successors(i))
    n_state = {name: sum(bool(f(s)) for s in states) for name, _t, f in dp.STATE_C2}
    n_step = {name: sum(bool(f(p, c, a)) for p, c, a in pairs) for name, _t, f in dp.STEP_C2}
    print(key, "true on: of %d states %s; of %d pairs %s" % (len(states), n_state, len(pairs), n_step))
    for name, k in n_state.items():
        assert dp.BOTH_VERDICTS <= k <= len(states) - dp.BOTH_VERDICTS, (name, k)
    for name, k in n_step.items():
        assert dp.BOTH_VERDICTS <= k <= len(pairs) - dp.BOTH_VERDICTS, (name, k)
    # the property the replaced predicate stands for holds on every sampled pair, and the bit does rise
    rose = collections.Counter(a for p, c, a in pairs if dp.executed_rose(p, c, a))
    assert set(rose) == {"ExecuteOp", "ReceivePrepareMsg"} and min(rose.values()) >= dp.BOTH_VERDICTS, rose
