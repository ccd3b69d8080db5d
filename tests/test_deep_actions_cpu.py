"""The action bodies deep in the view-change and state-transfer protocol at FIVE and FOUR replicas, CPU leg (`-m "not gpu"`).

Every per-state successor comparison elsewhere in the suite is at three replicas or fewer, and a BFS from Init reaches none of SendSV's successors
at R = 5 within any depth a test can afford (tests/deep_harvest.py says why).  Here the states are steered to (deep_harvest: a deterministic guided
walk on the C++ oracle) and

  * the harvest is pinned (tests/golden/deep_harvest_summary.json: state count, xor of the fingerprints, largest bag per space — numbers only),
    every bag below the device layout's capacity, so that the HIP path can take every one of them;
  * the C++ oracle is checked against itself on EVERY harvested state (a successor's fingerprint, auxkey and verdict as computed along the
    successor equal those of the finished record) and the instances per counted action reach the floors: >= 1000 at R = 5, >= 200 at R = 4;
  * on a sample of at least 60 states per enabled action and space the successor multiset (action name, normalised record, invariant verdict)
    equals those of the independent Python restatement (oracle/pyoracle.py, about 30 ms per state).
"""
import collections
import json
import os

import numpy as np
import pytest

import deep_harvest as dh
from oracle import orc, pycodec, pyoracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deep_harvest_summary.json")
SPACES = sorted(dh.SPACES)


@pytest.mark.parametrize("key", SPACES, ids=lambda k: "%d-%d-%d-%d" % k)
def test_harvest_is_the_pinned_one_and_fits_the_layout(key):
    h = dh.space(orc, key)
    with open(GOLDEN) as f:
        want = json.load(f)[",".join(str(x) for x in key)]
    got = h.summary()
    assert (got["states"], "%016x" % got["fp_xor"], got["max_bag"]) == (want["states"], want["fp_xor"], want["max_bag"])
    assert got["max_bag"] < dh.max_bag_of_layout(h.P)                 # (a successor adds at most R - 1 entries)
    assert got["states"] >= 4096
    e = h.enabled()
    for a in dh.EXPECTED[key]:
        assert e[a] >= 60, (orc.ACTIONS[a], e[a])


def test_cpp_oracle_is_self_consistent_on_every_harvested_state_and_the_floors_hold():
    inst = {4: collections.Counter(), 5: collections.Counter()}
    for key in SPACES:
        h = dh.space(orc, key)
        for i in range(len(h)):
            fp, _ak = orc.fingerprint(h.P, h.records[i])
            assert fp == h.fps[i] and orc.invariants(h.P, h.records[i]) == 0
            for s in h.successors(i):
                assert orc.fingerprint(h.P, s["words"]) == (s["fp"], s["auxkey"]), (key, i, orc.ACTIONS[s["action"]])
                assert orc.invariants(h.P, s["words"]) == s["inv"], (key, i, orc.ACTIONS[s["action"]])
                inst[key[0]][s["action"]] += 1
    print({R: {orc.ACTIONS[a]: inst[R][a] for a in dh.COUNTED} for R in inst})
    for R in inst:
        for a in dh.COUNTED:
            assert inst[R][a] >= dh.FLOOR[R], (R, orc.ACTIONS[a], inst[R][a])


SAMPLE = 150                                                          # states per enabled action and space (the issue's floor: 60)


@pytest.mark.parametrize("key", SPACES, ids=lambda k: "%d-%d-%d-%d" % k)
def test_cpp_oracle_equals_the_python_restatement_on_a_sample(key):
    """successor multisets with BOTH invariants' verdicts (mask 3: AcknowledgedWriteNotLost, VSR.tla:945-950, and
    AcknowledgedWritesExistOnMajority, :937-943).  Under mask 1 no harvested image violates (the walk drops such successors and found none), so
    the parents of every successor that violates mask 3 are added to the sample: in the two-value spaces the verdict False is compared too."""
    h = dh.space(orc, key)
    P3 = orc.Params(*key, invariant_mask=3)
    M = po.Model(key[0], key[1], tuple("v%d" % (i + 1) for i in range(key[2])), key[3])
    states_of = collections.defaultdict(list)
    sample = set()
    for i in range(len(h)):
        for a in set(h.actions(i)):
            states_of[a].append(i)
    for a, idx in states_of.items():
        k = min(SAMPLE, len(idx))
        sample.update(idx[(j * len(idx)) // k] for j in range(k))
    if key[2] == 2:                                                   # (one value: no operation ever reaches a log in these walks, nothing is acknowledged)
        for i in range(len(h)):
            if any(orc.invariants(P3, s["words"]) for s in h.successors(i)):
                sample.add(i)
    checked = collections.Counter()
    n_false = 0
    for i in sorted(sample):
        w = h.records[i]
        st = pycodec.unpack(M, [int(x) for x in w])
        assert pycodec.normalise(M, pycodec.pack(M, st)) == pycodec.normalise(M, [int(x) for x in w])      # the codec round trip at this R
        osucc = h.successors(i)
        cs = sorted((orc.ACTIONS[x["action"]], tuple(pycodec.normalise(M, [int(v) for v in x["words"]])), orc.invariants(P3, x["words"])) for x in osucc)
        ps = sorted((n, tuple(pycodec.normalise(M, pycodec.pack(M, t))),
                     (0 if po.AcknowledgedWriteNotLost(M, t) else 1) | (0 if po.AcknowledgedWritesExistOnMajority(M, t) else 2))
                    for n, t in po.successors(M, st))
        assert cs == ps, (key, i)
        assert all((x["inv"] != 0) == bool(orc.invariants(P3, x["words"]) & 1) for x in osucc)
        n_false += sum(1 for _n, _r, v in cs if v)
        assert (orc.invariants(h.P, w) == 0) == po.AcknowledgedWriteNotLost(M, st)
        for a in set(h.actions(i)):
            checked[a] += 1
    print(key, len(sample), "violating successors compared:", n_false, {orc.ACTIONS[a]: checked[a] for a in sorted(checked)})
    for a in dh.EXPECTED[key]:
        assert checked[a] >= 60, (orc.ACTIONS[a], checked[a])
    if key[2] == 2:
        assert n_false >= 100, n_false
    assert np.all([len(h.records[i]) == h.P.fixed_words() + dh.bag_size(h.records[i]) for i in sample])


@pytest.mark.parametrize("R", [5, 4])
def test_hand_built_view_change_and_state_transfer_records_on_both_oracles(R):
    """HighestLog's CHOOSE at a quorum of three (VSR.tla:716-722), HighestCommitNumber (:729-733), state transfer with lagging replicas and SendOnce
    (:496-516, :250-252): the C++ oracle and the Python restatement agree, and what SendSV installs is asserted by value (deep_harvest.hand_built)."""
    key = (R, 1, 2, 1)
    P = orc.Params(*key)
    M = po.Model(R, 1, ("v1", "v2"), 1)
    states, checks = dh.hand_built(R)
    succ = []
    for i, st in enumerate(states):
        w = np.array(pycodec.pack(M, st), dtype=np.uint64)
        assert len(w) <= P.fixed_words() + dh.max_bag_of_layout(P)
        osucc = orc.successors(P, w)
        cs = sorted((orc.ACTIONS[x["action"]], tuple(pycodec.normalise(M, [int(v) for v in x["words"]])), x["inv"] == 0) for x in osucc)
        ps = sorted((n, tuple(pycodec.normalise(M, pycodec.pack(M, t))), bool(po.AcknowledgedWriteNotLost(M, t))) for n, t in po.successors(M, st))
        assert cs == ps, (R, i)
        succ.append([(orc.ACTIONS[x["action"]], pycodec.unpack(M, [int(v) for v in x["words"]])) for x in osucc])
    for k, chk in checks:
        chk(succ[k])
    assert sum(1 for ss in succ for a, _t in ss if a == "SendSV") >= 9
