"""The predicate kernels at FIVE and FOUR replicas, CPU leg (`-m "not gpu"`): what test_deep_predicates_gpu.py relies on, checked without a device.

k_where, k_step_list / k_step_apply and k_simulate_where were never run on a record of more than three replicas; the GPU leg runs them on a deterministic
sample of the harvest of tests/deep_harvest.py (deep_predicates_reference.py: state_indices, parent_indices).  Here, by the compiler and the reference alone:

  * every predicate set the GPU leg uses compiles at the four spaces, below the caps of 4096 ops and depth 32;
  * the existing sets take the verdicts they are known to take over the union of the four samples (a predicate that is constant there pins nothing);
  * every predicate of the R >= 4 sets takes both verdicts at R = 5 and at R = 4;
  * the sample holds what makes it a test of the R >= 4 paths — states that hold a DoViewChange from source 4 or 5, bags above 32 messages, pairs whose
    successor changes the fourth word of a replica block, pairs that append R - 1 bag entries — at or above half of the measured figures
    (deep_predicates_reference.MEASURED);
  * NewKeyForLast, written over the fields the language reads, is true exactly on the pairs whose successor's bag holds a key for ReplicaCount that the
    parent's does not."""
import collections

import pytest

import deep_harvest as dh
import deep_predicates_reference as dp
import step_reference as sr
import where_reference as wr
from oracle import orc, pycodec, pyoracle as po

SPACES = sorted(dh.SPACES)
IDS = ["%d-%d-%d-%d" % k for k in SPACES]
MAX_OPS, MAX_DEPTH = 4096, 32


@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


def _pm(key):
    return po.Model(key[0], key[1], tuple("v%d" % (i + 1) for i in range(key[2])), key[3])


@pytest.fixture(scope="module")
def samples():
    """key -> (sampled states, pairs (parent, child, action name) of the sampled parents) as Python views; computed once, never changed"""
    out = {}
    for key in SPACES:
        h = dh.space(orc, key)
        PM = _pm(key)
        states = [pycodec.unpack(PM, [int(x) for x in h.records[i]]) for i in dp.state_indices(len(h))]
        assert len(set(dp.state_indices(len(h)))) == dp.N_STATES and set(dp.parent_indices(len(h))) <= set(dp.state_indices(len(h)))
        pairs = []
        for i in dp.parent_indices(len(h)):
            p = pycodec.unpack(PM, [int(x) for x in h.records[i]])
            pairs.extend((p, pycodec.unpack(PM, [int(x) for x in s["words"]]), orc.ACTIONS[s["action"]]) for s in h.successors(i))
        out[key] = (states, pairs)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. the sets compile under the caps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SPACES, ids=IDS)
def test_every_set_compiles_below_the_caps(vt, key):
    R, C_, n, L = key
    m = vt.Model.from_constants(R=R, C_=C_, n=n, L=L)
    sizes = {}
    for tag, preds, step in (("wr.SET_A", wr.SET_A, False), ("wr.set_b", wr.set_b(L), False), ("dp.STATE", dp.STATE, False), ("sr.SET_A", sr.SET_A, True),
                             ("sr.SET_B", sr.SET_B, True), ("sr.SET_C", sr.SET_C, True), ("dp.STEP", dp.STEP, True)):
        assert len(preds) <= 8
        w = (m.compile_step if step else m.compile_where)(dp.text_of(preds))
        d = w.describe()
        assert w.names == [p[0] for p in preds] and d["step"] is step
        assert 0 < d["n_ops"] <= MAX_OPS and 0 < d["depth"] <= MAX_DEPTH, (tag, d)
        sizes[tag] = (d["n_ops"], d["depth"], d["msg_loops"])
    print(key, sizes)
    assert sizes["dp.STATE"][2] >= 1 and sizes["dp.STEP"][2] == 2      # MsgTail's loop; NewKeyForLast's two loops, one over each bag
    # the random expressions of the GPU leg (the same seed): every one compiles at this R
    for j, (text, _f) in enumerate(wr.random_predicates(20261017, R, 100)):
        d = m.compile_where(text).describe()
        assert d["n_ops"] <= MAX_OPS and d["depth"] <= MAX_DEPTH, (j, text)
    m.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. verdicts over the samples, by the reference alone
# ---------------------------------------------------------------------------------------------------------------------
def _state_verdicts(samples, preds_of, keys=SPACES):
    seen = collections.defaultdict(set)
    for key in keys:
        for name, _t, f in preds_of(key):
            seen[name].update(bool(f(s)) for s in samples[key][0])
    return seen


def _step_verdicts(samples, preds, keys=SPACES):
    seen = collections.defaultdict(set)
    for key in keys:
        for name, _t, f in preds:
            seen[name].update(bool(f(p, c, a)) for p, c, a in samples[key][1])
    return seen


def test_existing_sets_take_the_known_verdicts_over_the_union(samples):
    both = {True, False}
    a = _state_verdicts(samples, lambda key: wr.SET_A)
    assert a.pop("LogDivergence") == {False} and all(v == both for v in a.values()), a
    b = _state_verdicts(samples, lambda key: wr.set_b(key[3]))
    assert b.pop("SameTypeTwoSources") == {True} and b.pop("AllDelivered") == {False} and all(v == both for v in b.values()), b
    sa = _step_verdicts(samples, sr.SET_A)
    assert sa.pop("Delivered") == {True} and all(v == both for v in sa.values()), sa
    sb = _step_verdicts(samples, sr.SET_B)
    assert sb.pop("ViewMonotonic") == {True} and all(v == both for v in sb.values()), sb
    sc = _step_verdicts(samples, sr.SET_C)
    assert sc.pop("SendShrinks") == {False} and all(v == both for v in sc.values()), sc
    # the two properties that fail: CommitMonotonic on 5 pairs, CommittedPrefixStable on 1, all at (4,1,2,1)
    false_on = {key: (sum(1 for p, c, act in samples[key][1] if not sr.commit_monotonic(p, c, act)),
                      sum(1 for p, c, act in samples[key][1] if not sr.committed_prefix_stable(p, c, act))) for key in SPACES}
    print("CommitMonotonic / CommittedPrefixStable false on:", false_on)
    assert false_on == {(4, 1, 1, 2): (0, 0), (4, 1, 2, 1): (5, 1), (5, 1, 1, 2): (0, 0), (5, 1, 2, 1): (0, 0)}


@pytest.mark.parametrize("R", [5, 4])
def test_every_r4_predicate_takes_both_verdicts_at_this_replica_count(samples, R):
    keys = [k for k in SPACES if k[0] == R]
    st = _state_verdicts(samples, lambda key: dp.STATE, keys)
    sp = _step_verdicts(samples, dp.STEP, keys)
    for name, _t, _f in dp.STATE:
        assert st[name] == {True, False}, (R, name, st[name])
    for name, _t, _f in dp.STEP:
        assert sp[name] == {True, False}, (R, name, sp[name])
    counts = {key: ({nm: sum(bool(f(s)) for s in samples[key][0]) for nm, _t, f in dp.STATE},
                    {nm: sum(bool(f(p, c, a)) for p, c, a in samples[key][1]) for nm, _t, f in dp.STEP}, len(samples[key][1])) for key in keys}
    print(counts)


@pytest.mark.parametrize("key", SPACES, ids=IDS)
def test_the_sample_holds_what_only_exists_at_four_and_five_replicas(samples, key):
    states, pairs = samples[key]
    R = key[0]
    got = dict(dvc45=sum(1 for s in states if dp.holds_dvc_from_4_or_5(s)), bag33=sum(1 for s in states if len(s["messages"]) > 32),
               word3=sum(1 for p, c, _a in pairs if dp.fourth_word_changes(p, c)), bcast=sum(1 for p, c, _a in pairs if dp.appended(p, c) == R - 1))
    most = max(dp.n_dvc(s, r) for s in states for r in dp.reps(s))
    print(key, "states", len(states), "pairs", len(pairs), got, "most DoViewChanges held by one replica", most,
          "growth", sorted(collections.Counter(dp.appended(p, c) for p, c, _a in pairs).items()))
    assert len(states) == dp.N_STATES
    for what, floor in dp.floors(key).items():
        assert got[what] >= floor, (key, what, got[what], floor)
    assert most >= R - 1
    assert all(dp.appended(p, c) in (0, 1, R - 1) for p, c, _a in pairs)


def test_new_key_for_last_is_exactly_a_new_key_for_the_last_replica(samples):
    n = collections.Counter()
    for key in SPACES:
        for p, c, a in samples[key][1]:
            v = dp.new_key_for_last(p, c, a)
            assert v == dp.new_key_for_last_by_keys(p, c), (key, a)
            n[(key[0], v)] += 1
    for R in (5, 4):                                                    # ... the hand-built records' successors included
        PM = _pm((R, 1, 2, 1))
        for st in dh.hand_built(R)[0]:
            for a, c in po.successors(PM, st):
                v = dp.new_key_for_last(st, c, a)
                assert v == dp.new_key_for_last_by_keys(st, c), (R, a)
                n[(R, v)] += 1
    print(dict(n))
    assert all(n[(R, v)] > 0 for R in (5, 4) for v in (True, False))
