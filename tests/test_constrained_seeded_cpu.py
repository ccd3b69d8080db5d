"""The constrained level step on harvested states, CPU leg (`-m "not gpu"`): what test_constrained_seeded_gpu.py relies on, checked without a device.

k_constrain, k_step_expand, k_step_keep and the gated trace decide what a search contains, and before these tests met five replicas and two clients only seven levels from
Init under the constraint TRUE.  The GPU leg runs them on the 1500-state sample of the harvest (tests/deep_harvest.py) of (5,1,2,1), (4,1,2,1) and (3,2,3,1), with
constraints that read what exists only at R >= 4 or at C = 2, against tests/constrained_seeded_reference.py.  Here, by the compiler and the reference alone:

  * every program of the GPU leg compiles for its space, exports what the reference says, and puts the constraint where the reference says (not at bit 0 everywhere);
  * the reference yields at least half of every measured figure (constrained_seeded_reference.MEASURED: transitions blocked, states pruned, states rescued, seeds
    whose instances are all blocked, violating successors on either side of a constraint), rescued >= 10 on every level-2 row, no deadlock, no fingerprint under two
    auxkeys among the permitted producers of level 2 and of level 3, and a further export that holds on some pruned state;
  * with TRUE / TRUE the reference's level 2 is the plain image of the seeds as deep_seeded_worker.Case computes it;
  * no parent of the five-replica steps has more than 64 instances (a list of VSRMC_ACTION_LIST_CAP=64 entries can hold every single parent)."""
import pytest

import constrained_seeded_reference as cs
import where_reference as wr
from deep_seeded_worker import Case
from oracle import orc

MAX_OPS, MAX_DEPTH = 4096, 32


@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


@pytest.fixture(scope="module")
def refs():
    """key -> dict(sp, a, d, e, c2, c3): the reference's steps of the GPU leg's cases, computed once per space, never changed"""
    cache = {}

    def get(key):
        if key not in cache:
            sp = cs.Space(orc, key)
            pr = cs.PROGRAMS[key]
            seeds, earlier = sp.seeds(), set(sp.fps)
            c2, c3, _parents3 = cs.two_levels(sp, pr["action"], pr["state"])
            cache[key] = dict(sp=sp, c2=c2, c3=c3, a=cs.step(sp, seeds, earlier, pr["action"], None, 3, seeds=True),
                              d=cs.step(sp, seeds, earlier, pr["second"], None, 3, seeds=True),
                              e=cs.step(sp, seeds, earlier, pr["action"], pr["e_state"], 3, seeds=True) if pr["e_state"] else None)
        return cache[key]
    return get


@pytest.mark.parametrize("key", cs.SPACES, ids=cs.IDS)
def test_the_programs_compile_and_export_what_the_reference_says(vt, key):
    R, C_, n, L = key
    sp_policy = dict(assume_commit_number=True) if C_ == 2 else {}
    m = vt.Model.from_constants(R=R, C_=C_, n=n, L=L, invariant_mask=3, **sp_policy)
    pr = cs.PROGRAMS[key]
    ks = []
    for tag, step in (("action", True), ("second", True), ("state", False), ("e_state", False)):
        prog = pr[tag]
        if prog is None:
            continue
        w = (m.compile_step_predicates if step else m.compile_predicates)(wr.text_of(prog["preds"]))
        d = w.describe()
        assert w.names == [p[0] for p in prog["preds"]] and d["step"] is step and w.names[prog["k"]] == prog["name"]
        assert 3 <= len(w.names) <= 8 and 0 < d["n_ops"] <= MAX_OPS and 0 < d["depth"] <= MAX_DEPTH, (tag, d)
        if prog["name"].startswith("Not"):                            # a negation is written in the text and as `not f(..)`
            assert prog["preds"][prog["k"]][1].startswith("~(")
        ks.append(prog["k"])
    assert any(k > 0 for k in ks), "the constraint is bit 0 of every program: k_bit is never non-zero"
    w = m.compile_step_predicates(wr.text_of(pr["step_set"]))
    assert len(w.names) == len(pr["step_set"])
    m.close()


@pytest.mark.parametrize("key", cs.SPACES, ids=cs.IDS)
def test_the_reference_keeps_the_measured_figures(refs, key):
    r = refs(key)
    want = cs.MEASURED[key]
    c2, c3, a, d, e = r["c2"], r["c3"], r["a"], r["d"], r["e"]
    got = dict(level2=cs.figures(c2), level3=cs.figures(c3),
               second=dict(blocked=d.blocked, blocked_actions=len(d.blocked_act), rescued=len(d.rescued)), all_blocked=c2.live_blocked,
               viol_blocked=a.blocked_violating, viol_new=len(a.viol), viol_new_second=len(d.viol),
               viol_pruned=len([f for f in e.viol if f in set(e.pruned)]) if e else 0)
    print(key, got)
    for row in ("level2", "level3", "second"):
        for what, floor in cs.floors(want[row]).items():
            assert got[row][what] >= floor, (key, row, what, got[row][what], floor)
    assert got["level2"]["rescued"] >= 10 and got["second"]["rescued"] >= 10 and len(a.rescued) >= 10
    assert got["all_blocked"] >= (want["all_blocked"] + 1) // 2
    for what in ("viol_blocked", "viol_new", "viol_new_second", "viol_pruned"):      # every one that was measured: at least one
        assert got[what] >= (1 if want[what] else 0), (key, what, got[what])
    assert a.blocked_violating + len(a.viol) == d.blocked_violating + len(d.viol) > 0      # the same violating successors, on one side or the other
    for st in (c2, c3, a, d) + ((e,) if e else ()):
        assert not st.ties                                            # no fingerprint under two auxkeys among the permitted producers
        assert st.deadlocks == 0 or st is c3                          # no seed is terminal, however many have every instance blocked (a kept level-2 state may be)
    # the action constraint alone and with the state constraint: the same gate (the state constraint does not change what is generated, blocked or new)
    assert (a.generated, a.blocked, a.new, a.rescued) == (c2.generated, c2.blocked, c2.new, c2.rescued)
    assert sorted(c2.kept + c2.pruned) == c2.new and c2.pruned and c3.parents == len(c2.kept)
    # a further export counts something among the pruned states; the constraint itself holds on none of them
    for st, prog in ((c2, cs.PROGRAMS[key]["state"]),) + (((e, cs.PROGRAMS[key]["e_state"]),) if e else ()):
        assert st.pruned_count[prog["name"]] == 0 and st.pruned_min_fp_k[prog["name"]] is None
        assert any(n > 0 for nm, n in st.pruned_count.items() if nm != prog["name"])
    if key[0] == 5:
        assert max(c2.max_instances, c3.max_instances) <= 64, "a single parent overflows a list of 64 entries: VSRMC_ACTION_LIST_CAP=64 cannot run"


@pytest.mark.parametrize("key", cs.SPACES, ids=cs.IDS)
def test_true_true_is_the_plain_image_of_the_seeds(refs, key):
    sp = refs(key)["sp"]
    st = cs.step(sp, sp.seeds(), set(sp.fps), cs.TRUE_STEP, cs.TRUE_STATE, 1, seeds=True)
    case = Case(orc, key, sp.recs, [orc.successors(sp.P, r) for r in sp.recs], policy=sp.policy)
    assert not case.ties                                              # the whole sample is one single-pass level
    assert (st.new, st.generated, st.act) == (case.new, case.generated, case.act)
    assert st.kept == st.new and not st.pruned and st.blocked == 0 and not st.rescued and st.deadlocks == len(case.deadlocks)
    assert st.kept_words == case.new_words_dev and sum(len(r) + sp.perms for r in sp.recs) == case.seed_words_dev
    for f in st.new[:: max(1, len(st.new) // 200)]:                    # ... and the producers are Case's
        assert sorted((ak, i) for ak, i, _s, _a in st.producers[f]) == sorted((ak, i) for ak, i, _s in case.by_fp[f])
