"""State constraints on the levels beyond the record buffers (`-m gpu`): k_constrain_slice through ModelChecker.constrain(.., deep=True) / deepen / advance /
run / check / constraint_results / constraint_deep_results / constraint_pruned and the CLI's -deepConstraint, against tests/constraint_reference.py — the
Python BFS over the CPU oracles' successor function with the constraint as a hand-written Python function.  A reference is computed once per space and
shared; every test compares per level, so a slice that escaped the filter anywhere changes a figure (levels 2 .. 23 of the main space all prune)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import constraint_reference as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
SIZES = dict(table_log2=20, frontier_words=1 << 22, frontier_states=1 << 17, pending_entries=1 << 17)
SMALL = dict(frontier_words=1 << 15, frontier_states=1 << 12)          # the buffers of test_constraint_gpu.py's out-of-room test
# the main space of the issue: (3,1,{v1,v2},1) under Replica3Normal
KEPT = [1, 2, 4, 8, 14, 21, 29, 40, 56, 72, 92, 119, 159, 211, 277, 361, 473, 588, 654, 632, 515, 339, 178, 66, 13]
PRUNED = [0, 1, 2, 5, 11, 21, 33, 48, 68, 93, 117, 145, 179, 214, 227, 212, 176, 136, 100, 68, 36, 12, 2, 0, 0]
# key -> (model, R, C, n, L, constraint name, Python constraint, level cap)
CASES = {
    "main": ("first", 3, 1, 2, 1, "Replica3Normal", cr.replica3_normal, None),
    "commit": ("first", 3, 1, 2, 1, "R3NormalCommitBelow2", cr.r3normal_commit_below2, 19),
    "nost-second": ("second", 3, 0, 2, 1, "NoStateTransfer", cr.no_state_transfer, 12),
}


@pytest.fixture(scope="module")
def vt():
    import vsr_tlaplus_amd as vt
    assert vt.load().vsrmc_device_count() >= 1, "no HIP device visible"
    return vt


@pytest.fixture(scope="module")
def refs():
    """key -> the reference's Result: computed once, shared, never changed"""
    cache = {}

    def get(key):
        if key not in cache:
            which, R, C, n, L, _name, fn, cap = CASES[key]
            cache[key] = cr.constrained_bfs(which, R, C, n, L, fn, max_levels=cap, with_unconstrained=False)
        return cache[key]
    return get


def _model(vt, key, **kw):
    which, R, C, n, L = CASES[key][:5]
    if which == "first":
        return vt.Model.from_constants(R=R, C_=C, n=n, L=L, **kw)
    return (vt.Model.second_model if which == "second" else vt.Model.third_model)(R=R, n=n, L=L)


def _checker(vt, key, deep=True, model_kw=None, **kw):
    m = _model(vt, key, **(model_kw or {}))
    mc = vt.ModelChecker(m, device=0, **dict(SIZES, **kw))
    w = m.compile_predicates(cr.TEXTS[CASES[key][5]])
    mc.constrain(w, deep=deep)
    return m, mc, w


def _check_level(mc, lv, lists=True, capped=None):
    """the recorded figures of level lv.level against the reference's level"""
    ci = mc.constraint_results(lv.level)
    x, s = cr.xor_sum(lv.kept)
    assert (ci["kept"], ci["pruned"], ci["n_states"]) == (len(lv.kept), len(lv.pruned), len(lv.kept) + len(lv.pruned)), (lv.level, ci)
    assert (ci["kept_xor"], ci["kept_sum"]) == (x, s), lv.level
    assert ci["pruned_min_fp"] == (min(lv.pruned) if lv.pruned else None), lv.level
    if capped is not None and len(lv.pruned) > capped:
        with pytest.raises(mc_error(mc)) as e:
            mc.constraint_pruned(lv.level)
        assert e.value.code == -5 and ("has %d pruned states" % len(lv.pruned)) in e.value.message and ("holds the %d " % capped) in e.value.message, e.value.message
        assert mc.constraint_deep_results(lv.level)["list_overflowed"]
    elif lists:
        assert np.array_equal(mc.constraint_pruned(lv.level), cr.fps_of(lv.pruned)), lv.level


def mc_error(mc):
    import vsr_tlaplus_amd as vt
    return vt.VsrmcError


def _deepen_to_the_end(mc, ref, base, capped=None):
    """step() to `base`, then deepen() until nothing is inserted; every level against the reference.  -> {level: kind} of the levels filtered in scratch"""
    by_level = {lv.level: lv for lv in ref.levels}
    for _ in range(base - 1):
        mc.step()
    assert mc.level == base and mc.distinct == sum(len(lv.kept) for lv in ref.levels[:base])
    distinct = mc.distinct
    # pass 1 inserts level base + 1 without records: its info carries the unfiltered figures, the deep info says so
    a, p = mc.deepen()
    lv = by_level[base + 1]
    assert p is None and (a["level"], a["n_new"], a["generated"]) == (base + 1, len(lv.kept) + len(lv.pruned), lv.generated), a
    assert a["distinct"] == distinct + len(lv.kept) + len(lv.pruned)
    di = mc.constraint_deep_results(base + 1)
    assert (di["kind"], di["filtered"]) == ("regenerated", False)
    with pytest.raises(mc_error(mc)):
        mc.constraint_results(base + 1)                                     # no figures before the level was judged
    distinct += len(lv.kept)
    level = base + 1
    while True:
        a, p = mc.deepen()
        nxt = by_level.get(level + 1)
        if level == base + 1:                                              # this descent regenerated the unfiltered level, filtered it, and only then expanded it
            _check_level(mc, by_level[level], capped=capped)
            di = mc.constraint_deep_results(level)
            assert (di["kind"], di["filtered"]) == ("regenerated", True) and di["slices"] >= 1
        if nxt is None:
            assert (a["n_new"], a["level"], a["distinct"]) == (0, level, distinct), a
            break
        distinct += len(nxt.kept)
        x, s = cr.xor_sum(nxt.kept)
        # `generated` is the expand pass's: a pruned parent that was expanded would show here
        assert (a["n_new"], a["generated"], a["distinct"]) == (len(nxt.kept), nxt.generated, distinct), (level + 1, a["n_new"], a["generated"], a["distinct"])
        assert (a["fp_xor"], a["fp_sum"]) == (x, s), level + 1
        _check_level(mc, nxt, capped=capped)
        di = mc.constraint_deep_results(level + 1)
        assert (di["kind"], di["filtered"]) == ("inserted", True) and di["slices"] >= 1
        if not nxt.kept:
            assert a["level"] == level
            break
        assert a["level"] == level + 1
        level += 1
    assert (mc.depth, mc.distinct) == (ref.depth, ref.in_model)
    return {d["level"]: d["kind"] for d in mc.constraint_deep_results()}


# ---------------------------------------------------------------------------------------------------------------------
# 1. equals the reference from several bases
# ---------------------------------------------------------------------------------------------------------------------
def test_equals_the_reference_from_several_bases(vt, refs):
    ref = refs("main")
    assert [len(lv.kept) for lv in ref.levels] == KEPT and [len(lv.pruned) for lv in ref.levels] == PRUNED
    assert (ref.in_model, ref.pruned_total, ref.depth) == (4924, 1906, 25)
    n_regenerated = n_inserted = 0
    for base in (6, 12, 17):
        m, mc, w = _checker(vt, "main")
        kinds = _deepen_to_the_end(mc, ref, base)
        assert sorted(kinds) == list(range(base + 1, 26)), kinds
        assert kinds[base + 1] == "regenerated" and all(k == "inserted" for lvl, k in kinds.items() if lvl > base + 1)
        n_regenerated += sum(k == "regenerated" for k in kinds.values())
        n_inserted += sum(k == "inserted" for k in kinds.values())
        # every later descent filtered the regenerated levels again: the pruned states come back each time
        di = mc.constraint_deep_results(base + 2)
        # (level base + 2 is regenerated by the descents that insert levels base + 3 .. 25 and by the last one, which inserts nothing)
        assert di["launches"] > di["slices"] and di["regen_pruned"] == PRUNED[base + 1] * (24 - base), di
        assert di["regen_records"] == (KEPT[base + 1] + PRUNED[base + 1]) * (24 - base), di
        rs = mc.constraint_results()
        assert [(r["level"], r["kept"], r["pruned"]) for r in rs] == [(i + 1, KEPT[i], PRUNED[i]) for i in range(25)]
        mc.close()
    assert n_regenerated >= 3 and n_inserted >= 3                          # (not a test of stored levels)


# ---------------------------------------------------------------------------------------------------------------------
# 2. run() through the automatic scheme, with record buffers the search outgrows
# ---------------------------------------------------------------------------------------------------------------------
def test_run_through_the_automatic_scheme(vt, refs):
    ref = refs("main")
    by_level = {lv.level: lv for lv in ref.levels}
    m, mc, w = _checker(vt, "main", **SMALL)
    kinds = []
    after_rebase = 0
    while True:                                                            # run()'s loop, with a look at every stored level
        assert mc.room() != 2
        n_rebased = len(mc.rebased)
        kind, d, p = mc.advance()
        assert kind != "stopped", mc.stopped
        kinds.append(kind)
        if d["n_new"] == 0:
            break
        if kind == "level":
            assert np.array_equal(mc.level_fps(), cr.fps_of(by_level[d["level"]].kept)), d["level"]
        if len(mc.rebased) > n_rebased:                                    # a re-basing packed a level from filtered slices: it is the stored base now,
            after_rebase += 1                                              # or (kind "level") the parent of the level just stored and compared above
            rb = mc.rebased[-1]
            assert rb["n"] == len(by_level[rb["level"]].kept), rb
            if kind == "deep":
                assert mc.level == rb["level"] and np.array_equal(mc.level_fps(), cr.fps_of(by_level[rb["level"]].kept)), rb
    assert "deep" in kinds and after_rebase >= 1, (kinds, mc.rebased)
    assert (mc.depth, mc.distinct) == (25, 4924)
    rs = mc.constraint_results()
    assert len(rs) == 25
    for r, lv in zip(rs, ref.levels):
        x, s = cr.xor_sum(lv.kept)
        assert (r["level"], r["kept"], r["pruned"], r["kept_xor"], r["kept_sum"]) == (lv.level, len(lv.kept), len(lv.pruned), x, s), lv.level
        assert r["pruned_min_fp"] == (min(lv.pruned) if lv.pruned else None)
    mc.close()
    for how in ("run", "check"):
        m, mc, w = _checker(vt, "main", **SMALL)
        assert (mc.run() if how == "run" else mc.check()) == "exhausted"
        assert (mc.depth, mc.distinct) == (25, 4924)
        assert [(r["kept"], r["pruned"]) for r in mc.constraint_results()] == list(zip(KEPT, PRUNED))
        mc.close()
    # the same sizes without the opt-in: the stop of the stored path, as before
    m, mc, w = _checker(vt, "main", deep=False, **SMALL)
    assert mc.run() == "constraint-out-of-room" and "not constrained" in mc.stopped and 1 < mc.distinct < 4924
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. slicing variants give identical figures
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["small-pieces", "grid1", "list-of-4"])
def test_slicing_variants_give_identical_figures(vt, refs, monkeypatch, variant):
    ref = refs("main")
    kw, capped = {}, None
    if variant == "small-pieces":
        kw = dict(frontier_words=1 << 15, frontier_states=1 << 11)        # 2048 indices: the smallest the library takes (one index chunk)
    if variant == "grid1":
        monkeypatch.setenv("VSRMC_CONSTRAIN_GRID", "1")
    if variant == "list-of-4":
        monkeypatch.setenv("VSRMC_WHERE_LIST_CAP", "4")
        capped = 4
    m, mc, w = _checker(vt, "main", **kw)
    base = 8 if variant == "small-pieces" else 12
    _deepen_to_the_end(mc, ref, base, capped=capped)
    ds = mc.constraint_deep_results()
    if variant == "small-pieces":
        assert max(d["slices"] for d in ds) > 1, ds                         # some level was filtered in more than one scratch slice
    if variant == "list-of-4":
        assert [d["level"] for d in ds if d["list_overflowed"]] == [i + 1 for i in range(base, 25) if PRUNED[i] > 4]
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. degenerate constraints
# ---------------------------------------------------------------------------------------------------------------------
def test_true_prunes_nothing_and_changes_nothing(vt):
    m = vt.Model.from_constants(R=3, C_=1, n=2, L=1, invariant_mask=3)
    sizes = dict(SIZES, frontier_words=1 << 17, frontier_states=1 << 13)
    mc = vt.ModelChecker(m, device=0, **sizes)
    mc.constrain(m.compile_predicates(cr.TEXTS["True"]), deep=True)
    plain = vt.ModelChecker(m, device=0, **sizes)
    keys = ("level", "frontier", "generated", "n_new", "distinct", "total_generated", "deadlocks", "max_bag", "fp_xor", "fp_sum", "viol_mask", "viol_fp", "act_generated")
    pkeys = ("level", "frontier", "generated", "distinct", "deadlocks", "viol_mask", "viol_fp", "act_generated")
    for _ in range(9):
        a, b = mc.step(), plain.step()
        assert a["n_new"] == b["n_new"] and not a["viol_mask"]
    violated = False
    for _ in range(8):
        (a, p), (b, q) = mc.deepen(), plain.deepen()
        assert {k: a[k] for k in keys} == {k: b[k] for k in keys}, a["level"]
        assert (p is None) == (q is None)
        if p is not None:
            assert {k: p[k] for k in pkeys} == {k: q[k] for k in pkeys}, p["level"]
        if a["viol_mask"] or (p is not None and p["viol_mask"]):
            violated = True
            assert mc.violation == plain.violation
            assert [r.tolist() for _a, r in mc.probe_trace()] == [r.tolist() for _a, r in plain.probe_trace()]
            break
    assert sum(r["pruned"] for r in mc.constraint_results()) == 0
    assert all(d["filtered"] for d in mc.constraint_deep_results()[:-1]) and len(mc.constraint_deep_results()) >= 2
    assert violated or a["level"] == 17
    mc.close()
    plain.close()


@pytest.mark.parametrize("name", ["False", "InitOnly"])
def test_nothing_in_the_model_ends_without_a_launch_beyond_init(vt, name):
    m = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
    mc = vt.ModelChecker(m, device=0, **dict(SIZES, **SMALL))
    mc.constrain(m.compile_predicates(cr.TEXTS[name]), deep=True)
    assert mc.run() == "exhausted"
    assert (mc.depth, mc.distinct) == (1, 0 if name == "False" else 1)
    assert mc.constraint_deep_results() == []                              # no level ever went through a scratch buffer
    assert len(mc.constraint_results()) == (1 if name == "False" else 2)
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. a built-in violation on a pruned state of a deep level: in the probed level, then in the inserted one
# ---------------------------------------------------------------------------------------------------------------------
def test_built_in_violation_on_a_pruned_state(vt, refs):
    ref = refs("commit")
    orc, unpack, make_pm = cr.oracle_of("first")
    P, PM = cr.params_of("first", 3, 1, 2, 1, invariant_mask=3), make_pm(3, 1, 2, 1)
    bad = sorted((lv.level, fp) for lv in ref.levels for fp, rec in lv.pruned.items() if orc.invariants(P, rec))
    assert bad and bad[0][0] == 19 and not any(orc.invariants(P, rec) for lv in ref.levels for rec in lv.kept.values())
    fp_bad = min(fp for lvl, fp in bad if lvl == 19)

    def behaviour(tr):
        assert len(tr) == 19 and orc.fingerprint(P, tr[-1][1])[0] == fp_bad and orc.invariants(P, tr[-1][1]) == 2
        states = [unpack(PM, [int(x) for x in rec]) for _a, rec in tr]
        assert all(cr.r3normal_commit_below2(s) for s in states[:-1]) and not cr.r3normal_commit_below2(states[-1])
        for t in range(1, len(tr)):
            assert orc.fingerprint(P, tr[t][1])[0] in set(s["fp"] for s in orc.successors(P, tr[t - 1][1])), t
        for t, (_act, rec) in enumerate(tr[:-1]):
            assert orc.fingerprint(P, rec)[0] in ref.levels[t].kept, t

    for base in (10, 16):
        m, mc, w = _checker(vt, "commit", model_kw=dict(invariant_mask=3))
        for _ in range(base - 1):
            assert not mc.step()["viol_mask"]
        while True:
            a, p = mc.deepen()
            assert not a["viol_mask"]
            if p is not None and p["viol_mask"]:
                break
            assert a["level"] < 18
        assert (a["level"], p["level"], p["viol_fp"], p["viol_mask"]) == (18, 19, fp_bad, 2), (a["level"], p)   # probed: a successor of an in-model state of level 18
        assert mc.violation == dict(level=19, index=None, fp=fp_bad, mask=2, probed=True)
        behaviour(mc.probe_trace())
        behaviour(mc.violation_trace())
        a, p = mc.deepen()                                                 # the caller goes on: level 19 is inserted, the violator with it, and pruned
        assert (a["level"], a["viol_fp"], a["viol_mask"]) == (19, fp_bad, 2) and p is None
        behaviour(mc.probe_trace())
        assert fp_bad in set(int(f) for f in mc.constraint_pruned(19))
        behaviour(mc.trace_fp(19, fp_bad))                                 # pruned, and still traceable by fingerprint
        mc.close()
    # through the automatic scheme, small buffers
    for how in ("run", "check"):
        m, mc, w = _checker(vt, "commit", model_kw=dict(invariant_mask=3), **SMALL)
        assert (mc.run() if how == "run" else mc.check()) == "violation"
        assert (mc.violation["level"], mc.violation["fp"], mc.violation["mask"]) == (19, fp_bad, 2), mc.violation
        behaviour(mc.violation_trace())
        mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. a user's invariant violated among the pruned states of a deep level
# ---------------------------------------------------------------------------------------------------------------------
def test_invariant_violated_among_the_pruned_states_of_a_deep_level(vt, refs):
    ref = refs("main")
    orc, unpack, make_pm = cr.oracle_of("first")
    P, PM = cr.params_of("first", 3, 1, 2, 1), make_pm(3, 1, 2, 1)
    level = fp = count = None
    for lv in ref.levels:
        hit = [f for f, rec in lv.pruned.items() if not cr.not_all_in_view_change(unpack(PM, [int(x) for x in rec]))]
        if hit:
            level, fp, count = lv.level, min(hit), len(hit)
            break
    assert level is not None and level >= 4
    m = _model(vt, "main")
    bad_text = r"Bad == \A r \in replicas : rep_status[r] = ViewChange"
    for base in (level - 1, level - 2, level - 3):                         # the level is the first unfiltered one, the first inserted one, a later inserted one
        assert 1 <= base < level                                           # the base is BELOW the level: the violator is pruned in a scratch buffer
        mc = vt.ModelChecker(m, device=0, **SIZES)
        mc.constrain(m.compile_predicates(cr.TEXTS["Replica3Normal"] + "\n" + bad_text), "Replica3Normal", deep=True)
        never = m.compile_predicates(bad_text)
        for _ in range(base - 1):
            mc.step()
        mc.deepen()
        mc._pruned_checked = base                                          # (run() has looked at the stored levels)
        while True:                                                        # run(never=..)'s own check, after every pass
            if mc._never_on_pruned(never):
                break
            a, p = mc.deepen()
            assert a["n_new"], "the search ended without the violation"
        wit = mc.witness
        assert (wit["level"], wit["fp"], wit["name"], wit.get("pruned")) == (level, fp, "Bad", True), wit
        assert mc.level == base and mc.depth >= level
        assert mc.constraint_results(level)["pruned_count"] == {"Replica3Normal": 0, "Bad": count}
        tr = mc.witness_trace()
        assert len(tr) == level and orc.fingerprint(P, tr[-1][1])[0] == fp
        states = [unpack(PM, [int(x) for x in rec]) for _a, rec in tr]
        assert all(cr.replica3_normal(s) and cr.not_all_in_view_change(s) for s in states[:-1])
        assert not cr.replica3_normal(states[-1]) and not cr.not_all_in_view_change(states[-1])
        mc.close()
    # run(never=..) itself, with buffers it outgrows below the level
    mc = vt.ModelChecker(m, device=0, **dict(SIZES, **SMALL))
    mc.constrain(m.compile_predicates(cr.TEXTS["Replica3Normal"] + "\n" + bad_text), "Replica3Normal", deep=True)
    assert mc.run(never=m.compile_predicates(bad_text)) == "violation"
    assert (mc.witness["level"], mc.witness["fp"], mc.witness.get("pruned")) == (level, fp, True)
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. every behaviour into a deep level stays in the model
# ---------------------------------------------------------------------------------------------------------------------
def test_trace_fp_stays_in_the_model(vt, refs):
    ref = refs("main")
    orc, unpack, make_pm = cr.oracle_of("first")
    P, PM = cr.params_of("first", 3, 1, 2, 1), make_pm(3, 1, 2, 1)
    m, mc, w = _checker(vt, "main")
    base = 9
    for _ in range(base - 1):
        mc.step()
    while mc.deepen()[0]["n_new"]:
        pass
    assert mc.level == base and mc.depth == 25
    picks = [(lv.level, f) for lv in ref.levels[base:] for f in sorted(lv.kept)[:2]][:20]
    assert len(picks) == 20 and all(lvl > base for lvl, _f in picks)
    for lvl, f in picks:
        tr = mc.trace_fp(lvl, f)
        assert len(tr) == lvl and orc.fingerprint(P, tr[-1][1])[0] == f
        for t, (_act, rec) in enumerate(tr):
            assert cr.replica3_normal(unpack(PM, [int(x) for x in rec])), (lvl, t)
            assert orc.fingerprint(P, rec)[0] in ref.levels[t].kept, (lvl, t)
        for t in range(1, len(tr)):
            assert orc.fingerprint(P, tr[t][1])[0] in set(s["fp"] for s in orc.successors(P, tr[t - 1][1])), (lvl, t)
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. one analysis model
# ---------------------------------------------------------------------------------------------------------------------
def test_analysis_model(vt, refs):
    ref = refs("nost-second")
    assert len(ref.levels) == 12 and [len(lv.pruned) for lv in ref.levels[10:]] == [4, 6]
    m, mc, w = _checker(vt, "nost-second", frontier_words=1 << 24, frontier_states=1 << 18)
    base = 8
    for _ in range(base - 1):
        mc.step()
    distinct = mc.distinct
    a, p = mc.deepen()
    assert a["n_new"] == len(ref.levels[base].kept) + len(ref.levels[base].pruned)
    distinct += len(ref.levels[base].kept)
    for lv in ref.levels[base + 1:]:
        a, p = mc.deepen()
        distinct += len(lv.kept)
        x, s = cr.xor_sum(lv.kept)
        assert (a["level"], a["n_new"], a["generated"], a["distinct"], a["fp_xor"], a["fp_sum"]) == (lv.level, len(lv.kept), lv.generated, distinct, x, s), lv.level
        if lv.level == base + 2:
            _check_level(mc, ref.levels[base])
        _check_level(mc, lv)
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals, and the CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(vt, tmp_path):
    import ctypes as C
    from vsr_tlaplus_amd import capi
    m = vt.Model.from_constants(R=3, C_=1, n=2, L=1)
    w = m.compile_predicates(cr.TEXTS["Replica3Normal"])
    step = m.compile_step("Mono == \\A r \\in replicas : rep_view_number'[r] >= rep_view_number[r]")
    lib = vt.load()

    def refused(f, code, needle):
        with pytest.raises(vt.VsrmcError) as e:
            f()
        assert e.value.code == code and needle in e.value.message, (e.value.code, e.value.message)

    mc = vt.ModelChecker(m, device=0, **SIZES)
    assert lib.vsrmc_checker_constrain_deep(mc._h, 1) == -6 and "no constraint attached" in lib.vsrmc_last_error().decode()
    # an action constraint, in either order
    mc.action_constrain(step)
    refused(lambda: mc.constrain(w, deep=True), -6, "an action constraint is attached")
    assert mc._constraint is None and mc.step()["n_new"] > 0
    mc.reset()
    mc.action_constrain(None)
    mc.constrain(w, deep=True)
    refused(lambda: mc.action_constrain(step), -6, "vsrmc_checker_constrain_deep")
    # after level 1
    mc.step()
    assert lib.vsrmc_checker_constrain_deep(mc._h, 0) == -6 and "at level 1 only" in lib.vsrmc_last_error().decode()
    # the paths that do not filter
    for name in ("vsrmc_checker_probe2", "vsrmc_checker_probe3"):
        infos = [capi.LevelInfo() for _ in range(3)]
        rc = getattr(lib, name)(mc._h, *[C.byref(i) for i in infos[: 2 if name.endswith("2") else 3]])
        assert rc == -6 and "does not filter" in lib.vsrmc_last_error().decode(), name
    refused(lambda: mc.deep_attach(m.compile_predicates(cr.TEXTS["True"]), None), -6, "judged on arrival")
    refused(mc.deep_terminal_attach, -6, "judged on arrival")
    refused(lambda: mc.save(str(tmp_path / "chk")), -6, "does not name it")
    assert not os.path.exists(str(tmp_path / "chk"))
    a, p = mc.deepen()                                                     # ... and what is not refused any more
    assert a["n_new"] > 0 and mc.probe if True else None
    mc.close()
    # probe() of the newest stored level: its states are all judged
    mc = vt.ModelChecker(m, device=0, **SIZES)
    mc.constrain(w, deep=True)
    for _ in range(4):
        mc.step()
    assert mc.probe()["level"] == 6
    mc.close()
    # exact_ties
    mc = vt.ModelChecker(m, device=0, exact_ties=True, **SIZES)
    refused(lambda: mc.constrain(w, deep=True), -6, "exact_ties")
    assert mc._constraint is None
    mc.close()
    # a sharded checker (world 2, one rank of it): no constraint is attached, so there is nothing to opt in
    o = capi.Options()
    lib.vsrmc_options_default(C.byref(o))
    o.table_log2, o.frontier_words, o.frontier_states, o.pending_entries, o.world, o.rank = 18, 1 << 20, 1 << 14, 1 << 15, 2, 0
    h = C.c_void_p()
    capi.check(lib.vsrmc_checker_create(m._h, C.byref(o), C.byref(h)))
    try:
        assert lib.vsrmc_checker_constrain_attach(h, w._h, 0) == -6 and "sharded" in lib.vsrmc_last_error().decode()
        assert lib.vsrmc_checker_constrain_deep(h, 1) == -6
    finally:
        lib.vsrmc_checker_destroy(h)


def _cli(tmp_path, extra, R="3", vals="v1, v2", both_invariants=False, frontier="0.0005", predicates=None):
    cfg = tmp_path / "VSR.cfg"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_cfg.py"), str(cfg), R, "1", vals, "1"], check=True)
    if both_invariants:
        with open(cfg, "a") as f:
            f.write("AcknowledgedWritesExistOnMajority\n")
    # 0.0005 GiB: 67 108 record words and 2 796 indices per buffer, which this space outgrows (the stored path ends with exit 4, below)
    args = [CLI, "-config", str(cfg), "-noTLA", "-tableLog2", "18", "-frontierGiB", frontier, "-predicates", predicates or os.path.join(ROOT, "tools", "constraints_example.txt")] + extra
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


def test_cli_rows_and_closing_line(vt, refs, tmp_path):
    ref = refs("main")
    r = _cli(tmp_path, ["-constraint", "Replica3Normal", "-deepConstraint"])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr)
    out = r.stdout
    virt = [ln for ln in out.splitlines() if ln.startswith("Virtual(")]
    assert virt, out[-3000:]
    seen_levels, deep_levels = set(), set()
    cum_kept = np.cumsum(KEPT)
    for ln in out.splitlines():
        if ln.startswith("Progress(") or ln.startswith("Virtual("):
            lvl = int(ln[ln.index("(") + 1: ln.index(")")])
            seen_levels.add(lvl)
            if ln.startswith("Virtual("):
                deep_levels.add(lvl)
            if ln.startswith("Virtual(") and "in the model" in ln:         # a filtered inserted level: in-model figures
                assert ("%d distinct states found, %d states in the level" % (cum_kept[lvl - 1], KEPT[lvl - 1])) in ln, ln
                assert ("%d in the model, %d out of model" % (KEPT[lvl - 1], PRUNED[lvl - 1])) in ln, ln
            if ln.startswith("Progress("):
                assert ("%d distinct states found, %d states left on queue." % (cum_kept[lvl - 1], KEPT[lvl - 1])) in ln, ln
    assert seen_levels == set(range(2, 26)), seen_levels
    filtered = {}
    for ln in out.splitlines():                                            # a level that was inserted before it could be judged: judged by the next pass
        if ln.startswith("Filtered("):
            lvl = int(ln[ln.index("(") + 1: ln.index(")")])
            filtered[lvl] = ln
            assert ("%d in the model, %d out of model" % (KEPT[lvl - 1], PRUNED[lvl - 1])) in ln, ln
    unjudged = set(int(ln[ln.index("(") + 1: ln.index(")")]) for ln in out.splitlines() if ln.startswith("Virtual(") and "not judged yet" in ln)
    assert unjudged and unjudged == set(filtered), (unjudged, sorted(filtered))
    assert len(deep_levels) >= 3
    assert "Model checking completed. No error has been found." in out
    assert ("CONSTRAINT Replica3Normal: %d states were out of model and not explored" % ref.pruned_total) in out
    assert ("levels beyond the record buffers included: %d in-model states kept and %d pruned in the %d level(s) filtered there." %
            (sum(KEPT[l - 1] for l in deep_levels), sum(PRUNED[l - 1] for l in deep_levels), len(deep_levels))) in out
    assert ("%d distinct states found, 0 states left on queue." % ref.in_model) in out
    assert "The depth of the complete state graph search is 25." in out
    # without the opt-in: the stop of the stored path, exit 4
    r = _cli(tmp_path, ["-constraint", "Replica3Normal"])
    assert r.returncode == 4, (r.returncode, r.stdout[-2000:], r.stderr)


def test_cli_exit_codes(vt, refs, tmp_path):
    # 12: -invariant violated among the pruned states of a level beyond the record buffers
    r = _cli(tmp_path, ["-constraint", "Replica3Normal", "-deepConstraint", "-invariant", "NotAllInViewChange"])
    assert r.returncode == 12, (r.returncode, r.stdout[-3000:], r.stderr)
    assert "Error: Invariant NotAllInViewChange is violated (by a state of level " in r.stdout and "outside CONSTRAINT Replica3Normal" in r.stdout
    # (on this space the first such state is in level 4, a stored level under every buffer size the CLI takes: the levels beyond the buffers are reached
    # through the Python interface, test_invariant_violated_among_the_pruned_states_of_a_deep_level; here: the flag changes nothing about that report)
    # a built-in invariant on an out-of-model state of a level beyond the buffers: the exit code and the message of the stored path, which the same
    # command line with buffers that hold every level gives
    text = tmp_path / "commit.txt"
    text.write_text(cr.TEXTS["R3NormalCommitBelow2"] + "\n")
    stored = _cli(tmp_path, ["-constraint", "R3NormalCommitBelow2"], both_invariants=True, frontier="0.05", predicates=str(text))
    assert stored.returncode == 12 and "Virtual(" not in stored.stdout, (stored.returncode, stored.stdout[-2000:], stored.stderr)
    # (0.00037 GiB: 49 660 words and 2 069 indices per buffer, the fewest indices the CLI's sizing rule gives above the library's floor of 2 048.  This
    # space is narrower than Replica3Normal's — 628 states written at level 18 — and fits the 2 796 indices of the other runs whole)
    r = _cli(tmp_path, ["-constraint", "R3NormalCommitBelow2", "-deepConstraint"], both_invariants=True, frontier="0.00037", predicates=str(text))
    assert r.returncode == stored.returncode, (r.returncode, r.stdout[-3000:], r.stderr)
    assert "Virtual(" in r.stdout and "Error: Invariant AcknowledgedWritesExistOnMajority is violated." in r.stdout
    assert "Error: Invariant AcknowledgedWritesExistOnMajority is violated." in stored.stdout
    last = lambda out: out.split("The behavior up to this point is:\n", 1)[1].split("State 19:", 1)[1]
    assert last(r.stdout).split("\n\n")[0] == last(stored.stdout).split("\n\n")[0]        # the same violator (the smallest fingerprint of level 19)
