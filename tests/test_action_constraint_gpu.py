"""Action constraints on the GPU (`-m gpu`): k_step_list / k_step_apply / k_step_expand through ModelChecker.action_constrain / step / run /
action_constraint_results, the traces and the CLI, against tests/action_constraint_reference.py — a Python BFS over the CPU oracles' successor function
that skips every transition a hand-written Python predicate forbids (the reference is never the parser).  Every figure is recomputed from the oracle
here; a reference is computed once per space and shared.  Per level the comparison is: new states, `generated`, the per-action counts, blocked in total
and per action, the fingerprint set, xor and sum."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import action_constraint_reference as ar
import constraint_reference as cr
import step_models_reference as smr
import step_reference as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
EXAMPLE = os.path.join(ROOT, "tools", "action_constraints_example.txt")
SIZES = dict(table_log2=20, frontier_words=1 << 22, frontier_states=1 << 17, pending_entries=1 << 17)
LOG_NEVER_SHRINKS_MODELS = "LogNeverShrinks == " + smr.LOG_NEVER_SHRINKS
# key -> (model, R, C, n, L, text of the constraint, Python predicate, level cap, Python state constraint or None)
CASES = {
    "quiet-2122": ("first", 2, 1, 2, 2, ar.TEXTS["QuietClient"], ar.quiet_client, None, None),
    "quiet-3121": ("first", 3, 1, 2, 1, ar.TEXTS["QuietClient"], ar.quiet_client, 11, None),
    "commit-3111": ("first", 3, 1, 1, 1, ar.TEXTS["CommitNeverDecreases"], sr.commit_monotonic, 15, None),
    "timers-2122": ("first", 2, 1, 2, 2, ar.TEXTS["TimersInView1"], ar.timers_in_view_1, None, None),
    "true-2122": ("first", 2, 1, 2, 2, ar.TEXTS["True"], ar.always, None, None),
    "true-3121": ("first", 3, 1, 2, 1, ar.TEXTS["True"], ar.always, 12, None),
    "false-2122": ("first", 2, 1, 2, 2, ar.TEXTS["False"], ar.never, None, None),
    "narrowprimed-2122": ("first", 2, 1, 2, 2, ar.TEXTS["NarrowNetworkPrimed"], ar.primed(cr.narrow_network), None, None),
    "both-3121": ("first", 3, 1, 2, 1, ar.TEXTS["QuietClient"], ar.quiet_client, 11, cr.replica3_normal),
    # the analysis models: LogNeverShrinks of their step reference, chosen with the reference — it blocks 2 + 22 ReceiveSV transitions on levels 10 and 11
    # (CommitMonotonic blocks nothing within 12 levels of either; "no replica enters StateTransfer" blocks 4 on level 11)
    "shrinks-second": ("second", 3, 0, 2, 1, LOG_NEVER_SHRINKS_MODELS, smr.log_never_shrinks, 11, None),
    "shrinks-third": ("third", 3, 0, 2, 1, LOG_NEVER_SHRINKS_MODELS, smr.log_never_shrinks, 11, None),
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
            which, R, C, n, L, _text, fn, cap, state = CASES[key]
            cache[key] = ar.constrained_bfs(which, R, C, n, L, fn, max_levels=cap, state_constraint=state)
        return cache[key]
    return get


def _model(vt, key):
    which, R, C, n, L = CASES[key][:5]
    if which == "first":
        return vt.Model.from_constants(R=R, C_=C, n=n, L=L)
    return (vt.Model.second_model if which == "second" else vt.Model.third_model)(R=R, n=n, L=L)


def _checker(vt, key, **kw):
    m = _model(vt, key)
    mc = vt.ModelChecker(m, device=0, **dict(SIZES, **kw))
    w = m.compile_step_predicates(CASES[key][5])
    mc.action_constrain(w)
    return m, mc, w


def _act_counts(vt, d):
    return {vt.ACTION_NAMES[a]: int(n) for a, n in enumerate(d["act_generated"]) if n and a > 0}


def _walk(vt, mc, ref):
    """step the checker level by level beside the reference, every figure compared; -> the list of per-level tuples (what the variants of one space must agree on)"""
    assert mc.distinct == len(ref.levels[0].new) and mc.n_frontier == len(ref.levels[0].new)
    distinct, rows = len(ref.levels[0].new), []
    for lv in ref.levels[1:]:
        d = mc.step()
        distinct += len(lv.new)
        print("level %d: new %d generated %d blocked %d (reference %d %d %d)" % (lv.level, d["n_new"], d["generated"], mc.action_constraint_results(0)["blocked"],
                                                                                   len(lv.new), lv.generated, lv.blocked))
        assert (d["n_new"], d["generated"], d["distinct"]) == (len(lv.new), lv.generated, distinct), (lv.level, d["n_new"], d["generated"], d["distinct"])
        assert _act_counts(vt, d) == lv.act_generated, lv.level
        ai = mc.action_constraint_results(lv.level)
        assert ai == mc.action_constraint_results(0) and ai["level"] == lv.level
        assert (ai["pairs"], ai["blocked"], ai["permitted"], ai["n_new"]) == (lv.generated, lv.blocked, lv.generated - lv.blocked, len(lv.new) + len(lv.pruned)), lv.level
        assert ai["blocked_act"] == lv.blocked_act, lv.level
        assert (ai["blocked_min_fp"] is None) == (lv.blocked == 0) and ai["slices"] >= 1 and ai["launches"] >= ai["slices"]
        x, s = ar.xor_sum(lv.new)
        if lv.new:
            assert d["level"] == lv.level
            assert np.array_equal(mc.level_fps(), ar.new_fps(lv)), lv.level
            assert mc.level_checksum() == (x, s, len(lv.new)), lv.level
        else:
            assert d["level"] == lv.level - 1 and mc.n_frontier == 0
        rows.append((lv.level, d["n_new"], d["generated"], tuple(d["act_generated"]), ai["blocked"], tuple(sorted(ai["blocked_act"].items())), x, s))
    return rows


# ---------------------------------------------------------------------------------------------------------------------
# 1. QuietClient on (2,1,{v1,v2},2), exhausted: every rescued state is there, no state the reference lacks
# ---------------------------------------------------------------------------------------------------------------------
def test_quiet_client_whole_space(vt, refs):
    ref = refs("quiet-2122")
    plain = refs("true-2122")
    assert ref.states < plain.states and ref.blocked >= 50 and ref.rescued >= 5     # the input bites: states lost, transitions blocked, states a per-state gate would lose
    m, mc, w = _checker(vt, "quiet-2122")
    _walk(vt, mc, ref)
    assert mc.distinct == ref.states and mc.depth == ref.depth
    assert mc.seen_set_load()[0] == mc.distinct                                        # a blocked successor takes no seen-set slot
    mc.reset()
    got = {}
    while True:
        got[mc.level] = set(int(f) for f in mc.level_fps())
        if mc.step()["n_new"] == 0:
            break
    for lv in ref.levels:
        if lv.new:
            assert got[lv.level] == set(lv.new), lv.level                              # nothing the reference lacks, nothing missing
            assert set(lv.rescued) <= got[lv.level], lv.level                          # in through a permitted edge although another edge into them was blocked
    mc.reset()
    assert mc.run() == "exhausted" and (mc.depth, mc.distinct) == (ref.depth, ref.states)
    rs = mc.action_constraint_results()
    assert [(r["level"], r["blocked"]) for r in rs] == [(lv.level, lv.blocked) for lv in ref.levels[1:]]
    assert sum(r["blocked"] for r in rs) == ref.blocked and all(r["list_ms"] > 0 for r in rs)


# ---------------------------------------------------------------------------------------------------------------------
# 2. QuietClient on (3,1,{v1,v2},1), levels 1-11, under four slice regimes: identical figures
# ---------------------------------------------------------------------------------------------------------------------
def test_slices_give_identical_figures(vt, refs, monkeypatch):
    ref = refs("quiet-3121")
    assert ref.blocked >= 100 and ref.rescued >= 10
    rows, shape = {}, {}
    for variant, env in (("default", {}), ("slice1", dict(VSRMC_ACTION_SLICE="1")), ("slice7", dict(VSRMC_ACTION_SLICE="7")),
                         ("overflow", dict(VSRMC_ACTION_LIST_CAP="64", VSRMC_ACTION_SLICE="64")), ("smallcap", dict(VSRMC_ACTION_LIST_CAP="64"))):
        for k in ("VSRMC_ACTION_SLICE", "VSRMC_ACTION_LIST_CAP"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m, mc, w = _checker(vt, "quiet-3121")
        rows[variant] = _walk(vt, mc, ref)
        rs = mc.action_constraint_results()
        shape[variant] = (sum(r["slices"] for r in rs), sum(r["relisted"] for r in rs))
        assert mc.seen_set_load()[0] == mc.distinct == ref.states
        mc.close()
    assert all(rows[v] == rows["default"] for v in rows)
    big = max(len(lv.new) for lv in ref.levels[:-1])
    assert shape["default"][1] == 0 and shape["default"][0] == len(ref.levels) - 1      # one slice per level, nothing listed again
    assert shape["slice1"][0] == sum(len(lv.new) for lv in ref.levels[:-1])             # a slice per parent
    assert shape["slice7"][0] >= big // 7
    assert shape["overflow"][1] > 0 and shape["smallcap"][0] > shape["default"][0]      # slices overflowed the list and were listed again in halves


# ---------------------------------------------------------------------------------------------------------------------
# 3. CommitMonotonic as a constraint on (3,1,{v1},1), levels 1-15: 99 ReceiveSV steps not taken, on levels 13-15
# ---------------------------------------------------------------------------------------------------------------------
def test_commit_never_decreases(vt, refs):
    ref = refs("commit-3111")
    assert ref.blocked > 0 and all(set(lv.blocked_act) <= {"ReceiveSV"} for lv in ref.levels)
    m, mc, w = _checker(vt, "commit-3111")
    _walk(vt, mc, ref)
    assert mc.seen_set_load()[0] == mc.distinct == ref.states


# ---------------------------------------------------------------------------------------------------------------------
# 4. TimersInView1: a small model, the run ends like an exhausted search
# ---------------------------------------------------------------------------------------------------------------------
def test_timers_in_view_1_exhausts(vt, refs):
    ref = refs("timers-2122")
    assert ref.states < refs("true-2122").states // 4
    m, mc, w = _checker(vt, "timers-2122")
    _walk(vt, mc, ref)
    mc.reset()
    assert mc.run() == "exhausted" and (mc.depth, mc.distinct) == (ref.depth, ref.states)
    mc.reset()
    assert mc.check() == "exhausted" and (mc.depth, mc.distinct) == (ref.depth, ref.states)


# ---------------------------------------------------------------------------------------------------------------------
# 5. TRUE: the plain search.  (3,1,{v1,v2},1), levels 1-12: against the plain checker and the Python reference, level by level — tests/golden has no level
#    file of that space (oracle_levels_*.json are configs 2, 3, 4, 5 and the analysis models, and bfs_counts.json has no (3,1,{v1,v2},1) either), so the comparison against golden files runs on the spaces
#    that have one: the first 10 levels of config 2 (3,1,{v1,v2},2), the first 7 of config 5 (five replicas) and of config 4 (two clients, policy
#    assume_commit_number).  Here k_step_expand meets five replicas and two clients near Init, where nothing is blocked and counts and checksums are compared;
#    test_constrained_seeded_gpu.py runs it on harvested states of (5,1,2,1), (4,1,2,1) and (3,2,3,1) under constraints that block, record by record.
# ---------------------------------------------------------------------------------------------------------------------
def test_true_equals_the_plain_checker(vt, refs):
    ref = refs("true-3121")
    m, mc, w = _checker(vt, "true-3121")
    plain = vt.ModelChecker(m, device=0, **SIZES)
    for lv in ref.levels[1:]:
        d, p = mc.step(), plain.step()
        for k in ("level", "n_new", "generated", "distinct", "deadlocks", "max_bag", "act_generated", "record_words", "viol_mask", "total_generated"):
            assert d[k] == p[k], (lv.level, k, d[k], p[k])
        assert (d["n_new"], d["generated"]) == (len(lv.new), lv.generated) and lv.blocked == 0
        assert np.array_equal(mc.level_fps(), plain.level_fps()) and mc.level_checksum() == plain.level_checksum()
        assert mc.action_constraint_results(0)["blocked"] == 0


@pytest.mark.parametrize("label,n_levels,kw", [("config2", 10, dict(R=3, C_=1, n=2, L=2)), ("config5", 7, dict(R=5, C_=1, n=2, L=2)),
                                                ("config4", 7, dict(R=3, C_=2, n=3, L=3, assume_commit_number=True))])
def test_true_equals_the_golden_levels(vt, oracle_levels, label, n_levels, kw):
    fx = oracle_levels[label]
    m = vt.Model.from_constants(**kw)
    mc = vt.ModelChecker(m, device=0, **SIZES)
    mc.action_constrain(m.compile_step_predicates(ar.TEXTS["True"]))
    for want in fx["levels"][1:n_levels]:
        d = mc.step()
        assert (d["level"], d["n_new"], d["generated"], d["deadlocks"], d["max_bag"]) == (want["level"], want["new"], want["generated"], want["deadlocks"], want["max_bag"])
        assert d["act_generated"][1:] == want["act_generated"][1:], want["level"]
        if fx["checksums"]:
            assert mc.level_checksum() == (int(want["fp_xor"], 16), int(want["fp_sum"], 16), want["new"]), want["level"]
        assert mc.action_constraint_results(0)["blocked"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. FALSE: nothing is taken — level 2 is empty, everything Init generates is blocked
# ---------------------------------------------------------------------------------------------------------------------
def test_false_blocks_everything(vt, refs):
    ref = refs("false-2122")
    assert len(ref.levels) == 2 and not ref.levels[1].new and ref.levels[1].blocked == ref.levels[1].generated > 0
    m, mc, w = _checker(vt, "false-2122")
    _walk(vt, mc, ref)
    assert (mc.level, mc.distinct, mc.n_frontier) == (1, 1, 0)
    mc.reset()
    assert mc.run() == "exhausted" and (mc.depth, mc.distinct) == (1, 1)
    assert mc.seen_set_load()[0] == 1


# ---------------------------------------------------------------------------------------------------------------------
# 7. a predicate of the successor alone keeps what the state constraint of the same text keeps, from level 2 on
# ---------------------------------------------------------------------------------------------------------------------
def test_primed_only_predicate_equals_the_state_constraint(vt, refs):
    ref = refs("narrowprimed-2122")
    m, mc, w = _checker(vt, "narrowprimed-2122")
    _walk(vt, mc, ref)
    mc2 = vt.ModelChecker(m, device=0, **SIZES)
    mc2.constrain(m.compile_predicates(cr.TEXTS["NarrowNetwork"]))
    mc.reset()
    assert mc2.n_frontier == 1                                                         # (Init satisfies NarrowNetwork: the two searches start alike)
    while True:
        assert np.array_equal(mc.level_fps(), mc2.level_fps()), mc.level
        a, b = mc.step(), mc2.step()
        assert (a["n_new"], a["generated"]) == (b["n_new"], b["generated"])
        if a["n_new"] == 0:
            break
    assert mc.distinct == mc2.distinct == ref.states


# ---------------------------------------------------------------------------------------------------------------------
# 8. a state constraint and an action constraint at once
# ---------------------------------------------------------------------------------------------------------------------
def test_both_kinds_attached(vt, refs):
    ref = refs("both-3121")
    assert ref.blocked > 0 and sum(len(lv.pruned) for lv in ref.levels) > 0
    m = _model(vt, "both-3121")
    mc = vt.ModelChecker(m, device=0, **SIZES)
    mc.constrain(m.compile_predicates(cr.TEXTS["Replica3Normal"]))
    mc.action_constrain(m.compile_step_predicates(ar.TEXTS["QuietClient"]))
    _walk(vt, mc, ref)
    for lv in ref.levels[1:]:
        ci = mc.constraint_results(lv.level) if (lv.new or lv.pruned) else None
        if ci:
            assert (ci["kept"], ci["pruned"]) == (len(lv.new), len(lv.pruned)), lv.level
    assert mc.seen_set_load()[0] == ref.states + sum(len(lv.pruned) for lv in ref.levels)   # (a state the STATE constraint pruned keeps its slot, §9h)


# ---------------------------------------------------------------------------------------------------------------------
# 9. a seen-set that starts far too small: it is re-hashed mid-run, the figures stay, occupied slots = distinct states
# ---------------------------------------------------------------------------------------------------------------------
def test_small_table_grows(vt, refs):
    ref = refs("quiet-3121")
    m, mc, w = _checker(vt, "quiet-3121", table_log2=8)
    distinct = 1
    for lv in ref.levels[1:]:
        assert mc.room() in (0, 1)
        d = mc.step()
        distinct += len(lv.new)
        assert (d["n_new"], d["generated"], d["distinct"]) == (len(lv.new), lv.generated, distinct), lv.level
        assert mc.action_constraint_results(0)["blocked"] == lv.blocked
        assert mc.level_checksum() == ar.xor_sum(lv.new) + (len(lv.new),)
        occ, slots = mc.seen_set_load()
        assert occ == distinct and slots == 1 << mc.options.table_log2
    assert mc.options.table_log2 > 8


# ---------------------------------------------------------------------------------------------------------------------
# 10. record buffers too small for a late level: the run ends with the constraint's own stop, incomplete, the levels before it correct
# ---------------------------------------------------------------------------------------------------------------------
def test_out_of_room_ends_the_run(vt, refs):
    ref = refs("quiet-3121")
    m, mc, w = _checker(vt, "quiet-3121", frontier_words=1 << 15, frontier_states=1 << 12)
    assert mc.run() == "constraint-out-of-room"
    assert "not constrained" in mc.stopped and 1 < mc.distinct < ref.states and mc.depth == mc.level < len(ref.levels)
    assert mc.distinct == sum(len(lv.new) for lv in ref.levels[: mc.level])
    assert np.array_equal(mc.level_fps(), ar.new_fps(ref.levels[mc.level - 1]))
    rs = mc.action_constraint_results()
    assert [(r["level"], r["blocked"]) for r in rs] == [(lv.level, lv.blocked) for lv in ref.levels[1: mc.level]]
    m2, mc2, w2 = _checker(vt, "quiet-3121", frontier_words=1 << 15, frontier_states=1 << 12)
    assert mc2.check() == "constraint-out-of-room" and "not constrained" in mc2.stopped


# ---------------------------------------------------------------------------------------------------------------------
# 11. queries on the constrained model; every trace takes permitted steps only
# ---------------------------------------------------------------------------------------------------------------------
COMMITTED = r"Committed == \E r \in replicas : rep_commit_number[r] >= 1"


def _committed(s):
    return any(c >= 1 for c in s["rep_commit_number"])


def _check_trace(tr, key, fp=None):
    which, R, C, n, L, _text, pred = CASES[key][:7]
    orc, unpack, make_pm = ar.oracle_of(which)
    P, PM = ar.params_of(which, R, C, n, L), make_pm(R, C, n, L)
    assert tr[0][0] == "Initial predicate" and orc.fingerprint(P, tr[0][1])[0] == orc.fingerprint(P, orc.init_record(P))[0]
    import vsr_tlaplus_amd as vt
    for t in range(1, len(tr)):
        succ = [(vt.ACTION_NAMES[s["action"]], s["fp"]) for s in orc.successors(P, tr[t - 1][1])]
        assert (tr[t][0], orc.fingerprint(P, tr[t][1])[0]) in succ, t                  # the step exists, with that action
        p, c = (unpack(PM, [int(x) for x in r]) for r in (tr[t - 1][1], tr[t][1]))
        assert pred(p, c, tr[t][0]), (t, tr[t][0])                                      # ... and it is a permitted one
    if fp is not None:
        assert orc.fingerprint(P, tr[-1][1])[0] == fp
    return [unpack(PM, [int(x) for x in rec]) for _a, rec in tr]


@pytest.mark.parametrize("how", ["never", "reach"])
def test_queries_and_traces_on_the_constrained_model(vt, refs, how):
    key = "quiet-2122"
    ref = refs(key)
    orc, unpack, make_pm = ar.oracle_of("first")
    PM = make_pm(2, 1, 2, 2)
    first = next(lv for lv in ref.levels if any(_committed(unpack(PM, [int(x) for x in rec])) for rec in lv.new.values()))
    want_fp = min(fp for fp, rec in first.new.items() if _committed(unpack(PM, [int(x) for x in rec])))
    m, mc, w = _checker(vt, key)
    q = m.compile_predicates(COMMITTED)
    assert mc.run(**{how: q}) == ("violation" if how == "never" else "reached")
    assert (mc.witness["level"], mc.witness["fp"]) == (first.level, want_fp)
    states = _check_trace(mc.witness_trace(), key, want_fp)
    assert len(states) == first.level and _committed(states[-1]) and not any(_committed(s) for s in states[:-1])
    _check_trace(mc.trace(mc.level, mc.witness["index"]), key, want_fp)
    # every state of the level: its behaviour takes permitted steps only (the rescued ones included — their blocked edge must not be in it)
    for fp in sorted(first.new)[:48] + sorted(first.rescued):
        _check_trace(mc.trace_fp(first.level, fp), key, fp)


def test_traces_of_rescued_states(vt, refs):
    """every rescued state has a blocked edge from a state of the level before: the behaviour into it must not end with that edge"""
    key = "quiet-3121"
    ref = refs(key)
    m, mc, w = _checker(vt, key)
    target = max((lv for lv in ref.levels if lv.rescued), key=lambda lv: lv.level)
    for _ in range(target.level - 1):
        mc.step()
    assert mc.level == target.level
    for fp in sorted(target.rescued)[:8]:
        _check_trace(mc.trace_fp(target.level, fp), key, fp)


def _run_cli(args):
    return subprocess.run([CLI] + args + ["-noTLA", "-tableLog2", "18", "-frontierGiB", "0.05"], capture_output=True, text=True, timeout=300)


def test_cli_dumped_trace_validates(vt, refs, tmp_path):
    from test_host_cpu import _cfg
    ref = refs("quiet-2122")
    orc, unpack, make_pm = ar.oracle_of("first")
    PM = make_pm(2, 1, 2, 2)
    first = next(lv for lv in ref.levels if any(_committed(unpack(PM, [int(x) for x in rec])) for rec in lv.new.values()))
    cfg = _cfg(tmp_path, R=2, vals="v1, v2", L=2)
    preds = tmp_path / "preds.txt"
    preds.write_text("NothingCommitted == ~(" + COMMITTED.split("== ", 1)[1] + ")\n")
    out = str(tmp_path / "trace.tla")
    r = _run_cli(["-config", cfg, "-steps", EXAMPLE, "-actionConstraint", "QuietClient", "-predicates", str(preds), "-invariant", "NothingCommitted",
                  "-dumpTrace", "tla", out])
    assert r.returncode == 12 and "Error: Invariant NothingCommitted is violated." in r.stdout, r.stdout[-3000:] + r.stderr
    v = _run_cli(["-config", cfg, "-validateTrace", out])
    assert v.returncode == 0 and ("%d states read" % first.level) in v.stdout and "The trace is a behaviour of the model." in v.stdout, v.stdout + v.stderr


# ---------------------------------------------------------------------------------------------------------------------
# 12. the analysis models
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["shrinks-second", "shrinks-third"])
def test_analysis_models(vt, refs, key):
    ref = refs(key)
    assert ref.blocked >= 20 and ref.states >= 10000
    m, mc, w = _checker(vt, key, frontier_words=1 << 24, frontier_states=1 << 18)
    _walk(vt, mc, ref)
    assert mc.seen_set_load()[0] == mc.distinct == ref.states


# ---------------------------------------------------------------------------------------------------------------------
# 13. refusals; a detached checker is the plain checker again
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_detach(vt, refs, tmp_path):
    import ctypes as C
    from vsr_tlaplus_amd import capi
    m = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
    w = m.compile_step_predicates(ar.TEXTS["QuietClient"])

    def refused(f, code, needle):
        with pytest.raises(vt.VsrmcError) as e:
            f()
        assert e.value.code == code and needle in e.value.message, (e.value.code, e.value.message)

    mc = vt.ModelChecker(m, device=0, **SIZES)
    refused(lambda: mc.action_constrain(m.compile_predicates(cr.TEXTS["True"])), -1, "a state program")
    refused(lambda: mc.action_constrain(vt.Model.from_constants(R=3, C_=1, n=2, L=1).compile_step_predicates(ar.TEXTS["True"])), -1, "compiled for another model")
    refused(lambda: mc.action_constrain(w, 3), -1, "exports no predicate of that index")
    refused(lambda: mc.action_constrain(m.compile_step_predicates("A == aux_svc' = aux_svc")), -1, "outside VIEW")
    refused(lambda: mc.action_constrain(m.compile_step_predicates("A == aux_svc < 2")), -1, "outside VIEW")
    refused(lambda: mc.action_constrain(m.compile_step_predicates(r"A == \A v \in Values : ~aux_client_acked'[v]")), -1, "outside VIEW")
    assert mc.step()["n_new"] > 0 and mc.distinct > 1                                  # (nothing was attached by the refused calls)
    refused(lambda: mc.action_constrain(w), -6, "at level 1 only")
    mc.reset()
    mc.action_constrain(w)
    refused(lambda: mc.action_constrain(w), -6, "attached already")
    mc.step()
    refused(mc.deepen, -6, "not constrained")
    refused(mc.probe, -6, "not constrained")
    for name in ("vsrmc_checker_probe2", "vsrmc_checker_probe3"):
        infos = [capi.LevelInfo() for _ in range(3)]
        rc = getattr(vt.load(), name)(mc._h, *[C.byref(i) for i in infos[: 2 if name.endswith("2") else 3]])
        assert rc == -6 and "not constrained" in vt.load().vsrmc_last_error().decode(), name
    refused(lambda: mc.deep_attach(m.compile_predicates(cr.TEXTS["True"]), None), -6, "not constrained")
    refused(lambda: mc.save(str(tmp_path / "chk")), -6, "does not name it")
    assert not os.path.exists(str(tmp_path / "chk"))
    # attached deep programs refuse the attachment
    mc3 = vt.ModelChecker(m, device=0, **SIZES)
    mc3.deep_attach(m.compile_predicates(cr.TEXTS["True"]), None)
    refused(lambda: mc3.action_constrain(w), -6, "vsrmc_checker_deep_attach")
    # exact_ties = 1
    mc4 = vt.ModelChecker(m, device=0, exact_ties=True, **SIZES)
    refused(lambda: mc4.action_constrain(w), -6, "exact_ties")
    # a sharded checker (world 2, one rank of it)
    o = capi.Options()
    vt.load().vsrmc_options_default(C.byref(o))
    o.table_log2, o.frontier_words, o.frontier_states, o.pending_entries, o.world, o.rank = 18, 1 << 20, 1 << 14, 1 << 15, 2, 0
    h = C.c_void_p()
    capi.check(vt.load().vsrmc_checker_create(m._h, C.byref(o), C.byref(h)))
    try:
        assert vt.load().vsrmc_checker_action_constrain_attach(h, w._h, 0) == -6 and "sharded" in vt.load().vsrmc_last_error().decode()
    finally:
        vt.load().vsrmc_checker_destroy(h)
    # detached, in the middle of a search (no reset first): the checker starts over and is the plain checker
    assert mc.level == 2 and mc.distinct > 1
    mc.action_constrain(None)
    assert (mc.level, mc.distinct) == (1, 1)
    plain = refs("true-2122")
    for lv in plain.levels[1:]:
        d = mc.step()
        assert (d["n_new"], d["generated"]) == (len(lv.new), lv.generated), lv.level
        if lv.new:
            assert np.array_equal(mc.level_fps(), ar.new_fps(lv))
    assert mc.distinct == plain.states
    with pytest.raises(ValueError):
        mc.action_constraint_results()


# ---------------------------------------------------------------------------------------------------------------------
# 15. step queries on a constrained checker judge the transitions of the model only (k_step_keep): the scan neither counts nor lists a blocked one, and the
#     behaviour into a step witness ends with a permitted step
# ---------------------------------------------------------------------------------------------------------------------
STEP_QUERIES = "Lowers == ~(" + sr.COMMIT_MONOTONIC + ")\nIsReceiveSV == step_action = ReceiveSV"


def test_step_scan_of_a_constrained_checker(vt, refs):
    key = "commit-3111"
    ref = refs(key)
    first = next(lv for lv in ref.levels if lv.blocked)                                # the first level a blocked transition leads into
    assert first.blocked_act == {"ReceiveSV": first.blocked} and first.act_generated["ReceiveSV"] > first.blocked
    m, mc, w = _checker(vt, key)
    q = m.compile_step_predicates(STEP_QUERIES)
    plain = vt.ModelChecker(m, device=0, **SIZES)
    for _ in range(first.level - 2):
        mc.step()
        plain.step()
    # the level before `first`: the same states in both searches (nothing was blocked so far); the plain scan sees the steps that lower a commit number ..
    assert np.array_equal(mc.level_fps(), plain.level_fps())
    tp = plain.step_scan(q)
    assert tp["count"] == [first.blocked, first.act_generated["ReceiveSV"]] and tp["n_pairs"] + tp["n_err"] == first.generated
    # .. the constrained one does not: they are not transitions of the model
    for lv in ref.levels[first.level - 1:]:
        t = mc.step_scan(q)
        print("level %d: pairs %d Lowers %d IsReceiveSV %d" % (t["level"], t["n_pairs"], t["count"][0], t["count"][1]))
        assert t["level"] == lv.level - 1 and t["n_pairs"] + t["n_err"] == lv.generated - lv.blocked
        assert t["count"] == [0, lv.act_generated.get("ReceiveSV", 0) - lv.blocked_act.get("ReceiveSV", 0)] and t["min_fp"][0] is None
        fps, ords, bits = mc.step_pairs()
        assert len(fps) == t["count"][1] and all(b == 2 for b in bits)
        assert t["min_fp"][1] == (min(int(f) for f in fps) if len(fps) else None)
        d = mc.step()
        assert (d["n_new"], d["generated"]) == (len(lv.new), lv.generated)


@pytest.mark.parametrize("how", ["step_never", "step_reach"])
def test_step_witness_takes_permitted_steps_only(vt, refs, how):
    key = "commit-3111"
    ref = refs(key)
    m, mc, w = _checker(vt, key)
    q = m.compile_step_predicates("IsReceiveSV == step_action = ReceiveSV")
    want = next(lv for lv in ref.levels if lv.act_generated.get("ReceiveSV", 0) - lv.blocked_act.get("ReceiveSV", 0) > 0)
    assert mc.run(**{how: q}) == ("violation" if how == "step_never" else "reached")
    assert mc.witness["level"] == want.level - 1 and mc.witness["action"] == "ReceiveSV"
    tr = mc.step_witness_trace()
    assert len(tr) == want.level and tr[-1][0] == "ReceiveSV"
    _check_trace(tr, key)
    # ... and at the first level with blocked ReceiveSV steps: the witness pair of that level's scan is a permitted one
    first = next(lv for lv in ref.levels if lv.blocked)
    mc.reset()
    for _ in range(first.level - 2):
        mc.step()
    t = mc.step_scan(q)
    mc.witness = dict(level=t["level"], k=0, name="IsReceiveSV", fp=t["min_fp"][0], index=t["min_index"][0], kind="reached", ordinal=t["min_ordinal"][0],
                      action=vt.ACTION_NAMES[t["min_action"][0]])
    tr = mc.step_witness_trace()
    assert len(tr) == first.level and tr[-1][0] == "ReceiveSV"
    _check_trace(tr, key)


def test_cli_step_invariant_on_the_constrained_model(vt, refs, tmp_path):
    """-stepInvariant CommitNeverDecreases holds on the model -actionConstraint CommitNeverDecreases leaves, and fails without the constraint"""
    from test_host_cpu import _cfg
    cfg = _cfg(tmp_path, R=3, vals="v1", L=1)
    args = ["-config", cfg, "-steps", EXAMPLE, "-stepInvariant", "CommitNeverDecreases", "-maxDepth", "14"]
    r = _run_cli(args)
    assert r.returncode == 12 and "Error: Action property CommitNeverDecreases is violated." in r.stdout, r.stdout[-2000:] + r.stderr
    r = _run_cli(args + ["-actionConstraint", "CommitNeverDecreases"])
    assert r.returncode == 0 and "is violated" not in r.stdout, r.stdout[-2000:] + r.stderr
    ref = refs("commit-3111")
    assert ("ActionConstraint(13): %d of %d transitions were not taken" % (ref.levels[12].blocked, ref.levels[12].generated)) in r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# 14. the CLI end to end, on case 1
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_rows_and_closing_line(vt, refs, tmp_path):
    from test_host_cpu import _cfg
    ref = refs("quiet-2122")
    cfg = _cfg(tmp_path, R=2, vals="v1, v2", L=2)
    args = ["-config", cfg, "-steps", EXAMPLE, "-actionConstraint", "QuietClient"]
    r = _run_cli(args)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr)
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("ActionConstraint(")]
    assert rows == ["ActionConstraint(%d): %d of %d transitions were not taken, %d taken, %d new states." % (lv.level, lv.blocked, lv.generated, lv.generated - lv.blocked, len(lv.new))
                    for lv in ref.levels[1:]]
    prog = [ln for ln in r.stdout.splitlines() if ln.startswith("Progress(")]
    distinct, generated = 1, 0
    for ln, lv in zip(prog, [lv for lv in ref.levels[1:] if lv.new]):
        distinct += len(lv.new)
        generated += lv.generated
        assert ln.startswith("Progress(%d): %d states generated, %d distinct states found, %d states left on queue." % (lv.level, generated, distinct, len(lv.new))), ln
    assert "Model checking completed. No error has been found." in r.stdout
    total = {}
    for lv in ref.levels:
        for a, n in lv.blocked_act.items():
            total[a] = total.get(a, 0) + n
    per = ", ".join("%s: %d" % (a, total[a]) for a in vt.ACTION_NAMES if a in total)
    assert ("ACTION_CONSTRAINT QuietClient: %d transitions were not taken (per action: %s)" % (ref.blocked, per)) in r.stdout, r.stdout[-1500:]
    assert ("%d distinct states found, 0 states left on queue." % ref.states) in r.stdout
    assert ("The depth of the complete state graph search is %d." % ref.depth) in r.stdout
    rj = _run_cli(args + ["-json"])
    assert rj.returncode == 0
    objs = [json.loads(ln) for ln in rj.stdout.splitlines() if ln.startswith("{\"level\"")]
    assert [(o["new"], o["generated"], o["blocked"], o["permitted"]) for o in objs] == [(len(lv.new), lv.generated, lv.blocked, lv.generated - lv.blocked) for lv in ref.levels[1:]]
