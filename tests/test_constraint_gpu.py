"""State constraints on the GPU (`-m gpu`): k_constrain through ModelChecker.constrain / step / run / constraint_results / constraint_pruned and the CLI,
against tests/constraint_reference.py — a Python BFS over the CPU oracles' successor function with the constraint as a hand-written Python function
(the reference is never the parser).  Every figure is recomputed from the oracle here; a reference is computed once per space and shared."""
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
# key -> (model, R, C, n, L, constraint name, Python constraint, level cap, with the unconstrained search)
CASES = {
    "narrow-2122": ("first", 2, 1, 2, 2, "NarrowNetwork", cr.narrow_network, None, True),
    "r3normal-3121": ("first", 3, 1, 2, 1, "Replica3Normal", cr.replica3_normal, None, False),
    "r3normal-3111": ("first", 3, 1, 1, 1, "Replica3Normal", cr.replica3_normal, None, False),
    "nost-second": ("second", 3, 0, 2, 1, "NoStateTransfer", cr.no_state_transfer, 12, False),
    "nost-third": ("third", 3, 0, 2, 1, "NoStateTransfer", cr.no_state_transfer, 12, False),
    "true-2122": ("first", 2, 1, 2, 2, "True", lambda s: True, None, False),
    "initonly-2122": ("first", 2, 1, 2, 2, "InitOnly", cr.init_only, None, False),
    "false-2122": ("first", 2, 1, 2, 2, "False", lambda s: False, None, False),
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
            which, R, C, n, L, _name, fn, cap, plain = CASES[key]
            cache[key] = cr.constrained_bfs(which, R, C, n, L, fn, max_levels=cap, with_unconstrained=plain)
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
    w = m.compile_predicates(cr.TEXTS[CASES[key][5]])
    mc.constrain(w)
    return m, mc, w


def _walk(mc, ref, whole=True):
    """step the constrained checker level by level beside the reference; -> every in-model fingerprint seen in a level"""
    init = ref.levels[0]
    assert mc.distinct == len(init.kept) and mc.n_frontier == len(init.kept)
    r1 = mc.constraint_results(1)
    assert (r1["kept"], r1["pruned"], r1["n_states"]) == (len(init.kept), len(init.pruned), 1)
    seen = set(init.kept)
    distinct = len(init.kept)
    for lv in ref.levels[1:]:
        d = mc.step()
        distinct += len(lv.kept)
        assert (d["n_new"], d["generated"], d["distinct"]) == (len(lv.kept), lv.generated, distinct), (lv.level, d["n_new"], d["generated"], d["distinct"])
        ci = mc.constraint_results(lv.level)
        x, s = cr.xor_sum(lv.kept)
        assert (ci["kept"], ci["pruned"], ci["n_states"]) == (len(lv.kept), len(lv.pruned), len(lv.kept) + len(lv.pruned)), lv.level
        assert (ci["kept_xor"], ci["kept_sum"]) == (x, s), lv.level
        assert ci["pruned_min_fp"] == (min(lv.pruned) if lv.pruned else None)
        assert np.array_equal(mc.constraint_pruned(), cr.fps_of(lv.pruned)), lv.level
        if lv.kept:
            assert d["level"] == lv.level
            assert np.array_equal(mc.level_fps(), cr.fps_of(lv.kept)), lv.level
            assert mc.level_checksum() == (x, s, len(lv.kept)), lv.level          # a second pass over the filtered level gives the kernel's own figures
            seen |= set(int(f) for f in mc.level_fps())
        else:
            assert d["level"] == lv.level - 1 and mc.n_frontier == 0                # nothing of the level is in the model: the checker stays at the level before
    if whole:
        d = mc.step()
        assert d["n_new"] == 0 and d["level"] == ref.depth and d["distinct"] == ref.in_model == mc.distinct
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# 1. whole spaces, level by level; run() ends "exhausted" at the reference's depth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["narrow-2122", "r3normal-3121", "r3normal-3111"])
def test_constrained_search_equals_the_reference(vt, refs, key):
    ref = refs(key)
    assert ref.in_model >= 100 and ref.pruned_total >= 20                          # (the floors of test_constraint_cpu.py: no empty case)
    m, mc, w = _checker(vt, key)
    seen = _walk(mc, ref)
    assert seen == set(fp for lv in ref.levels for fp in lv.kept)
    if ref.unreachable is not None:                                                # satisfying, reachable, but only through out-of-model states: never reached
        assert len(ref.unreachable) >= 100 and not (seen & ref.unreachable)
        assert not any(fp in ref.unreachable for lv in ref.levels for fp in lv.pruned)
    mc.reset()
    assert mc.run() == "exhausted"
    assert (mc.depth, mc.distinct) == (ref.depth, ref.in_model)
    rs = mc.constraint_results()
    assert [(r["level"], r["kept"], r["pruned"]) for r in rs] == [(lv.level, len(lv.kept), len(lv.pruned)) for lv in ref.levels]
    assert all(r["kernel_ms"] > 0 for r in rs)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the same run through the other level scheme, through levels with holes, through several trips of the grid-stride loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["exact_ties", "holes", "grid1"])
def test_variants_give_identical_figures(vt, refs, monkeypatch, variant):
    key = "r3normal-3121"
    ref = refs(key)
    kw = {}
    if variant == "exact_ties":
        kw = dict(exact_ties=True)
    if variant == "holes":
        kw = dict(frontier_words=1 << 19, frontier_states=1 << 14)
    if variant == "grid1":
        monkeypatch.setenv("VSRMC_CONSTRAIN_GRID", "1")
    m, mc, w = _checker(vt, key, **kw)
    if variant == "holes":                                                         # walk to the largest level and look at its index range first
        big = max(ref.levels, key=lambda lv: len(lv.kept))
        for _ in range(big.level - 1):
            mc.step()
        idx = [mc.find_fp(int(fp)) for fp in list(big.kept)[:64]]
        assert None not in idx and max(idx) >= len(big.kept) + len(big.pruned), "the level has no holes: the index range is dense"
        assert all(mc.find_fp(int(fp)) is None for fp in list(big.pruned)[:16])   # a pruned state has left the level
        mc.reset()
    _walk(mc, ref)


# ---------------------------------------------------------------------------------------------------------------------
# 3. degenerate constraints, and reset
# ---------------------------------------------------------------------------------------------------------------------
def test_true_prunes_nothing_and_changes_nothing(vt, refs):
    m, mc, w = _checker(vt, "true-2122")
    plain = vt.ModelChecker(m, device=0, **SIZES)
    keys = ("level", "generated", "n_new", "distinct", "total_generated", "deadlocks", "max_bag", "record_words", "viol_mask", "act_generated")      # (frontier and words_new are index / word RANGES, chunk slack included: they depend on which blocks drew chunks)
    for round_ in range(2):
        while True:
            assert np.array_equal(mc.level_fps(), plain.level_fps())
            assert mc.level_checksum() == plain.level_checksum()
            a, b = mc.step(), plain.step()
            assert {k: a[k] for k in keys} == {k: b[k] for k in keys}, a["level"]
            if a["n_new"] == 0:
                break
        assert sum(r["pruned"] for r in mc.constraint_results()) == 0
        assert mc.distinct == refs("true-2122").in_model
        mc.reset()
        plain.reset()


def test_init_only_init_out_of_model_and_reset(vt, refs):
    for round_ in range(2):
        m, mc, w = _checker(vt, "initonly-2122") if round_ == 0 else (m, mc, w)
        ref = refs("initonly-2122")
        assert ref.in_model == 1 and len(ref.levels) == 2
        _walk(mc, ref)
        assert (mc.level, mc.distinct) == (1, 1)
        mc.reset()
        assert mc.run() == "exhausted" and (mc.depth, mc.distinct) == (1, 1)
        mc.reset()
    m0, mc0, w0 = _checker(vt, "false-2122")
    for round_ in range(2):
        assert (mc0.distinct, mc0.n_frontier) == (0, 0)
        r1 = mc0.constraint_results(1)
        assert (r1["kept"], r1["pruned"]) == (0, 1) and len(mc0.constraint_pruned()) == 1
        d = mc0.step()
        assert (d["n_new"], d["generated"], d["distinct"], d["level"]) == (0, 0, 0, 1)
        mc0.reset()
        assert mc0.run() == "exhausted" and mc0.distinct == 0
        mc0.reset()


# ---------------------------------------------------------------------------------------------------------------------
# 4. a trace into the deepest level: a behaviour of the spec, every state of it in the model
# ---------------------------------------------------------------------------------------------------------------------
def test_trace_stays_in_the_model(vt, refs):
    key = "r3normal-3121"
    ref = refs(key)
    orc, unpack, make_pm = cr.oracle_of("first")
    P, PM = cr.params_of("first", 3, 1, 2, 1), make_pm(3, 1, 2, 1)
    m, mc, w = _checker(vt, key)
    for _ in range(ref.depth - 1):
        mc.step()
    assert mc.level == ref.depth
    fp = int(mc.level_fps()[-1])
    tr = mc.trace_fp(ref.depth, fp)
    assert len(tr) == ref.depth and orc.fingerprint(P, tr[-1][1])[0] == fp
    assert orc.fingerprint(P, tr[0][1])[0] == orc.fingerprint(P, orc.init_record(P))[0]
    for t in range(1, len(tr)):                                                    # the oracle accepts every step
        assert orc.fingerprint(P, tr[t][1])[0] in set(s["fp"] for s in orc.successors(P, tr[t - 1][1])), t
    for t, (_act, rec) in enumerate(tr):
        assert cr.replica3_normal(unpack(PM, [int(x) for x in rec])), t
        assert orc.fingerprint(P, rec)[0] in ref.levels[t].kept, t                 # ... and level t + 1 of the constrained search holds state t


# ---------------------------------------------------------------------------------------------------------------------
# 5. a pruned list that overflows
# ---------------------------------------------------------------------------------------------------------------------
def test_pruned_list_overflow_keeps_counts_exact(vt, refs, monkeypatch):
    key = "r3normal-3121"
    ref = refs(key)
    lv = next(lv for lv in ref.levels if len(lv.pruned) > 8)
    monkeypatch.setenv("VSRMC_WHERE_LIST_CAP", "3")
    m, mc, w = _checker(vt, key)
    for _ in range(lv.level - 1):
        d = mc.step()
    with pytest.raises(vt.VsrmcError) as e:
        mc.constraint_pruned()
    assert e.value.code == -5 and ("has %d pruned states" % len(lv.pruned)) in e.value.message and "holds the 3 " in e.value.message
    ci = mc.constraint_results(lv.level)
    assert (ci["kept"], ci["pruned"], ci["pruned_min_fp"]) == (len(lv.kept), len(lv.pruned), min(lv.pruned))
    assert d["n_new"] == len(lv.kept) and np.array_equal(mc.level_fps(), cr.fps_of(lv.kept))


# ---------------------------------------------------------------------------------------------------------------------
# 6. a user's invariant that first fails on an out-of-model state
# ---------------------------------------------------------------------------------------------------------------------
def _first_pruned_violation(ref):
    orc, unpack, make_pm = cr.oracle_of("first")
    PM = make_pm(3, 1, 2, 1)
    for lv in ref.levels:
        bad = [fp for fp, rec in lv.pruned.items() if not cr.not_all_in_view_change(unpack(PM, [int(x) for x in rec]))]
        if bad:
            return lv.level, min(bad), len(bad)
    return None


def test_invariant_violated_among_the_pruned_states(vt, refs):
    key = "r3normal-3121"
    ref = refs(key)
    level, fp, count = _first_pruned_violation(ref)
    orc, unpack, make_pm = cr.oracle_of("first")
    P, PM = cr.params_of("first", 3, 1, 2, 1), make_pm(3, 1, 2, 1)
    for lv in ref.levels[:level]:                                                  # the reference finds the level: no in-model state violates it up to there
        assert all(cr.not_all_in_view_change(unpack(PM, [int(x) for x in rec])) for rec in lv.kept.values()), lv.level
    m = _model(vt, key)
    mc = vt.ModelChecker(m, device=0, **SIZES)
    bad_text = r"Bad == \A r \in replicas : rep_status[r] = ViewChange"
    w = m.compile_predicates(cr.TEXTS["Replica3Normal"] + "\n" + bad_text)
    never = m.compile_predicates(bad_text)
    mc.constrain(w, "Replica3Normal")
    assert mc.run(never=never) == "violation"
    wit = mc.witness
    assert (wit["level"], wit["fp"], wit["name"], wit.get("pruned")) == (level, fp, "Bad", True)
    assert mc.constraint_results(level)["pruned_count"] == {"Replica3Normal": 0, "Bad": count}
    tr = mc.witness_trace()                                                        # the violation is reported with that state's behaviour
    assert len(tr) == level and orc.fingerprint(P, tr[-1][1])[0] == fp
    states = [unpack(PM, [int(x) for x in rec]) for _a, rec in tr]
    assert all(cr.replica3_normal(s) and cr.not_all_in_view_change(s) for s in states[:-1])
    assert not cr.replica3_normal(states[-1]) and not cr.not_all_in_view_change(states[-1])
    for t in range(1, len(tr)):
        assert orc.fingerprint(P, tr[t][1])[0] in set(s["fp"] for s in orc.successors(P, tr[t - 1][1])), t


# ---------------------------------------------------------------------------------------------------------------------
# 7. the analysis models
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["nost-second", "nost-third"])
def test_analysis_models(vt, refs, key):
    ref = refs(key)
    assert ref.pruned_total >= 5 and ref.in_model >= 10000
    m, mc, w = _checker(vt, key, frontier_words=1 << 24, frontier_states=1 << 18)
    _walk(mc, ref, whole=False)


# ---------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(vt, tmp_path):
    import ctypes as C
    from vsr_tlaplus_amd import capi
    m = vt.Model.from_constants(R=3, C_=1, n=2, L=1)
    w = m.compile_predicates(cr.TEXTS["Replica3Normal"])

    def refused(f, code, needle):
        with pytest.raises(vt.VsrmcError) as e:
            f()
        assert e.value.code == code and needle in e.value.message, (e.value.code, e.value.message)

    mc = vt.ModelChecker(m, device=0, **SIZES)
    refused(lambda: mc.constrain(m.compile_step("Mono == \\A r \\in replicas : rep_view_number'[r] >= rep_view_number[r]")), -1, "a step program")
    refused(lambda: mc.constrain(vt.Model.from_constants(R=2, C_=1, n=2, L=2).compile_predicates(cr.TEXTS["True"])), -1, "compiled for another model")
    refused(lambda: mc.constrain(w, 3), -1, "exports no predicate of that index")
    refused(lambda: mc.constrain(m.compile_predicates("A == aux_svc < 2")), -1, "outside VIEW")
    refused(lambda: mc.constrain(m.compile_predicates(r"A == \A v \in Values : ~aux_client_acked[v]")), -1, "outside VIEW")
    assert mc.step()["n_new"] > 0 and mc.distinct > 1                              # (nothing was attached by the refused calls)
    refused(lambda: mc.constrain(w), -6, "at level 1 only")
    mc.reset()
    mc.constrain(w)
    refused(lambda: mc.constrain(w), -6, "attached already")
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
    # a sharded checker (world 2, one rank of it)
    o = capi.Options()
    vt.load().vsrmc_options_default(C.byref(o))
    o.table_log2, o.frontier_words, o.frontier_states, o.pending_entries, o.world, o.rank = 18, 1 << 20, 1 << 14, 1 << 15, 2, 0
    h = C.c_void_p()
    capi.check(vt.load().vsrmc_checker_create(m._h, C.byref(o), C.byref(h)))
    try:
        assert vt.load().vsrmc_checker_constrain_attach(h, w._h, 0) == -6 and "sharded" in vt.load().vsrmc_last_error().decode()
    finally:
        vt.load().vsrmc_checker_destroy(h)


def test_out_of_room_ends_the_run(vt, refs):
    """record buffers the search outgrows: the run ends with the stop of its own, nothing goes on unconstrained"""
    key = "r3normal-3121"
    m, mc, w = _checker(vt, key, frontier_words=1 << 15, frontier_states=1 << 12)
    assert mc.run() == "constraint-out-of-room"
    assert "not constrained" in mc.stopped and 1 < mc.distinct < refs(key).in_model
    m2, mc2, w2 = _checker(vt, key, frontier_words=1 << 15, frontier_states=1 << 12)
    assert mc2.check() == "constraint-out-of-room" and "not constrained" in mc2.stopped


# ---------------------------------------------------------------------------------------------------------------------
# 9. the CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_rows_and_closing_line(vt, refs, tmp_path):
    ref = refs("narrow-2122")
    cfg = tmp_path / "VSR.cfg"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_cfg.py"), str(cfg), "2", "1", "v1, v2", "2"], check=True)
    args = [CLI, "-config", str(cfg), "-noTLA", "-tableLog2", "18", "-frontierGiB", "0.05", "-predicates", os.path.join(ROOT, "tools", "constraints_example.txt"),
            "-constraint", "NarrowNetwork"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr)
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("Progress(")]
    kept_levels = [lv for lv in ref.levels[1:] if lv.kept]
    assert len(rows) == len(kept_levels)
    distinct, generated = len(ref.levels[0].kept), 0
    for ln, lv in zip(rows, kept_levels):
        distinct += len(lv.kept)
        generated += lv.generated
        assert ln.startswith("Progress(%d): %d states generated, %d distinct states found, %d states left on queue." % (lv.level, generated, distinct, len(lv.kept))), ln
    assert "Model checking completed. No error has been found." in r.stdout
    assert ("CONSTRAINT NarrowNetwork: %d states were out of model and not explored" % ref.pruned_total) in r.stdout
    assert ("%d distinct states found, 0 states left on queue." % ref.in_model) in r.stdout
    assert ("The depth of the complete state graph search is %d." % ref.depth) in r.stdout
    r = subprocess.run(args + ["-json"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr)
    objs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{\"level\"")]
    by_level = {lv.level: lv for lv in ref.levels}
    got = [(o["level"], o["new"], o["kept"], o["pruned"], o["generated"]) for o in objs if o["kept"] or o["pruned"]]
    assert got == [(lv.level if lv.kept else lv.level - 1, len(lv.kept), len(lv.kept), len(lv.pruned), lv.generated) for lv in ref.levels[1:]]
    assert objs[-1]["new"] == 0 and by_level


def _printed_behaviour(m, stdout):
    """the states a CLI run printed after "The behavior up to this point is:" -> [(action name, wire record)]"""
    import re
    body = stdout.split("The behavior up to this point is:\n", 1)[1]
    parts = re.split(r"State \d+: <([^>]*)>\n", body)[1:]
    return [(act, m.parse_states(text.split("\n\n")[0])[0][1]) for act, text in zip(parts[0::2], parts[1::2])]


def test_cli_invariant_violated_among_the_pruned_states(vt, refs, tmp_path):
    """`-constraint Replica3Normal -invariant NotAllInViewChange`: the CLI's own path (a combined program, the per-export figures over the pruned states)"""
    key = "r3normal-3121"
    ref = refs(key)
    level, fp, count = _first_pruned_violation(ref)
    orc, unpack, make_pm = cr.oracle_of("first")
    P, PM = cr.params_of("first", 3, 1, 2, 1), make_pm(3, 1, 2, 1)
    m = _model(vt, key)
    cfg = tmp_path / "VSR.cfg"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_cfg.py"), str(cfg), "3", "1", "v1, v2", "1"], check=True)
    args = [CLI, "-config", str(cfg), "-noTLA", "-tableLog2", "18", "-frontierGiB", "0.05", "-predicates", os.path.join(ROOT, "tools", "constraints_example.txt"),
            "-constraint", "Replica3Normal", "-invariant", "NotAllInViewChange"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 12, (r.returncode, r.stdout[-2000:], r.stderr)
    assert ("Error: Invariant NotAllInViewChange is violated (by a state of level %d that is outside CONSTRAINT Replica3Normal)." % level) in r.stdout
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("Progress(")]
    assert len(rows) == level - 1 and rows[-1].startswith("Progress(%d):" % level)                # the run stopped at the level that pruned the violator
    tr = _printed_behaviour(m, r.stdout)
    assert len(tr) == level and tr[0][0] == "Initial predicate" and orc.fingerprint(P, tr[-1][1])[0] == fp
    states = [unpack(PM, [int(x) for x in rec]) for _a, rec in tr]
    assert all(cr.replica3_normal(s) and cr.not_all_in_view_change(s) for s in states[:-1])
    assert not cr.replica3_normal(states[-1]) and not cr.not_all_in_view_change(states[-1])
    for t in range(1, len(tr)):
        assert orc.fingerprint(P, tr[t][1])[0] in set(s["fp"] for s in orc.successors(P, tr[t - 1][1])), t
    # an invariant that holds everywhere: nothing is reported, the constrained search runs to its end
    r = subprocess.run(args[:-1] + ["ViewsBelow3"], capture_output=True, text=True, timeout=300)
    assert ("Invariant ViewsBelow3 is violated" in r.stdout) == any(not cr.views_below(3)(unpack(PM, [int(x) for x in rec]))
                                                                     for lv in ref.levels for d in (lv.kept, lv.pruned) for rec in d.values())


# ---------------------------------------------------------------------------------------------------------------------
# 10. a BUILT-IN invariant violated by an out-of-model state still gives its behaviour
# ---------------------------------------------------------------------------------------------------------------------
def test_built_in_violation_on_a_pruned_state(vt):
    ref = cr.constrained_bfs("first", 3, 1, 2, 1, cr.r3normal_commit_below2, max_levels=19, with_unconstrained=False)
    orc, unpack, make_pm = cr.oracle_of("first")
    P, PM = cr.params_of("first", 3, 1, 2, 1, invariant_mask=3), make_pm(3, 1, 2, 1)
    bad = sorted((lv.level, fp) for lv in ref.levels for fp, rec in lv.pruned.items() if orc.invariants(P, rec))
    assert bad and bad[0][0] == 19 and not any(orc.invariants(P, rec) for lv in ref.levels for rec in lv.kept.values())   # (test_constraint_cpu.py: the reference's finding)
    m = vt.Model.from_constants(R=3, C_=1, n=2, L=1, invariant_mask=3)
    w = m.compile_predicates(cr.TEXTS["R3NormalCommitBelow2"])
    for how in ("run", "check"):
        mc = vt.ModelChecker(m, device=0, **SIZES)
        mc.constrain(w)
        assert (mc.run() if how == "run" else mc.check()) == "violation"
        v = mc.violation
        assert (v["level"], v["fp"], v["mask"]) == (19, bad[0][1], 2), v                  # the smallest fingerprint among the violators, an out-of-model state
        assert mc.find_fp(v["fp"]) is None and v["fp"] in set(int(f) for f in mc.constraint_pruned())
        assert mc.distinct == sum(len(lv.kept) for lv in ref.levels)
        tr = mc.violation_trace()
        assert len(tr) == 19 and orc.fingerprint(P, tr[-1][1])[0] == v["fp"] and orc.invariants(P, tr[-1][1]) == 2
        states = [unpack(PM, [int(x) for x in rec]) for _a, rec in tr]
        assert all(cr.r3normal_commit_below2(s) for s in states[:-1]) and not cr.r3normal_commit_below2(states[-1])
        for t in range(1, len(tr)):
            assert orc.fingerprint(P, tr[t][1])[0] in set(s["fp"] for s in orc.successors(P, tr[t - 1][1])), t
        mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 11. the seen-set's load counts the pruned states: a table far too small grows by it, the figures stay the reference's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["r3normal-3111", "r3normal-3121"])
def test_small_table_grows_by_kept_plus_pruned(vt, refs, key):
    ref = refs(key)
    assert ref.pruned_total * 4 >= ref.in_model                                            # a constraint that prunes much of what it generates
    m, mc, w = _checker(vt, key, table_log2=8)
    used = 1
    for lv in ref.levels[1:]:
        assert mc.room() in (0, 1)
        # room()'s contract: when it returns 0 or 1 the load is at most 85 % of the slots (within a level it may pass that: the next call grows the table)
        assert used <= 0.85 * (1 << mc.options.table_log2), (lv.level, used, mc.options.table_log2)
        d = mc.step()
        assert (d["n_new"], d["generated"]) == (len(lv.kept), lv.generated), lv.level
        ci = mc.constraint_results(lv.level)
        assert (ci["kept"], ci["pruned"], ci["kept_xor"], ci["kept_sum"]) == (len(lv.kept), len(lv.pruned)) + cr.xor_sum(lv.kept), lv.level
        used += len(lv.kept) + len(lv.pruned)                                              # every one of them holds a slot
    assert mc.room() in (0, 1)
    assert mc.step()["n_new"] == 0 and mc.distinct == ref.in_model
    assert used == ref.in_model + ref.pruned_total and mc.options.table_log2 > 8
    assert (1 << mc.options.table_log2) * 0.85 >= used > ref.in_model                      # grown for what the table holds, not for the in-model count alone
    mc.reset()
    assert mc.run() == "exhausted" and (mc.depth, mc.distinct) == (ref.depth, ref.in_model)
