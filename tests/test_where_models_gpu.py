"""State predicates on the two analysis models on the GPU (`-m gpu`): k_where<1> / k_where<2> through Model.where_flags, ModelChecker.where_scan /
where_states / witness_trace, run(reach=, never=) and the CLI, against hand-written Python functions over pyoracle2 / pyoracle3's unpack of the CPU
oracles' records (tests/where_models_reference.py — the reference is never the parser).  Every figure is recomputed from the oracle here.

Hits / first level per predicate on (3, {v1,v2}, 1), levels 1-12, as the oracle alone gives them (asserted below):
  both models  InStateTransfer 14 / 11, GetStateToAny 22 / 11, DvcLogBelowCommit 1588 / 8, SvLogDropsEntry 546 / 9, LogDivergence 78 / 10,
               NewStateCarriesV2 2 / 12; CountedDvc 21514 / 4 (second model), 21405 / 4 (third)
  third model  AppAheadOfSomeLog 6258 / 5, TwoDvcsHeld 2848 / 7, HeldDvcShorterLog 1454 / 7"""
import collections
import json
import os
import subprocess

import numpy as np
import pytest

import where_models_reference as wm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
# (R, values, limit, levels walked (None = exhausted))
SPACES = {"321": (3, 2, 1, 12), "311": (3, 1, 1, None), "222": (2, 2, 2, None)}
SIZES = dict(table_log2=20, frontier_words=1 << 22, frontier_states=1 << 17, pending_entries=1 << 17)
REACH_SIZES = dict(table_log2=20, frontier_words=1 << 24, frontier_states=1 << 20, pending_entries=1 << 19)
Level = collections.namedtuple("Level", "level words off recs states fps")
# the issue's table for (3, {v1,v2}, 1), levels 1-12: name -> (hits, first level), per model
TABLE = {
    "second": {"InStateTransfer": (14, 11), "GetStateToAny": (22, 11), "DvcLogBelowCommit": (1588, 8), "SvLogDropsEntry": (546, 9), "LogDivergence": (78, 10),
               "CountedDvc": (21514, 4), "NewStateCarriesV2": (2, 12)},
    "third": {"InStateTransfer": (14, 11), "GetStateToAny": (22, 11), "DvcLogBelowCommit": (1588, 8), "SvLogDropsEntry": (546, 9), "LogDivergence": (78, 10),
              "CountedDvc": (21405, 4), "NewStateCarriesV2": (2, 12), "AppAheadOfSomeLog": (6258, 5), "TwoDvcsHeld": (2848, 7), "HeldDvcShorterLog": (1454, 7)},
}
N_STATES = {"second": 40360, "third": 40251}


@pytest.fixture(scope="module")
def vt():
    import vsr_tlaplus_amd as vt
    assert vt.load().vsrmc_device_count() >= 1, "no HIP device visible"
    return vt


def _oracle(which):
    from oracle import orc2, orc3, pyoracle2, pyoracle3
    return (orc2, pyoracle2) if which == "second" else (orc3, pyoracle3)


def _values(which, n):
    return tuple("v%d" % (i + 1) for i in range(n)) if which == "second" else tuple("abc"[:n])


@pytest.fixture(scope="module")
def spaces():
    """(model, key) -> (oracle params, value names, [Level]): every level of the oracle's BFS once — records, their Python view, their fingerprints;
    shared, never changed"""
    cache = {}

    def get(which, key):
        if (which, key) not in cache:
            orc, po = _oracle(which)
            R, n, L, depth = SPACES[key]
            P = orc.Params(R, n, L)
            PM = po.Model(R, _values(which, n), L)
            b = orc.Bfs(P)
            out = []
            level = 1
            init = orc.init_record(P)
            words, off = init, np.array([0, len(init)], dtype=np.uint64)
            while True:
                recs = [words[int(off[i]): int(off[i + 1])] for i in range(len(off) - 1)]
                out.append(Level(level, words, off, recs, [po.unpack(PM, [int(x) for x in r]) for r in recs], [orc.fingerprint(P, r)[0] for r in recs]))
                if (depth is not None and level >= depth) or b.step() == 0:
                    break
                level += 1
                words, off = b.frontier()
            b.close()
            cache[(which, key)] = (P, _values(which, n), out)
        return cache[(which, key)]
    return get


def _model(vt, which, key):
    R, n, L, _depth = SPACES[key]
    return (vt.Model.second_model if which == "second" else vt.Model.third_model)(R=R, n=n, L=L)


def _same_but_time(a, b):
    return {k: v for k, v in a.items() if k != "kernel_ms"} == {k: v for k, v in b.items() if k != "kernel_ms"}


def _sets(which, values):
    """[(tag, predicates, first set?)]: two compiled objects per model where more than 8 names are needed"""
    out = [("A", wm.set_a(values), True), ("B", wm.SET_B, False)]
    if which == "third":
        out += [("A3", wm.SET_A3, True), ("B3", wm.SET_B3, False)]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. state by state
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", wm.MODELS)
def test_where_flags_state_by_state(vt, spaces, which):
    seen = {}                                                   # (tag, name) -> set of verdicts
    hits = collections.Counter()
    first = {}
    n_states = collections.Counter()
    for key in sorted(SPACES):
        m = _model(vt, which, key)
        _P, values, levels = spaces(which, key)
        for tag, preds, _ in _sets(which, values):
            w = m.compile_predicates(wm.text_of(preds))
            assert w.names == [p[0] for p in preds]
            for lv in levels:
                flags = m.where_flags(w, lv.words, lv.off)
                assert len(flags) == len(lv.recs)
                n_states[(key, tag)] += len(lv.recs)
                for i, s in enumerate(lv.states):
                    want = wm.bits_of(preds, s)
                    assert int(flags[i]) == want, (which, key, tag, lv.level, i, bin(int(flags[i])), bin(want))
                    for k in range(len(preds)):
                        v = (want >> k) & 1
                        seen.setdefault((tag, preds[k][0]), set()).add(v)
                        if v:
                            hits[(key, preds[k][0])] += 1
                            first.setdefault((key, preds[k][0]), lv.level)
    for (key, name), n in sorted(hits.items()):
        print("where_flags %s model, %s %s: %d hits, first at level %d" % (which, key, name, n, first[(key, name)]))
    # the issue's table, recomputed from the oracle above
    assert n_states[("321", "A")] == N_STATES[which]
    for name, (n, lvl) in TABLE[which].items():
        assert (hits[("321", name)], first[("321", name)]) == (n, lvl), name
    # condition: every predicate of the first set saw both verdicts somewhere; of the second set at most one in eight is vacuous
    second = []
    for tag, preds, is_first in _sets(which, spaces(which, "321")[1]):
        for p in preds:
            if is_first:
                assert seen[(tag, p[0])] == {0, 1}, p[0]
            else:
                second.append(seen[(tag, p[0])] == {0, 1})
    assert 8 * second.count(False) <= len(second), second


# ---------------------------------------------------------------------------------------------------------------------
# 2. random differential
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", wm.MODELS)
def test_random_expressions(vt, spaces, which):
    m = _model(vt, which, "321")
    _P, _values_, all_levels = spaces(which, "321")
    levels = [lv for lv in all_levels if lv.level <= 11]
    words = np.concatenate([lv.words for lv in levels])
    off = [0]
    for lv in levels:
        base = off[-1]
        off.extend(base + int(x) for x in lv.off[1:])
    off = np.array(off, dtype=np.uint64)
    states = [s for lv in levels for s in lv.states]
    preds = wm.random_predicates(20261018, 3, 1, 104, third=which == "third")
    n_true = collections.Counter()
    for j in range(0, len(preds), 8):
        chunk = preds[j: j + 8]
        w = m.compile_predicates("\n".join("P%d == %s" % (k, t) for k, (t, _) in enumerate(chunk)))
        flags = m.where_flags(w, words, off)
        for k, (text, f) in enumerate(chunk):
            for i, s in enumerate(states):
                want = f(s)
                n_true[j + k] += want
                assert bool((int(flags[i]) >> k) & 1) == want, "%s model, state %d: %s is %s in the reference" % (which, i, text, want)
    used = sum(1 for k in range(len(preds)) if 0 < n_true[k] < len(states))
    print("random expressions, %s model: %d of %d have both verdicts on (3,{v1,v2},1) levels 1-11" % (which, used, len(preds)))
    assert len(preds) >= 100 and 2 * used >= len(preds)            # (the reference alone meets this: it does not depend on the kernel)


# ---------------------------------------------------------------------------------------------------------------------
# 3. inside a search
# ---------------------------------------------------------------------------------------------------------------------
def _scan_search(vt, spaces, which, key, sizes=SIZES, count_holes=False, **kw):
    orc, _po = _oracle(which)
    P, values, levels = spaces(which, key)
    preds = wm.set_a(values) if which == "second" else wm.set_a(values)[:5] + wm.SET_A3
    m = _model(vt, which, key)
    w = m.compile_predicates(wm.text_of(preds))
    mc = vt.ModelChecker(m, **dict(sizes, **kw))
    ob = orc.Bfs(P)
    holes = 0
    for lv in levels:
        want = sorted((fp, wm.bits_of(preds, s)) for fp, s in zip(lv.fps, lv.states))
        t = mc.where_scan(w)
        assert _same_but_time(t, mc.where_scan(w))                  # any number of times, nothing changes
        assert (t["level"], t["n_states"]) == (lv.level, len(lv.recs))
        if count_holes:
            holes += max(mc.find_fp(fp) for fp in lv.fps) + 1 - t["n_states"]
        fps, bits = mc.where_states()
        assert [(int(a), int(b)) for a, b in zip(fps, bits)] == [x for x in want if x[1]], lv.level
        for k in range(len(preds)):
            mine = [fp for fp, b in want if (b >> k) & 1]
            assert t["count"][k] == len(mine), (lv.level, k)
            if mine:
                assert t["min_fp"][k] == mine[0] and mc.find_fp(mine[0]) == t["min_index"][k]
            else:
                assert t["min_fp"][k] is None and t["min_index"][k] is None
        assert np.array_equal(mc.level_fps(), ob.level_fps(lv.level))   # the scan left the level as it was
        d = mc.step()
        nn = ob.step()
        assert d["n_new"] == nn and d["generated"] == ob.info["generated"], lv.level
    last = (d, mc.where_scan(w), mc.where_states())
    mc.close()
    ob.close()
    return holes, last


@pytest.mark.parametrize("which", wm.MODELS)
@pytest.mark.parametrize("key", ["222", "321"])
def test_where_scan_inside_a_search(vt, spaces, which, key):
    _holes, (d, t, (fps, _bits)) = _scan_search(vt, spaces, which, key)
    if key == "222":                                                # exhausted: the last level is empty, and scanning it says so
        n = len(t["count"])
        assert d["n_new"] == 0 and t["n_states"] == 0 and t["count"] == [0] * n and t["min_fp"] == [None] * n and len(fps) == 0


@pytest.mark.parametrize("which", wm.MODELS)
def test_where_scan_exact_ties_and_host_frontier(vt, spaces, which):
    _scan_search(vt, spaces, which, "222", exact_ties=True)
    _scan_search(vt, spaces, which, "321", host_frontier=True)


@pytest.mark.parametrize("which", wm.MODELS)
def test_where_scan_of_a_frontier_with_holes(vt, spaces, which, monkeypatch):
    """the work-list-overflow configuration of test_gpu_parity.py: every wave of k_expand publishes the unused tail of its last chunk of indices as
    withdrawn indices (refs[i] == 0), and the scan must step over them"""
    monkeypatch.setenv("VSRMC_CCAP", "256")
    holes, _ = _scan_search(vt, spaces, which, "321", sizes=dict(table_log2=20, frontier_words=1 << 24, frontier_states=1 << 20, pending_entries=1 << 19),
                            count_holes=True)
    print("withdrawn indices scanned over (%s model): %d" % (which, holes))
    assert holes > 0


@pytest.mark.parametrize("which", wm.MODELS)
def test_where_list_overflow_keeps_counters_and_minima_exact(vt, which, monkeypatch):
    m = _model(vt, which, "222")
    w = m.compile_predicates(wm.text_of(wm.set_a(_values(which, 2))))
    mc = vt.ModelChecker(m, **SIZES)
    while mc.level < 12:
        mc.step()
    full = mc.where_scan(w)
    fps, _ = mc.where_states()
    assert len(fps) > 1
    monkeypatch.setenv("VSRMC_WHERE_LIST_CAP", "1")
    assert _same_but_time(mc.where_scan(w), full)
    with pytest.raises(vt.VsrmcError) as e:
        mc.where_states()
    assert e.value.code == -5 and ("has %d" % len(fps)) in e.value.message
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. reach and witness
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", wm.MODELS)
def test_reach_stops_at_the_first_level_and_the_witness_is_a_shortest_behaviour(vt, spaces, which):
    orc, po = _oracle(which)
    P, values, levels = spaces(which, "321")
    PM = po.Model(3, values, 1)
    first = next(lv for lv in levels if any(wm.in_state_transfer(s) for s in lv.states))
    assert first.level == 11
    want_fp = min(fp for fp, s in zip(first.fps, first.states) if wm.in_state_transfer(s))
    m = _model(vt, which, "321")
    w = m.compile_predicates("InStateTransfer == " + wm.set_a(values)[0][1])
    norm = lambda r: tuple(int(x) for x in orc.normalise(P, r))   # noqa: E731
    traces = []
    # run() stores a level only while the next one is predicted to fit the record buffers (a level that is not stored is not examined): the two
    # sets of sizes both leave room for level 12 as predicted from level 11's successors per state
    for kw in (REACH_SIZES, dict(table_log2=19, frontier_words=1 << 23, frontier_states=1 << 19, pending_entries=1 << 18)):
        mc = vt.ModelChecker(m, **kw)
        assert mc.run(reach=w) == "reached", (mc.level, mc.depth)
        assert mc.level == 11 and mc.witness["level"] == 11 and mc.witness["name"] == "InStateTransfer" and mc.witness["fp"] == want_fp
        tr = mc.witness_trace()
        assert [norm(r) for _, r in mc.witness_trace("InStateTransfer")] == [norm(r) for _, r in tr]
        mc.close()
        assert len(tr) == 11 and tr[0][0] == "Initial predicate" and norm(tr[0][1]) == norm(orc.init_record(P))
        states = [po.unpack(PM, [int(x) for x in r]) for _, r in tr]
        assert po.view_of(states[0]) == po.view_of(po.Init(PM))
        for a, b in zip(states, states[1:]):                        # every consecutive pair is a (state, successor) of the Python oracle
            assert po.view_of(b) in [po.view_of(t) for _, t in po.successors(PM, a)]
        assert wm.in_state_transfer(states[-1]) and orc.fingerprint(P, tr[-1][1])[0] == want_fp
        traces.append([(a, norm(r)) for a, r in tr])
    assert traces[0] == traces[1]
    print("InStateTransfer on (3,{v1,v2},1), %s model: first at level %d, witness fingerprint %016x" % (which, first.level, want_fp))
    # never= reports a predicate that first fails at a known level like a built-in violation: DvcLogBelowCommit, level 8
    w2 = m.compile_predicates("DvcLogBelowCommit == " + wm.set_a(values)[2][1])
    lv8 = levels[7]
    fp8 = min(fp for fp, s in zip(lv8.fps, lv8.states) if wm.dvc_log_below_commit(s))
    assert not any(wm.dvc_log_below_commit(s) for lv in levels[:7] for s in lv.states)
    mc = vt.ModelChecker(m, **REACH_SIZES)
    assert mc.run(never=w2) == "violation" and mc.witness["kind"] == "violation" and mc.witness["level"] == 8 and mc.witness["fp"] == fp8
    assert len(mc.witness_trace()) == 8
    mc.close()
    mc = vt.ModelChecker(m, **REACH_SIZES)                            # the defaults scan nothing
    assert mc.run(max_depth=9) == "max-depth" and mc.witness is None
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", wm.MODELS)
def test_where_scan_is_refused_where_it_is_for_vsr_tla(vt, which):
    import ctypes as C
    from vsr_tlaplus_amd import capi
    m = _model(vt, which, "222")
    w = m.compile_predicates("TRUE")
    o = capi.Options()
    capi.load().vsrmc_options_default(C.byref(o))
    o.table_log2, o.frontier_words, o.frontier_states, o.pending_entries, o.rank, o.world = 16, 1 << 18, 1 << 13, 1 << 14, 0, 2
    h = C.c_void_p()
    capi.check(capi.load().vsrmc_checker_create(m._h, C.byref(o), C.byref(h)))
    info = capi.WhereInfo()
    assert capi.load().vsrmc_checker_where_scan(h, w._h, C.byref(info)) == -6
    assert b"sharded" in capi.load().vsrmc_last_error()
    capi.load().vsrmc_checker_destroy(h)
    mc = vt.ModelChecker(m, **SIZES)
    with pytest.raises(vt.VsrmcError) as e:
        mc.where_states()
    assert e.value.code == -6
    for _ in range(5):
        mc.step()
    t = mc.where_scan(w)
    assert t["level"] == 6 and t["count"] == [t["n_states"]]
    # another model's program — the other analysis model with the same constants, VSR.tla, other constants — and a step program
    other = _model(vt, "third" if which == "second" else "second", "222")
    vsr = vt.Model.from_constants(R=2, C_=1, n=2, L=2, symmetry=False)
    for prog in (other.compile_predicates("TRUE"), vsr.compile_predicates("TRUE"), vsr.compile_where("TRUE"), _model(vt, which, "321").compile_predicates("TRUE")):
        with pytest.raises(vt.VsrmcError) as e:
            mc.where_scan(prog)
        assert e.value.code == -1 and "compiled for another model" in e.value.message
    with pytest.raises(vt.VsrmcError) as e:
        mc.where_scan(vsr.compile_step("aux_svc' >= aux_svc"))
    assert e.value.code == -1 and "step program" in e.value.message
    for entry in (m.compile_where, m.compile_step):                 # the two older entries keep refusing the analysis models
        with pytest.raises(vt.VsrmcError) as e:
            entry("TRUE")
        assert e.value.code == -1 and e.value.message.endswith("VSR.tla only")
    mc.deepen()
    with pytest.raises(vt.VsrmcError) as e:
        mc.where_scan(w)
    assert e.value.code == -6 and "seen-set only" in e.value.message
    mc.close()
    vmc = vt.ModelChecker(vsr, **SIZES)                              # and the reverse: an analysis model's program on a VSR.tla checker
    with pytest.raises(vt.VsrmcError) as e:
        vmc.where_scan(w)
    assert e.value.code == -1 and "compiled for another model" in e.value.message
    vmc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the CLI
# ---------------------------------------------------------------------------------------------------------------------
def _run_cli(args):
    return subprocess.run([CLI] + args + ["-noTLA", "-tableLog2", "18", "-frontierGiB", "0.05"], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("which", wm.MODELS)
def test_cli_reach_invariant_and_where_report(vt, spaces, which, tmp_path):
    if which == "second":
        from test_model2_host_cpu import _cfg
    else:
        from test_model3_host_cpu import _cfg
    _P, values, levels = spaces(which, "321")
    cfg = _cfg(tmp_path, R=3, vals=", ".join(values), L=1)
    name, text, fn = wm.set_a(values)[2]                            # DvcLogBelowCommit: first at level 8
    per_level = {lv.level: sum(1 for s in lv.states if fn(s)) for lv in levels}
    first = min(k for k, v in per_level.items() if v)
    assert first == 8
    preds = tmp_path / "predicates.txt"
    preds.write_text("\\* two predicates and a helper\nLOCAL Three == 3\n%s == %s\nLogsCovered == ~%s /\\ ReplicaCount = Three\n" % (name, text, name))
    r = _run_cli(["-config", cfg, "-predicates", str(preds), "-reach", name, "-maxDepth", "12"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("State satisfying %s found at depth %d (%d of" % (name, first, per_level[first])) in r.stdout and "Error" not in r.stdout
    blocks = [ln for ln in r.stdout.splitlines() if ln.startswith("State ") and ": <" in ln]
    assert len(blocks) == first and blocks[0] == "State 1: <Initial predicate>"
    # the trace is printed by the model's own printer: its variables, a DoViewChangeMsg with its log in the last state
    assert "no_progress_ctr" in r.stdout and "rep_client_table" not in r.stdout and ("rep_app_state" in r.stdout) == (which == "third")
    assert "type |-> DoViewChangeMsg" in r.stdout.split("State %d: <" % first)[1]
    # the negation as an invariant: reported and exit-coded like a built-in one, the same behaviour
    r2 = _run_cli(["-config", cfg, "-predicates", str(preds), "-invariant", "LogsCovered", "-maxDepth", "12"])
    assert r2.returncode == 12 and "Error: Invariant LogsCovered is violated." in r2.stdout and "Error: The behavior up to this point is:" in r2.stdout
    assert [ln for ln in r2.stdout.splitlines() if ln.startswith("State ") and ": <" in ln] == blocks
    # not reachable within the depth: exit 14
    r3 = _run_cli(["-config", cfg, "-predicates", str(preds), "-reach", name, "-maxDepth", str(first - 1)])
    assert r3.returncode == 14 and ("No state satisfying %s was found" % name) in r3.stdout, r3.stdout + r3.stderr
    # the report: per-level counts, no stop
    r4 = _run_cli(["-config", cfg, "-predicates", str(preds), "-whereReport", "-json", "-maxDepth", "12"])
    assert r4.returncode == 0, r4.stdout + r4.stderr
    rows = [json.loads(ln) for ln in r4.stdout.splitlines() if ln.startswith("{")]
    got = {}
    for row in rows:                                                # line k is the step that expands level k - 1; the last level has a line of its own
        assert set(row["where"]) == {name, "LogsCovered"}
        got[row["level"] if row.get("expanded") is False else row["level"] - 1] = row["where"]
    assert {k: v[name] for k, v in got.items()} == per_level
    assert all(v[name] + v["LogsCovered"] == len(levels[k - 1].recs) for k, v in got.items())
    assert ("Where report: %s holds in %d of %d states" % (name, sum(per_level.values()), sum(len(lv.recs) for lv in levels))) in r4.stdout
    # a file that does not compile: the analysis model's own refusal, with the file's name and the position
    bad = tmp_path / "bad.txt"
    bad.write_text("A == \\E r \\in replicas : rep_status[r] = Recovering\n")
    r5 = _run_cli(["-config", cfg, "-predicates", str(bad), "-whereReport"])
    assert r5.returncode == 1 and "bad.txt:1:" in r5.stderr and "not a status of" in r5.stderr
