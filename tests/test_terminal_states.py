"""Terminal states (`-m gpu`): k_terminal — the guards-only scan that finds the states without any enabled (action, binding) instance
(TLC's deadlock check) and marks the ones in which AllReplicasMoveToSameView (VSR.tla:958-962) is false — through vsrmc_terminal_batch,
vsrmc_checker_terminal_scan / _terminal_states, ModelChecker.deadlock_trace and the CLI, against the CPU oracles.

Bit 0 is compared with `orc.successors(P, rec) == []`, bit 1 with the predicate computed here from oracle/pycodec.py's unpack.  The totals
per configuration are pinned from the CPU oracle (Kahn's algorithm over its successor edges also showed these spaces acyclic)."""
import collections
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")

# (R, C, values, limit, assume_commit_number, levels walked (None = exhausted), (neither, unsettled only, terminal only, both), first level with a terminal state)
CONFIGS = {
    "2122": (2, 1, 2, 2, False, None, (501, 1444, 128, 0), 18),
    "2221a": (2, 2, 2, 1, True, None, (318, 575, 80, 0), 14),
    "3111": (3, 1, 1, 1, False, 14, (1321, 14387, 39, 0), 11),
    "3121": (3, 1, 2, 1, False, 12, (239, 9995, 0, 0), None),
}
SIZES = dict(table_log2=20, frontier_words=1 << 22, frontier_states=1 << 17, pending_entries=1 << 17)


@pytest.fixture(scope="module")
def vt():
    import vsr_tlaplus_amd as vt
    assert vt.load().vsrmc_device_count() >= 1, "no HIP device visible"
    return vt


@pytest.fixture(scope="module")
def orc():
    from oracle import orc
    return orc


def _setup(vt, orc, key):
    R, C, n, L, assume, depth, totals, first = CONFIGS[key]
    P = orc.Params(R, C, n, L, assume_commit_number=assume)
    m = vt.Model.from_constants(R=R, C_=C, n=n, L=L, assume_commit_number=assume)
    return P, m, depth, totals, first


def _levels(orc, P, depth):
    """(level, words, off) of every level of the oracle's BFS, level 1 from orc.init_record; `depth` levels or to exhaustion"""
    b = orc.Bfs(P)
    level = 1
    init = orc.init_record(P)
    yield 1, init, np.array([0, len(init)], dtype=np.uint64)
    while depth is None or level < depth:
        if b.step() == 0:
            break
        level += 1
        words, off = b.frontier()
        yield level, words, off
    b.close()


def _unsettled(pycodec, PM, rec):
    s = pycodec.unpack(PM, [int(x) for x in rec])
    return not (all(st == "Normal" for st in s["rep_status"]) and len(set(s["rep_view_number"])) == 1)


def _same_but_time(a, b):
    return {k: v for k, v in a.items() if k != "kernel_ms"} == {k: v for k, v in b.items() if k != "kernel_ms"}


# ---------------------------------------------------------------------------------------------------------------------
# 1. state by state, both bits, both values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(CONFIGS))
def test_terminal_flags_state_by_state(vt, orc, key):
    from oracle import pycodec, pyoracle as po
    P, m, depth, totals, first = _setup(vt, orc, key)
    R, C, n, L, assume = CONFIGS[key][:5]
    PM = po.Model(R, C, tuple("v%d" % (i + 1) for i in range(n)), L, assume_commit_number=assume)
    count = collections.Counter()
    first_seen = None
    for level, words, off in _levels(orc, P, depth):
        flags = m.terminal_flags(words, off)
        assert len(flags) == len(off) - 1
        for i in range(len(off) - 1):
            rec = words[int(off[i]): int(off[i + 1])]
            term = orc.successors(P, rec) == []
            uns = _unsettled(pycodec, PM, rec)
            assert int(flags[i]) == (1 if term else 0) | (2 if uns else 0), (level, i, int(flags[i]), term, uns)
            count[(term, uns)] += 1
            if term and first_seen is None:
                first_seen = level
    got = (count[(False, False)], count[(False, True)], count[(True, False)], count[(True, True)])
    print("terminal_flags %s: neither %d, unsettled only %d, terminal only %d, both %d; first terminal level %s" % ((key,) + got + (first_seen,)))
    assert got == totals
    assert first_seen == first


# ---------------------------------------------------------------------------------------------------------------------
# 2. the scan inside a search
# ---------------------------------------------------------------------------------------------------------------------
def _scan_search(vt, orc, key, sizes=SIZES, exact_ties=False, host_frontier=False):
    P, m, depth, totals, first = _setup(vt, orc, key)
    mc = vt.ModelChecker(m, exact_ties=exact_ties, host_frontier=host_frontier, **sizes)
    ob = orc.Bfs(P)
    level, first_hit, n_term_total = 1, None, 0
    while True:
        if level == 1:
            init = orc.init_record(P)
            words, off = init, np.array([0, len(init)], dtype=np.uint64)
        else:
            words, off = ob.frontier()
        recs = [words[int(off[i]): int(off[i + 1])] for i in range(len(off) - 1)]
        want = sorted(orc.fingerprint(P, r)[0] for r in recs if orc.successors(P, r) == [])
        t = mc.terminal_scan()
        assert _same_but_time(t, mc.terminal_scan())                # any number of times, nothing changes
        assert (t["level"], t["n_states"]) == (level, len(recs))
        fps, flags = mc.terminal_states()
        assert [int(x) for x in fps] == want, level
        assert t["n_terminal"] == len(want) and all(int(f) & 1 for f in flags)
        assert t["n_unsettled"] == sum(1 for f in flags if int(f) & 2)
        if want:
            assert t["min_fp"] == want[0] == int(fps[0]) and mc.find_fp(t["min_fp"]) == t["min_index"]
            first_hit = first_hit or level
        else:
            assert t["min_fp"] is None and t["min_index"] is None
        assert np.array_equal(mc.level_fps(), ob.level_fps(level))  # the scan left the level as it was
        d = mc.step()
        nn = ob.step()
        assert d["deadlocks"] == t["n_terminal"] == ob.info["deadlocks"], (level, d["deadlocks"], t["n_terminal"], ob.info["deadlocks"])
        assert d["n_new"] == nn
        n_term_total += t["n_terminal"]
        level += 1
        if nn == 0 or (depth is not None and level > depth):
            break
    mc.close()
    ob.close()
    assert first_hit == first
    assert n_term_total == totals[2] + totals[3]
    return first_hit


@pytest.mark.parametrize("key", sorted(CONFIGS))
def test_terminal_scan_equals_the_next_steps_deadlocks(vt, orc, key):
    _scan_search(vt, orc, key)


def test_terminal_scan_exact_ties_and_host_frontier(vt, orc):
    """the order inside a level differs (two-kernel levels; records in pinned host memory), the result must not"""
    assert _scan_search(vt, orc, "2122", exact_ties=True) == 18
    assert _scan_search(vt, orc, "2221a", host_frontier=True) == 14


def test_terminal_scan_in_the_smallest_record_buffers_that_store_every_level(vt, orc):
    """(3,1,1,1) through level 14 with record buffers of 2^k states (32 words per state), k rising from 11 (the checker takes no fewer: one index chunk): the runs whose buffers are too
    small end in "frontier full" (ERR 21), the first one that stores every level — the smallest such power of two — gives the results of
    every other run (_scan_search asserts them level by level)"""
    too_small = 0
    for k in range(11, 18):
        try:
            hit = _scan_search(vt, orc, "3111", sizes=dict(table_log2=17, frontier_words=32 << k, frontier_states=1 << k, pending_entries=1 << 14))
        except vt.VsrmcError as e:
            assert e.code == -5 and "error 21" in e.message, e.message
            too_small += 1
            continue
        assert hit == 11
        break
    else:
        raise AssertionError("no buffer size stored every level")
    print("smallest record buffers that store every level of (3,1,1,1) through 14: 2^%d states" % k)
    assert too_small >= 1


def test_terminal_list_overflow_keeps_counters_and_minima_exact(vt, orc, monkeypatch):
    P, m, _depth, _totals, _first = _setup(vt, orc, "2122")
    mc = vt.ModelChecker(m, **SIZES)
    while mc.level < 18:
        mc.step()
    full = mc.terminal_scan()
    fps, _ = mc.terminal_states()
    assert full["n_terminal"] == len(fps) > 1
    monkeypatch.setenv("VSRMC_TERMINAL_LIST_CAP", "1")
    assert _same_but_time(mc.terminal_scan(), full)
    with pytest.raises(vt.VsrmcError) as e:
        mc.terminal_states()
    assert e.value.code == -5 and ("has %d" % len(fps)) in e.value.message
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the trace
# ---------------------------------------------------------------------------------------------------------------------
def test_deadlock_trace_is_a_behaviour_into_the_smallest_terminal_state(vt, orc):
    P, m, _depth, _totals, _first = _setup(vt, orc, "2122")
    norm = lambda w: tuple(int(x) for x in orc.normalise(P, w))   # noqa: E731
    ob = orc.Bfs(P)                                                # the smallest fingerprint among the 18th level's terminal states, by the oracle
    for _ in range(17):
        ob.step()
    words, off = ob.frontier()
    recs = [words[int(off[i]): int(off[i + 1])] for i in range(len(off) - 1)]
    want_fp = min(orc.fingerprint(P, r)[0] for r in recs if orc.successors(P, r) == [])
    ob.close()
    traces = []
    for exact in (False, True):
        mc = vt.ModelChecker(m, exact_ties=exact, **SIZES)
        assert mc.run(check_deadlock=True) == "deadlock"
        assert mc.level == 18 and mc.deadlock["level"] == 18 and mc.deadlock["n_terminal"] > 0
        assert mc.deadlock["min_fp"] == want_fp
        tr = mc.deadlock_trace()
        mc.close()
        traces.append([(a, norm(w)) for a, w in tr])
        assert len(tr) == 18 and tr[0][0] == "Initial predicate" and norm(tr[0][1]) == norm(orc.init_record(P))
        for t in range(len(tr) - 1):
            hits = [s for s in orc.successors(P, tr[t][1]) if norm(s["words"]) == norm(tr[t + 1][1])]
            assert hits and orc.ACTIONS[hits[0]["action"]] == tr[t + 1][0], t
        assert [orc.invariants(P, rec) for _, rec in tr] == [0] * 18
        assert orc.successors(P, tr[-1][1]) == []
        assert orc.fingerprint(P, tr[-1][1])[0] == want_fp
    assert traces[0] == traces[1]
    mc = vt.ModelChecker(m, **SIZES)                               # the default stays off: the search runs through its terminal states
    assert mc.run() == "exhausted" and mc.deadlock is None
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the CLI
# ---------------------------------------------------------------------------------------------------------------------
def _run_cli(args):
    return subprocess.run([CLI] + args + ["-noTLA", "-tableLog2", "16", "-frontierGiB", "0.01"], capture_output=True, text=True, timeout=300)


def test_cli_check_deadlock_prints_and_dumps_the_behaviour(vt, tmp_path):
    from test_host_cpu import _cfg
    cfg = _cfg(tmp_path, R=2, vals="v1, v2", L=2)
    out = str(tmp_path / "deadlock_trace.tla")
    r = _run_cli(["-config", cfg, "-checkDeadlock", "-dumpTrace", "tla", out])
    assert r.returncode == 11, r.stdout + r.stderr
    assert "Error: Deadlock reached (" in r.stdout and "of level 18 have no successor)." in r.stdout
    assert "Error: The behavior up to this point is:" in r.stdout
    blocks = [ln for ln in r.stdout.splitlines() if ln.startswith("State ") and ": <" in ln]
    assert len(blocks) == 18 and blocks[0] == "State 1: <Initial predicate>"
    v = _run_cli(["-config", cfg, "-validateTrace", out])
    assert v.returncode == 0 and "18 states read" in v.stdout and "The trace is a behaviour of the model." in v.stdout, v.stdout + v.stderr
    # CHECK_DEADLOCK TRUE in the cfg, no switch: the same
    (tmp_path / "b").mkdir()
    cfg2 = _cfg(tmp_path / "b", R=2, vals="v1, v2", L=2, symmetry="SYMMETRY symmValues\nCHECK_DEADLOCK TRUE")
    r2 = _run_cli(["-config", cfg2])
    strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith(("Finished in", "Progress(", "The counter-example was written"))]   # noqa: E731
    assert r2.returncode == 11 and strip(r2.stdout) == strip(r.stdout)
    # without the switch nothing is scanned: the run goes through its terminal states
    r3 = _run_cli(["-config", cfg])
    assert r3.returncode == 0 and "Deadlock" not in r3.stdout and "2073 distinct states found" in r3.stdout
    # -json: terminal / unsettled per level — of the level the line's step expanded, like its deadlocks
    import json
    r4 = _run_cli(["-config", cfg, "-terminalReport", "-json"])
    assert r4.returncode == 0, r4.stdout + r4.stderr
    rows = [json.loads(ln) for ln in r4.stdout.splitlines() if ln.startswith("{")]
    assert len(rows) == 27 and all(row["terminal"] == row["deadlocks"] and row["unsettled"] == 0 for row in rows)
    # line k is the step that expands level k: levels 1-17 have no terminal state, level 18 has the first ones, 128 in all
    assert [row["terminal"] for row in rows[:17]] == [0] * 17 and rows[17]["level"] == 19 and rows[17]["terminal"] > 0
    assert sum(row["terminal"] for row in rows) == 128
    r5 = _run_cli(["-config", cfg, "-json"])                     # without a scan the lines are today's
    assert r5.returncode == 0 and '"terminal"' not in r5.stdout


def test_cli_terminal_report(vt, tmp_path):
    from test_host_cpu import _cfg
    cfg = _cfg(tmp_path, R=2, vals="v1, v2", L=2)
    r = _run_cli(["-config", cfg, "-terminalReport"])
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Terminal report:")]
    assert len(line) == 1 and "128 terminal states" in line[0] and "level 18:" in line[0] and ", 0 unsettled" in line[0], r.stdout
    assert "no verdict on ViewChangeCompletes" in r.stdout and "Stuttering" not in r.stdout
    assert "Model checking completed. No error has been found." in r.stdout and "2073 distinct states found" in r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# 5. the analysis models
# ---------------------------------------------------------------------------------------------------------------------
# The prefixes test_model2_successors_state_by_state and its model-3 twin walk are the whole space of (2 replicas, 2 values, limit 2):
# 14 735 states in 27 levels.  From the CPU oracles (orc2 / orc3: successors == []; the predicate from pyoracle2 / pyoracle3's unpack):
# 3 642 neither, 10 085 unsettled only, 1 008 terminal only, 0 both; the first terminal state at level 15.
ANALYSIS_TOTALS = {2: ((3642, 10085, 1008, 0), 15), 3: ((3642, 10085, 1008, 0), 15)}


@pytest.mark.parametrize("which", [2, 3])
def test_terminal_flags_and_scan_on_the_analysis_models(vt, which):
    if which == 2:
        from oracle import orc2 as o, pyoracle2 as po
        m = vt.Model.second_model(R=2, n=2, L=2)
        PM = po.Model(2, ("v1", "v2"), 2)
    else:
        from oracle import orc3 as o, pyoracle3 as po
        m = vt.Model.third_model(R=2, n=2, L=2)
        PM = po.Model(2, ("a", "b"), 2)
    P = o.Params(2, 2, 2)
    mc = vt.ModelChecker(m, **SIZES)
    b = o.Bfs(P)
    level, first = 1, None
    count = collections.Counter()
    while True:
        if level == 1:
            init = o.init_record(P)
            words, off = init, np.array([0, len(init)], dtype=np.uint64)
        else:
            words, off = b.frontier()
        flags = m.terminal_flags(words, off)
        n_term = 0
        for i in range(len(off) - 1):
            rec = words[int(off[i]): int(off[i + 1])]
            term = o.successors(P, rec) == []
            st = po.unpack(PM, [int(x) for x in rec])
            uns = not (all(x == po.Normal for x in st["rep_status"]) and len(set(st["rep_view_number"])) == 1)
            assert int(flags[i]) == (1 if term else 0) | (2 if uns else 0), (level, i, int(flags[i]), term, uns)
            count[(term, uns)] += 1
            n_term += term
        t = mc.terminal_scan()
        d = mc.step()
        nn = b.step()
        assert t["n_terminal"] == n_term == d["deadlocks"] == b.info["deadlocks"], level
        assert t["n_states"] == len(off) - 1 and d["n_new"] == nn and t["n_unsettled"] == 0
        if n_term and first is None:
            first = level
        level += 1
        if nn == 0:
            break
    mc.close()
    b.close()
    assert ((count[(False, False)], count[(False, True)], count[(True, False)], count[(True, True)]), first) == ANALYSIS_TOTALS[which]


# ---------------------------------------------------------------------------------------------------------------------
# 6. where there are no records to scan
# ---------------------------------------------------------------------------------------------------------------------
def test_terminal_scan_is_refused_on_sharded_checkers_and_seen_set_only_levels(vt):
    import ctypes as C
    from vsr_tlaplus_amd import capi
    m = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
    o = capi.Options()
    capi.load().vsrmc_options_default(C.byref(o))
    o.table_log2, o.frontier_words, o.frontier_states, o.pending_entries, o.rank, o.world = 16, 1 << 18, 1 << 13, 1 << 14, 0, 2
    h = C.c_void_p()
    capi.check(capi.load().vsrmc_checker_create(m._h, C.byref(o), C.byref(h)))
    info = capi.TerminalInfo()
    assert capi.load().vsrmc_checker_terminal_scan(h, C.byref(info)) == -6
    assert b"sharded" in capi.load().vsrmc_last_error()
    capi.load().vsrmc_checker_destroy(h)
    mc = vt.ModelChecker(m, **SIZES)
    for _ in range(5):
        mc.step()
    assert mc.terminal_scan()["level"] == 6
    mc.deepen()
    with pytest.raises(vt.VsrmcError) as e:
        mc.terminal_scan()
    assert e.value.code == -6 and "seen-set only" in e.value.message
    mc.close()
