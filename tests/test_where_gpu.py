"""State predicates on the GPU (`-m gpu`): k_where through Model.where_flags, ModelChecker.where_scan / where_states / witness_trace and
run(reach=..), against hand-written Python functions over oracle/pycodec.py's unpack of the CPU oracle's records (tests/where_reference.py — the
reference is never the parser).  The spaces are the small ones of test_terminal_states.py; every figure is recomputed from the oracle here."""
import collections
import os
import subprocess

import numpy as np
import pytest

import where_reference as wr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
# (R, C, values, limit, levels walked (None = exhausted))
SPACES = {"2122": (2, 1, 2, 2, None), "3121": (3, 1, 2, 1, 12), "3111": (3, 1, 1, 1, 14)}
SIZES = dict(table_log2=20, frontier_words=1 << 22, frontier_states=1 << 17, pending_entries=1 << 17)
Level = collections.namedtuple("Level", "level words off recs states fps")


@pytest.fixture(scope="module")
def vt():
    import vsr_tlaplus_amd as vt
    assert vt.load().vsrmc_device_count() >= 1, "no HIP device visible"
    return vt


@pytest.fixture(scope="module")
def orc():
    from oracle import orc
    return orc


@pytest.fixture(scope="module")
def spaces(orc):
    """key -> (oracle params, [Level]): every level of the oracle's BFS once — records, their Python view, their fingerprints; shared, never changed"""
    from oracle import pycodec, pyoracle as po
    cache = {}

    def get(key):
        if key not in cache:
            R, C, n, L, depth = SPACES[key]
            P = orc.Params(R, C, n, L)
            PM = po.Model(R, C, tuple("v%d" % (i + 1) for i in range(n)), L)
            b = orc.Bfs(P)
            out = []
            level = 1
            init = orc.init_record(P)
            words, off = init, np.array([0, len(init)], dtype=np.uint64)
            while True:
                recs = [words[int(off[i]): int(off[i + 1])] for i in range(len(off) - 1)]
                out.append(Level(level, words, off, recs, [pycodec.unpack(PM, [int(x) for x in r]) for r in recs], [orc.fingerprint(P, r)[0] for r in recs]))
                if (depth is not None and level >= depth) or b.step() == 0:
                    break
                level += 1
                words, off = b.frontier()
            b.close()
            cache[key] = (P, out)
        return cache[key]
    return get


def _model(vt, key):
    R, C, n, L, _depth = SPACES[key]
    return vt.Model.from_constants(R=R, C_=C, n=n, L=L)


def _same_but_time(a, b):
    return {k: v for k, v in a.items() if k != "kernel_ms"} == {k: v for k, v in b.items() if k != "kernel_ms"}


# ---------------------------------------------------------------------------------------------------------------------
# 1. state by state
# ---------------------------------------------------------------------------------------------------------------------
def test_where_flags_state_by_state(vt, spaces):
    seen = {}                                                   # (set, k) -> set of verdicts
    hits = collections.Counter()
    first = {}
    for key in sorted(SPACES):
        m = _model(vt, key)
        L = SPACES[key][3]
        for tag, preds in (("A", wr.SET_A), ("B", wr.set_b(L))):
            w = m.compile_where(wr.text_of(preds))
            assert w.names == [p[0] for p in preds]
            for lv in spaces(key)[1]:
                flags = m.where_flags(w, lv.words, lv.off)
                assert len(flags) == len(lv.recs)
                for i, s in enumerate(lv.states):
                    want = wr.bits_of(preds, s)
                    assert int(flags[i]) == want, (key, tag, lv.level, i, bin(int(flags[i])), bin(want))
                    for k in range(len(preds)):
                        v = (want >> k) & 1
                        seen.setdefault((tag, k), set()).add(v)
                        if v:
                            hits[(key, preds[k][0])] += 1
                            first.setdefault((key, preds[k][0]), lv.level)
    for (key, name), n in sorted(hits.items()):
        print("where_flags %s %s: %d hits, first at level %d" % (key, name, n, first[(key, name)]))
    # every predicate of set A (eight, all bits of one compiled object) saw both verdicts somewhere: a vacuous predicate fails here
    for k in range(len(wr.SET_A)):
        assert seen[("A", k)] == {0, 1}, wr.SET_A[k][0]
    assert sum(1 for k in range(8) if seen[("B", k)] == {0, 1}) >= 7


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the built-in invariants
# ---------------------------------------------------------------------------------------------------------------------
def test_restated_acknowledged_write_invariants_equal_the_built_in_ones(vt, orc, golden_trace):
    from oracle import pycodec, pyoracle as po
    p = golden_trace["params"]
    P = orc.Params(p["R"], p["C"], len(p["values"]), p["L"], invariant_mask=3)
    PM = po.Model(p["R"], p["C"], tuple(p["values"]), p["L"])
    m = vt.Model.from_constants(R=p["R"], C_=p["C"], n=len(p["values"]), L=p["L"])
    recs = [np.array([int(x, 16) for x in st["words"]], dtype=np.uint64) for st in golden_trace["states"]]
    for r in list(recs):
        recs.extend(s["words"] for s in orc.successors(P, r))
    words = np.concatenate(recs)
    off = np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64)
    w = m.compile_where(wr.ACK_TEXT)
    assert w.names == ["HasNotLost", "OnMajority", "CommittedDivergence"]
    flags = m.where_flags(w, words, off)
    split = collections.Counter()
    for i, rec in enumerate(recs):
        bad = orc.invariants(P, rec)                            # bit 0 AcknowledgedWriteNotLost violated, bit 1 AcknowledgedWritesExistOnMajority violated
        assert (~int(flags[i])) & 3 == bad, (i, int(flags[i]), bad)
        s = pycodec.unpack(PM, [int(x) for x in rec])
        assert wr.bits_of([(None, None, f) for f in wr.ACK_FUNCS], s) == int(flags[i]), i
        split[bad] += 1
    print("acknowledged-write predicates on %d records: violation masks %s" % (len(recs), dict(split)))
    assert len(recs) > len(golden_trace["states"]) and split[0] and split[2] and split[3]      # both verdicts of both


# ---------------------------------------------------------------------------------------------------------------------
# 3. random differential
# ---------------------------------------------------------------------------------------------------------------------
def test_random_expressions(vt, spaces):
    n_true = collections.Counter()
    for key, keep in (("2122", lambda lv: True), ("3121", lambda lv: 10 <= lv.level <= 12)):
        m = _model(vt, key)
        levels = [lv for lv in spaces(key)[1] if keep(lv)]
        words = np.concatenate([lv.words for lv in levels])
        off = [0]
        for lv in levels:
            base = off[-1]
            off.extend(base + int(x) for x in lv.off[1:])
        off = np.array(off, dtype=np.uint64)
        states = [s for lv in levels for s in lv.states]
        preds = wr.random_predicates(20261017, SPACES[key][0], 100)
        for j in range(0, 100, 8):
            chunk = preds[j: j + 8]
            w = m.compile_where("\n".join("P%d == %s" % (k, t) for k, (t, _) in enumerate(chunk)))
            flags = m.where_flags(w, words, off)
            for i, s in enumerate(states):
                got = int(flags[i])
                for k, (text, f) in enumerate(chunk):
                    want = f(s)
                    n_true[(key, j + k)] += want
                    assert bool((got >> k) & 1) == want, "space %s, state %d: %s is %s in the reference" % (key, i, text, want)
    used = sum(1 for k in range(100) if 0 < n_true[("2122", k)] < 2073)
    print("random expressions: %d of 100 have both verdicts on (2,1,2,2)" % used)
    assert used >= 30                                          # (most random expressions are constant on a small space; not all may be)


# ---------------------------------------------------------------------------------------------------------------------
# 4. inside a search
# ---------------------------------------------------------------------------------------------------------------------
def _scan_search(vt, orc, spaces, key, sizes=SIZES, count_holes=False, **kw):
    P, levels = spaces(key)
    m = _model(vt, key)
    w = m.compile_where(wr.text_of(wr.SET_A))
    mc = vt.ModelChecker(m, **dict(sizes, **kw))
    ob = orc.Bfs(P)
    holes = 0
    for lv in levels:
        want = sorted((fp, wr.bits_of(wr.SET_A, s)) for fp, s in zip(lv.fps, lv.states))
        t = mc.where_scan(w)
        assert _same_but_time(t, mc.where_scan(w))                  # any number of times, nothing changes
        assert (t["level"], t["n_states"]) == (lv.level, len(lv.recs))
        if count_holes:                                             # the level's index range is longer than its states: withdrawn indices lie between them
            holes += max(mc.find_fp(fp) for fp in lv.fps) + 1 - t["n_states"]
        fps, bits = mc.where_states()
        assert [(int(a), int(b)) for a, b in zip(fps, bits)] == [x for x in want if x[1]], lv.level
        for k in range(len(wr.SET_A)):
            mine = [fp for fp, b in want if (b >> k) & 1]
            assert t["count"][k] == len(mine), (lv.level, k)
            if mine:
                assert t["min_fp"][k] == mine[0] and mc.find_fp(mine[0]) == t["min_index"][k]
            else:
                assert t["min_fp"][k] is None and t["min_index"][k] is None
        assert np.array_equal(mc.level_fps(), ob.level_fps(lv.level))   # the scan left the level as it was
        d = mc.step()
        nn = ob.step()
        assert d["n_new"] == nn and d["generated"] == ob.info["generated"] and d["deadlocks"] == ob.info["deadlocks"], lv.level
    last = (d, mc.where_scan(w), mc.where_states())
    mc.close()
    ob.close()
    return holes, last


@pytest.mark.parametrize("key", ["2122", "3121"])
def test_where_scan_inside_a_search(vt, orc, spaces, key):
    holes, (d, t, (fps, bits)) = _scan_search(vt, orc, spaces, key)
    if key == "2122":                                               # exhausted: the last level is empty, and scanning it says so
        assert d["n_new"] == 0 and t["n_states"] == 0 and t["count"] == [0] * 8 and t["min_fp"] == [None] * 8 and len(fps) == 0


def test_where_scan_exact_ties_and_host_frontier(vt, orc, spaces):
    _scan_search(vt, orc, spaces, "2122", exact_ties=True)
    _scan_search(vt, orc, spaces, "3121", host_frontier=True)


def test_where_scan_of_a_frontier_with_holes(vt, orc, spaces, monkeypatch):
    """the work-list-overflow configuration of test_gpu_parity.py (tiles taken again in pieces).  Every wave of k_expand draws its successors' indices in
    chunks and publishes the unused tail of its last chunk as withdrawn indices (refs[i] == 0): the scan must step over them"""
    monkeypatch.setenv("VSRMC_CCAP", "256")
    holes, _ = _scan_search(vt, orc, spaces, "3121", sizes=dict(table_log2=20, frontier_words=1 << 24, frontier_states=1 << 20, pending_entries=1 << 19),
                            count_holes=True)
    print("withdrawn indices scanned over: %d" % holes)
    assert holes > 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. the witness
# ---------------------------------------------------------------------------------------------------------------------
def test_reach_stops_at_the_first_level_and_the_witness_is_a_shortest_behaviour(vt, orc, spaces):
    P, levels = spaces("3121")
    first = next(lv for lv in levels if any(wr.log_divergence(s) for s in lv.states))
    want_fp = min(fp for fp, s in zip(first.fps, first.states) if wr.log_divergence(s))
    from oracle import pycodec, pyoracle as po
    PM = po.Model(3, 1, ("v1", "v2"), 1)
    m = _model(vt, "3121")
    w = m.compile_where("LogDivergence == " + wr.LOG_DIVERGENCE)
    norm = lambda r: tuple(int(x) for x in orc.normalise(P, r))   # noqa: E731
    traces = []
    for kw in (dict(), dict(exact_ties=True), dict(table_log2=17, frontier_words=32 << 14, frontier_states=1 << 14, pending_entries=1 << 14)):
        mc = vt.ModelChecker(m, **dict(SIZES, **kw))
        assert mc.run(reach=w) == "reached"
        assert mc.level == first.level and mc.witness["level"] == first.level and mc.witness["name"] == "LogDivergence" and mc.witness["fp"] == want_fp
        tr = mc.witness_trace()
        assert [norm(r) for _, r in mc.witness_trace("LogDivergence")] == [norm(r) for _, r in tr]
        mc.close()
        assert len(tr) == first.level and tr[0][0] == "Initial predicate" and norm(tr[0][1]) == norm(orc.init_record(P))
        chk = m.check_trace([r for _, r in tr])
        assert chk["ok"] and chk["actions"][1:] == [a for a, _ in tr[1:]]
        assert wr.log_divergence(pycodec.unpack(PM, [int(x) for x in tr[-1][1]])) and orc.fingerprint(P, tr[-1][1])[0] == want_fp
        traces.append([(a, norm(r)) for a, r in tr])
    assert traces[0] == traces[1] == traces[2]
    print("log divergence on (3,1,2,1): first at level %d, witness fingerprint %016x" % (first.level, want_fp))
    # never= reports the same state as a violation; the defaults scan nothing
    mc = vt.ModelChecker(m, **SIZES)
    assert mc.run(never=w) == "violation" and mc.witness["kind"] == "violation" and mc.witness["fp"] == want_fp
    mc.close()
    mc = vt.ModelChecker(m, **SIZES)
    assert mc.run(max_depth=first.level + 1) == "max-depth" and mc.witness is None
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. edges
# ---------------------------------------------------------------------------------------------------------------------
def test_where_list_overflow_keeps_counters_and_minima_exact(vt, monkeypatch):
    m = _model(vt, "2122")
    w = m.compile_where(wr.text_of(wr.SET_A))
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


def test_where_scan_is_refused_where_the_terminal_scan_is(vt):
    import ctypes as C
    from vsr_tlaplus_amd import capi
    m = _model(vt, "2122")
    w = m.compile_where("TRUE")
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
    mc.deepen()
    with pytest.raises(vt.VsrmcError) as e:
        mc.where_scan(w)
    assert e.value.code == -6 and "seen-set only" in e.value.message
    mc.close()
    other = _model(vt, "3121")                                      # a program is compiled for one model's constants
    mc = vt.ModelChecker(other, **SIZES)
    with pytest.raises(vt.VsrmcError) as e:
        mc.where_scan(w)
    assert e.value.code == -1
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the CLI
# ---------------------------------------------------------------------------------------------------------------------
def _run_cli(args):
    return subprocess.run([CLI] + args + ["-noTLA", "-tableLog2", "18", "-frontierGiB", "0.05"], capture_output=True, text=True, timeout=300)


def test_cli_reach_invariant_and_where_report(vt, spaces, tmp_path):
    import json
    from test_host_cpu import _cfg
    _P, levels = spaces("3121")
    per_level = {lv.level: sum(1 for s in lv.states if wr.log_divergence(s)) for lv in levels}
    first = min(k for k, v in per_level.items() if v)
    cfg = _cfg(tmp_path, R=3, vals="v1, v2", L=1)
    preds = tmp_path / "predicates.txt"
    preds.write_text("\\* two predicates and a helper\nLOCAL Three == 3\nLogDivergence == " + wr.LOG_DIVERGENCE + "\nLogsAgree == ~LogDivergence /\\ ReplicaCount = Three\n")
    out = str(tmp_path / "witness.tla")
    r = _run_cli(["-config", cfg, "-predicates", str(preds), "-reach", "LogDivergence", "-maxDepth", "12", "-dumpTrace", "tla", out])
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("State satisfying LogDivergence found at depth %d (%d of" % (first, per_level[first])) in r.stdout and "Error" not in r.stdout
    blocks = [ln for ln in r.stdout.splitlines() if ln.startswith("State ") and ": <" in ln]
    assert len(blocks) == first and blocks[0] == "State 1: <Initial predicate>"
    v = _run_cli(["-config", cfg, "-validateTrace", out])
    assert v.returncode == 0 and ("%d states read" % first) in v.stdout and "The trace is a behaviour of the model." in v.stdout, v.stdout + v.stderr
    # the negation as an invariant: reported and exit-coded like a built-in one, the same behaviour
    r2 = _run_cli(["-config", cfg, "-predicates", str(preds), "-invariant", "LogsAgree", "-maxDepth", "12"])
    assert r2.returncode == 12 and "Error: Invariant LogsAgree is violated." in r2.stdout and "Error: The behavior up to this point is:" in r2.stdout
    assert [ln for ln in r2.stdout.splitlines() if ln.startswith("State ") and ": <" in ln] == blocks
    # not reachable within the depth: exit 14
    r3 = _run_cli(["-config", cfg, "-predicates", str(preds), "-reach", "LogDivergence", "-maxDepth", str(first - 1)])
    assert r3.returncode == 14 and "No state satisfying LogDivergence was found" in r3.stdout, r3.stdout + r3.stderr
    # the report: per-level counts, no stop
    r4 = _run_cli(["-config", cfg, "-predicates", str(preds), "-whereReport", "-json", "-maxDepth", "12"])
    assert r4.returncode == 0, r4.stdout + r4.stderr
    rows = [json.loads(ln) for ln in r4.stdout.splitlines() if ln.startswith("{")]
    got = {}
    for row in rows:                                                # line k is the step that expands level k - 1; the last level has a line of its own
        assert set(row["where"]) == {"LogDivergence", "LogsAgree"}
        got[row["level"] if row.get("expanded") is False else row["level"] - 1] = row["where"]
    assert {k: v["LogDivergence"] for k, v in got.items()} == per_level
    assert all(v["LogDivergence"] + v["LogsAgree"] == len(levels[k - 1].recs) for k, v in got.items())
    assert ("Where report: LogDivergence holds in %d of %d states" % (sum(per_level.values()), sum(len(lv.recs) for lv in levels))) in r4.stdout
    # a name the file does not export, a file that does not compile
    assert _run_cli(["-config", cfg, "-predicates", str(preds), "-reach", "Three"]).returncode == 2
    bad = tmp_path / "bad.txt"
    bad.write_text("A == rep_status[1] = 1\n")
    r5 = _run_cli(["-config", cfg, "-predicates", str(bad), "-whereReport"])
    assert r5.returncode == 1 and "bad.txt:1:" in r5.stderr and "type mismatch" in r5.stderr
