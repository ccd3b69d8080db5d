"""The deadlock check on the levels beyond the record buffers (`-m gpu`): ModelChecker.deep_terminal_attach / deep_terminal_results / deep_terminal_states /
deep_terminal_trace, run(check_deadlock=True, deep=True) and the CLI's -deepTerminal — csrc/host_deep_terminal.hpp, k_probe_children
(csrc/vsr_deep_terminal.hpp), k_terminal unchanged.

Expected values come from three routes, never from the code under test: the CPU oracle (`orc.successors(P, rec) == []`, the unsettled predicate of
test_terminal_states.py), the stored scans (terminal_scan / terminal_states) of a second checker whose buffers hold the space, and the `deadlocks` figure of
the step that expands a level.  Every comparison is exact."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_deep_terminal_cpu import STATES_3111, STATES_3121, TERMINAL_3111, TERMINAL_3121

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
BIG = dict(table_log2=20, frontier_words=1 << 22, frontier_states=1 << 17, pending_entries=1 << 17)
KEEP = ("level", "frontier", "generated", "n_new", "distinct", "total_generated", "deadlocks", "max_bag", "viol_fp", "viol_mask", "act_generated", "fp_xor", "fp_sum")


@pytest.fixture(scope="module")
def vt():
    import vsr_tlaplus_amd as vt
    assert vt.load().vsrmc_device_count() >= 1, "no HIP device visible"
    return vt


@pytest.fixture(scope="module")
def orc():
    from oracle import orc
    return orc


def _stored_scan(vt, m, upto=None, sizes=BIG):
    """level -> (terminal_scan, fingerprints, flags, deadlocks of the step that expands the level or None) of a checker that stores every level"""
    mc = vt.ModelChecker(m, **sizes)
    out = {}
    while True:
        t = mc.terminal_scan()
        fps, flags = mc.terminal_states()
        lvl = mc.level
        if upto is not None and lvl >= upto:
            out[lvl] = (t, [int(x) for x in fps], [int(x) for x in flags], None)
            break
        d = mc.step()
        out[lvl] = (t, [int(x) for x in fps], [int(x) for x in flags], d["deadlocks"])
        assert d["deadlocks"] == t["n_terminal"]
        if d["n_new"] == 0:
            break
    mc.close()
    return out


@pytest.fixture(scope="module")
def stored(vt):
    """the stored scans of a space, once per module (computed before a test sets a knob: a fixture is set up ahead of the test's body), never changed"""
    cache = {}

    def get(key, make, upto=None):
        if key not in cache:
            assert not any(k in os.environ for k in ("VSRMC_TERMINAL_LIST_CAP", "VSRMC_STEP_SLICE", "VSRMC_DEEP_CHILD_WORDS"))
            cache[key] = _stored_scan(vt, make(), upto)
        return cache[key]
    return get


def _oracle_terminal(orc, P, level):
    """(records of the level, sorted fingerprints of its terminal states) by the CPU oracle"""
    b = orc.Bfs(P)
    for _ in range(level - 1):
        b.step()
    words, off = b.frontier() if level > 1 else (orc.init_record(P), np.array([0, len(orc.init_record(P))], dtype=np.uint64))
    b.close()
    recs = [words[int(off[i]): int(off[i + 1])] for i in range(len(off) - 1)]
    return recs, sorted(int(orc.fingerprint(P, r)[0]) for r in recs if orc.successors(P, r) == [])


def _new_results(mc, seen):
    out = []
    for r in mc.deep_terminal_results():
        key = (r["level"], r["kind"] == "probed")
        if key not in seen:
            seen[key] = r
            out.append(r)
        else:                                                       # reported once: a later pass regenerates the level and leaves its figures alone
            assert r == seen[key], key
    return out


def _check_against_stored(mc, r, st, listed=True):
    t, fps, flags, _dl = st
    probed = r["kind"] == "probed"
    assert (r["n_terminal"], r["n_unsettled"], r["min_fp"], r["min_fp_unsettled"]) == (t["n_terminal"], t["n_unsettled"], t["min_fp"], t["min_fp_unsettled"]), (r, t)
    assert r["exact"] is True
    if not probed:
        assert r["n_states"] == t["n_states"], (r["level"], r["n_states"], t["n_states"])
    else:
        assert r["n_states"] >= r["n_terminal"]                     # copies scanned, not states
    if listed:
        f, fl = mc.deep_terminal_states(r["level"], probed=probed)
        assert [int(x) for x in f] == fps and [int(x) for x in fl] == flags, (r["level"], r["kind"])
        assert r["n_listed"] == len(fps)


def _deepen_to_exhaustion(mc, stored_levels, check, max_level=None):
    """deepen() until the space is exhausted (or max_level is inserted); every result, when first reported, goes through check(r) -> {(level, probed): r}"""
    seen, deadlocks = {}, {}
    while True:
        a, b = mc.deepen()
        if a["n_new"] == 0:
            break
        assert a["viol_mask"] == 0 and (b is None or b["viol_mask"] == 0)
        deadlocks[a["level"] - 1] = a["deadlocks"]                   # of the level this pass expanded
        for r in _new_results(mc, seen):
            check(r)
        if max_level is not None and a["level"] >= max_level:
            break
    for (lvl, probed), r in seen.items():                           # n_terminal of a scanned level == deadlocks of its expanding step, wherever the search reports one
        if not probed and lvl in deadlocks:
            assert r["n_terminal"] == deadlocks[lvl], (lvl, r["n_terminal"], deadlocks[lvl])
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# 1. a whole small space
# ---------------------------------------------------------------------------------------------------------------------
def test_whole_small_space(vt, orc, stored):
    """(2,1,{v1,v2},2): 2 073 states in 27 levels, 128 terminal states, the first at level 18; two steps, then deepen() to exhaustion"""
    from oracle import pycodec, pyoracle as po
    P = orc.Params(2, 1, 2, 2)
    PM = po.Model(2, 1, ("v1", "v2"), 2)
    m = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
    ref = stored("2122", lambda: m)
    top = max(ref)
    assert top == 27 and sum(v[0]["n_states"] for v in ref.values()) == 2073
    oracle = {}
    for lvl in range(4, top + 1):
        recs, want = _oracle_terminal(orc, P, lvl)
        assert ref[lvl][1] == want and ref[lvl][0]["n_states"] == len(recs), lvl
        term = [r for r in recs if orc.successors(P, r) == []]
        for r in term:                                              # none of these terminal states is unsettled
            s = pycodec.unpack(PM, [int(x) for x in r])
            assert all(st == "Normal" for st in s["rep_status"]) and len(set(s["rep_view_number"])) == 1
        oracle[lvl] = want
    mc = vt.ModelChecker(m, table_log2=16, frontier_words=1 << 20, frontier_states=1 << 14, pending_entries=1 << 15)
    for _ in range(2):
        mc.step()
    base = mc.level
    assert base == 3
    mc.deep_terminal_attach()
    mc.deep_terminal_attach()                                       # a second attachment is a no-op
    assert mc.deep_terminal_results() == []

    def check(r):
        if r["level"] > top:                                        # the level after the last one: nothing is new there
            assert r["kind"] == "probed" and r["n_terminal"] == 0 and r["exact"] is True
            return
        _check_against_stored(mc, r, ref[r["level"]])
        assert r["n_unsettled"] == 0 and r["n_terminal"] == len(oracle[r["level"]])
        assert r["min_fp"] == (oracle[r["level"]][0] if oracle[r["level"]] else None)

    seen = _deepen_to_exhaustion(mc, ref, check)
    scanned = sorted(lvl for (lvl, probed) in seen if not probed)
    assert scanned == list(range(base + 1, top + 1)), scanned       # every level beyond the base exactly once, as a regenerated or inserted level
    assert all(seen[(lvl, False)]["kind"] in ("regenerated", "inserted") for lvl in scanned) and seen[(base + 1, False)]["kind"] == "regenerated"
    probed = sorted(lvl for (lvl, p) in seen if p and lvl <= top)
    assert probed == list(range(base + 3, top + 1)), probed
    assert sum(seen[(lvl, False)]["n_terminal"] for lvl in scanned) == 128
    assert min(lvl for lvl in scanned if seen[(lvl, False)]["n_terminal"]) == 18
    # every list is kept, also the ones of the first descents
    f, _ = mc.deep_terminal_states(18)
    assert [int(x) for x in f] == oracle[18]
    # a stored-level scan keeps refusing a seen-set-only level, word for word
    with pytest.raises(vt.VsrmcError) as e:
        mc.terminal_scan()
    assert e.value.code == -6 and "the deepest complete level exists in the seen-set only (vsrmc_checker_deepen): it has no records to scan; its terminal states stay counted" in e.value.message
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. several slices and chunks: the figures of a level accumulate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob", [None, ("VSRMC_STEP_SLICE", "7"), ("VSRMC_DEEP_CHILD_WORDS", "1"), ("VSRMC_TERMINAL_LIST_CAP", "4")],
                         ids=["plain", "small-sub-slices", "small-child-chunks", "list-of-4"])
def test_levels_that_pass_in_several_slices_and_chunks(vt, stored, knob, monkeypatch):
    """(3,1,{v1},1), levels 8-16 beyond a base of 7, with record buffers so small that a pass takes several slices and sub-slices"""
    m = vt.Model.from_constants(R=3, C_=1, n=1, L=1)
    ref = stored("3111", lambda: m, 17)
    assert [ref[lvl][0]["n_states"] for lvl in range(1, 17)] == STATES_3111 and [ref[lvl][0]["n_terminal"] for lvl in range(1, 17)] == TERMINAL_3111
    if knob:
        monkeypatch.setenv(*knob)
    mc = vt.ModelChecker(m, table_log2=20, frontier_words=1 << 17, frontier_states=1 << 13, pending_entries=1 << 16)
    for _ in range(6):
        mc.step()
    assert mc.level == 7
    mc.deep_terminal_attach()
    cap = knob is not None and knob[0] == "VSRMC_TERMINAL_LIST_CAP"

    def check(r):
        lvl, st = r["level"], ref[r["level"]]
        t, fps, _flags, _dl = st
        if r["kind"] != "probed":
            # counters and minima never come from the list: exact under every knob
            assert (r["n_states"], r["n_terminal"], r["n_unsettled"], r["min_fp"], r["n_listed"]) == (t["n_states"], t["n_terminal"], t["n_unsettled"], t["min_fp"], len(fps)), (lvl, r)
            assert r["exact"] is True and r["n_terminal"] == TERMINAL_3111[lvl - 1] and r["n_states"] == STATES_3111[lvl - 1]
            if cap and len(fps) > 4:
                with pytest.raises(vt.VsrmcError) as e:
                    mc.deep_terminal_states(lvl)
                assert e.value.code == -5 and ("has %d," % len(fps)) in e.value.message, e.value.message
            else:
                _check_against_stored(mc, r, st)
        elif r["exact"]:
            _check_against_stored(mc, r, st)
        else:                                                       # an overflowed list of terminal copies: lower bounds, never reported as exact
            assert cap and r["n_listed"] > 4
            assert r["n_terminal"] <= t["n_terminal"] and r["n_unsettled"] <= t["n_unsettled"]
            with pytest.raises(vt.VsrmcError) as e:
                mc.deep_terminal_states(lvl, probed=True)
            assert e.value.code == -5

    seen = _deepen_to_exhaustion(mc, ref, check, max_level=16)
    print("level: kind slices chunks |", ", ".join("%d%s: %s %d %d" % (lvl, "p" if p else "", r["kind"][:3], r["slices"], r["chunks"]) for (lvl, p), r in sorted(seen.items())))
    assert sorted(lvl for (lvl, p) in seen if not p) == list(range(8, 17))
    assert sorted(lvl for (lvl, p) in seen if p) == list(range(10, 18))
    for lvl in (14, 15, 16):
        assert seen[(lvl, False)]["slices"] > 1, (lvl, seen[(lvl, False)])
        assert seen[(lvl, True)]["slices"] > 1 and seen[(lvl, True)]["bytes_written"] > 0
    if knob and knob[0] == "VSRMC_DEEP_CHILD_WORDS":                # the smallest chunk the library takes: 64 records of the largest size
        for lvl in (14, 15, 16, 17):
            assert seen[(lvl, True)]["chunks"] >= 2 * seen[(lvl, True)]["slices"], (lvl, seen[(lvl, True)])
    elif knob is None:
        assert all(seen[(lvl, True)]["chunks"] == seen[(lvl, True)]["slices"] for lvl in range(10, 18))
    if knob and knob[0] == "VSRMC_STEP_SLICE":                      # sub-slices of seven parents: many instance lists per scratch slice
        assert seen[(16, True)]["slices"] > STATES_3111[14] // 14    # (level 15's parents; a list without an instance is not consumed)
    if cap:
        assert any(not r["exact"] for (lvl, p), r in seen.items() if p)
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the same deadlock from three bases
# ---------------------------------------------------------------------------------------------------------------------
def test_the_same_deadlock_as_the_probed_the_inserted_and_the_regenerated_level(vt, orc):
    P = orc.Params(3, 1, 2, 1)
    recs, want = _oracle_terminal(orc, P, 15)
    assert len(recs) == STATES_3121[15] and len(want) == TERMINAL_3121[15] == 4
    norm = lambda w: tuple(int(x) for x in orc.normalise(P, w))    # noqa: E731
    m = vt.Model.from_constants(R=3, C_=1, n=2, L=1)
    traces = []
    for base, kind in ((12, "probed"), (13, "inserted"), (14, "regenerated")):
        for _rerun in range(2):
            mc = vt.ModelChecker(m, table_log2=20, frontier_words=1 << 21, frontier_states=1 << 15, pending_entries=1 << 16)
            for _ in range(base - 1):
                mc.step()
            assert mc.level == base
            a, _b = mc.deepen()                                     # level base + 1 becomes a seen-set-only level; run() attaches and its first advance() descends
            assert a["level"] == base + 1 and mc.depth != mc.level
            assert mc.run(check_deadlock=True, deep=True) == "deadlock"
            assert mc.depth == base + 2
            d = mc.deadlock
            assert (d["level"], d["kind_of_level"], d["exact"], d["n_terminal"], d["min_fp"], d["n_unsettled"]) == (15, kind, True, 4, want[0], 0), d
            f, fl = mc.deep_terminal_states(15, probed=kind == "probed")
            assert [int(x) for x in f] == want and [int(x) for x in fl] == [1] * 4
            tr = mc.deadlock_trace()
            assert [(a_, norm(w)) for a_, w in mc.deep_terminal_trace()] == [(a_, norm(w)) for a_, w in tr]
            mc.close()
            assert len(tr) == 15 and tr[0][0] == "Initial predicate" and norm(tr[0][1]) == norm(orc.init_record(P))
            for t in range(len(tr) - 1):                            # every step is an oracle successor under its action name
                hits = [s for s in orc.successors(P, tr[t][1]) if norm(s["words"]) == norm(tr[t + 1][1])]
                assert hits and orc.ACTIONS[hits[0]["action"]] == tr[t + 1][0], t
            assert [orc.invariants(P, rec) for _, rec in tr] == [0] * 15
            assert orc.successors(P, tr[-1][1]) == [] and int(orc.fingerprint(P, tr[-1][1])[0]) == want[0]
            traces.append([(a_, norm(w)) for a_, w in tr])
    assert all(t == traces[0] for t in traces[1:])                 # one behaviour: in two runs and from all three bases
    # run(check_deadlock=True) without deep behaves as before: beyond the record buffers it does not look
    mc = vt.ModelChecker(m, table_log2=20, frontier_words=1 << 21, frontier_states=1 << 15, pending_entries=1 << 16)
    for _ in range(12):
        mc.step()
    mc.deepen()
    assert mc.run(check_deadlock=True, max_depth=16) == "max-depth" and mc.deadlock is None
    with pytest.raises(vt.VsrmcError) as e:
        mc.deep_terminal_results()
    assert e.value.code == -6
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the analysis models, and two clients
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["second", "third", "two-clients"])
def test_analysis_models_and_two_clients_whole(vt, stored, which):
    if which == "two-clients":
        make = lambda: vt.Model.from_constants(R=2, C_=2, n=2, L=1, assume_commit_number=True)   # noqa: E731
        states, total, first, base = 973, 80, 14, 5
    else:
        make = lambda: (vt.Model.second_model if which == "second" else vt.Model.third_model)(R=2, n=2, L=2)   # noqa: E731
        states, total, first, base = 14735, 1008, 15, 8
    m = make()
    ref = stored(which, lambda: m)
    top = max(ref)
    assert sum(v[0]["n_states"] for v in ref.values()) == states and sum(v[0]["n_terminal"] for v in ref.values()) == total
    assert min(lvl for lvl, v in ref.items() if v[0]["n_terminal"]) == first and all(v[0]["n_unsettled"] == 0 for v in ref.values())
    mc = vt.ModelChecker(m, table_log2=18, frontier_words=1 << 21, frontier_states=1 << 15, pending_entries=1 << 16)
    for _ in range(base - 1):
        mc.step()
    assert mc.level == base < first
    mc.deep_terminal_attach()

    def check(r):
        if r["level"] > top:
            assert r["kind"] == "probed" and r["n_terminal"] == 0
            return
        _check_against_stored(mc, r, ref[r["level"]])

    seen = _deepen_to_exhaustion(mc, ref, check)
    scanned = sorted(lvl for (lvl, p) in seen if not p)
    assert scanned == list(range(base + 1, top + 1))
    assert sum(seen[(lvl, False)]["n_terminal"] for lvl in scanned) == total
    assert min(lvl for lvl in scanned if seen[(lvl, False)]["n_terminal"]) == first
    assert min(lvl for (lvl, p), r in seen.items() if p and r["n_terminal"]) == first
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. off means off, on changes nothing else
# ---------------------------------------------------------------------------------------------------------------------
def test_off_means_off_and_on_changes_nothing_else(vt):
    import where_reference as wr
    m = vt.Model.from_constants(R=3, C_=1, n=2, L=1, invariant_mask=2)
    w_state = m.compile_where(wr.text_of(wr.SET_A))

    def run(terminal, predicates):
        mc = vt.ModelChecker(m, table_log2=20, frontier_words=1 << 21, frontier_states=1 << 15, pending_entries=1 << 16)
        for _ in range(8):
            mc.step()
        if predicates:
            mc.deep_attach(w_state, None)
        if terminal:
            mc.deep_terminal_attach()
        rows = []
        while True:
            a, b = mc.deepen()
            rows.append(({k: a[k] for k in KEEP}, None if b is None else {k: b[k] for k in KEEP}))
            if a["viol_mask"] or (b is not None and b["viol_mask"]):
                break
        tr = [(a_, [int(x) for x in r]) for a_, r in mc.probe_trace()]
        viol = dict(mc.violation)
        strip = lambda rs, keys: [{k: v for k, v in r.items() if k not in keys} for r in rs]   # noqa: E731
        # (times apart, and the number of slices: the scratch buffers are cut from what the device has free, which the other attachment's buffers change)
        term = strip(mc.deep_terminal_results(), ("ms", "children_ms", "slices", "chunks")) if terminal else None
        pred = strip(mc.deep_results(), ("where_ms", "step_ms", "slices")) if predicates else None
        mc.close()
        return (rows, tr, viol), term, pred

    plain, _, _ = run(False, False)
    assert plain[0][-1][1]["level"] == 19 and plain[0][-1][1]["viol_mask"] == 2      # the violation of test_deep_search.py, found by the probe of the pass that inserts 18
    with_term, term, _ = run(True, False)
    assert with_term == plain                                       # level infos, checksums, the violation and its trace
    with_pred, _, pred = run(False, True)
    both, term2, pred2 = run(True, True)
    assert both == plain and with_pred == plain
    assert term2 == term and pred2 == pred                          # each attachment's results are what its separate run gave
    scanned = {r["level"]: r for r in term if r["kind"] != "probed"}
    assert sorted(scanned) == list(range(10, 19))
    assert {lvl: scanned[lvl]["n_terminal"] for lvl in range(11, 19)} == TERMINAL_3121
    assert {lvl: scanned[lvl]["n_states"] for lvl in range(11, 19)} == STATES_3121
    assert [r["level"] for r in term if r["kind"] == "probed"] == list(range(12, 20))


# ---------------------------------------------------------------------------------------------------------------------
# 6. the command line
# ---------------------------------------------------------------------------------------------------------------------
def _cli(tmp_path, args):
    cfg = tmp_path / "VSR.cfg"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_cfg.py"), str(cfg), "3", "1", "v1, v2", "1"], check=True)
    # (-frontierGiB 0.0004: the smallest record buffers the command line takes, 2 236 states — level 11 of (3,1,{v1,v2},1) has 2 533)
    return subprocess.run([CLI, "-config", str(cfg), "-noTLA", "-tableLog2", "20", "-frontierGiB", "0.0004"] + args, capture_output=True, text=True, timeout=300)


def _untimed(text):
    """the lines of a run without its times and without the name of the trace file"""
    out = []
    for ln in text.splitlines():
        if ln.startswith(("Finished in", "The counter-example was written")):
            continue
        out.append(re.sub(r"\d+\.\d+ ?s\b", "T s", re.sub(r"\d+ launches", "N launches", ln)))
    return out


def test_cli_check_deadlock_beyond_the_buffers(vt, tmp_path):
    out = str(tmp_path / "deadlock.tla")
    r = _cli(tmp_path, ["-checkDeadlock", "-deepTerminal", "-dumpTrace", "tla", out])
    print(r.stdout[:1500], r.stdout[-800:], r.stderr)
    assert r.returncode == 11, (r.returncode, r.stderr)
    assert "Error: Deadlock reached (4 state(s) of level 15 have no successor)." in r.stdout
    head = r.stdout.split("Error: Deadlock reached")[0]
    assert "Virtual(" in head and "Progress(15)" not in head
    assert len(re.findall(r"^State \d+: <", r.stdout, re.M)) == 15
    v = _cli(tmp_path, ["-validateTrace", out])
    assert v.returncode == 0 and "15 states read" in v.stdout and "The trace is a behaviour of the model." in v.stdout, v.stdout + v.stderr
    # without the switch: every line is what the build before this feature printed (recorded from it; the times and launch counts apart)
    r0 = _cli(tmp_path, ["-checkDeadlock", "-dumpTrace", "tla", out])
    golden = open(os.path.join(ROOT, "tests", "golden", "deep_terminal_cli_parent.txt")).read()
    assert r0.returncode == 11 and _untimed(r0.stdout) == golden.splitlines(), "\n".join(_untimed(r0.stdout))


@pytest.fixture(scope="module")
def whole_3121(orc):
    """(states per level, terminal states per level) of the whole space (3,1,{v1,v2},1) by the CPU oracle: 30 levels, once per module"""
    b = orc.Bfs(orc.Params(3, 1, 2, 1))
    states, term, n = [], [], 1
    while n:
        nn = b.step()
        states.append(n)
        term.append(b.info["deadlocks"])
        n = nn
    b.close()
    return states, term


def _report_line(stdout):
    """the `Terminal report:` line -> ([(level, terminal states)] as listed, total, levels with one, levels scanned, unsettled)"""
    line = [ln for ln in stdout.splitlines() if ln.startswith("Terminal report:")]
    assert len(line) == 1, line
    mt = re.match(r"Terminal report: (\d+) terminal states in (\d+) of (\d+) scanned levels(?: \((.*)\))?, (\d+) unsettled", line[0])
    assert mt, line[0]
    pairs = [(int(a), int(b)) for a, b in re.findall(r"level (\d+): (\d+)", mt.group(4) or "")]
    return pairs, int(mt.group(1)), int(mt.group(2)), int(mt.group(3)), int(mt.group(5))


def test_cli_terminal_report_rows_of_the_levels_beyond_the_buffers(vt, tmp_path, whole_3121):
    r = _cli(tmp_path, ["-terminalReport", "-deepTerminal", "-json", "-maxDepth", "18"])
    print(r.stdout[-2500:], r.stderr)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    deep = [x for x in rows if x.get("stored") is False and "kind" in x]
    virt = sorted(x["level"] for x in rows if x.get("stored") is False and "kind" not in x)
    scanned = {x["level"]: x for x in deep if x["kind"] != "probed"}
    assert len(virt) >= 3 and max(virt) == 18 and sorted(scanned) == virt, (virt, sorted(scanned))
    for lvl, x in scanned.items():
        assert x["exact"] is True and x["terminal"] == TERMINAL_3121.get(lvl, 0) and x["unsettled"] == 0, x   # (no terminal state through level 14)
    probed = {x["level"]: x for x in deep if x["kind"] == "probed"}
    assert sorted(probed) == sorted(x["probed_level"] for x in rows if "probed_level" in x)
    for lvl, x in probed.items():
        assert x["exact"] is True and (lvl > 18 or x["terminal"] == TERMINAL_3121.get(lvl, 0)), x
    term = whole_3121[1]
    assert [term[lvl - 1] for lvl in range(11, 19)] == [TERMINAL_3121[lvl] for lvl in range(11, 19)]
    assert probed[19]["terminal"] == term[18]
    # the report line: every level once (a list, not a set), the total and the number of scanned levels by the oracle — levels 1-18 and the probed level 19
    assert _report_line(r.stdout) == ([(lvl, term[lvl - 1]) for lvl in range(1, 20) if term[lvl - 1]], sum(term[:19]), 5, 19, 0)
    assert "counted, not listed" not in r.stdout and "Stuttering" not in r.stdout and "lower bounds" not in r.stdout
    assert "Terminal states were examined through level 19" in r.stdout


def test_cli_terminal_report_counts_a_probed_level_that_is_stored_later_once(vt, tmp_path, whole_3121):
    """The whole space: the levels shrink at the end, the search re-bases onto level 28 after it has examined level 29 as the probed level, and levels 29 and
    30 are stored and scanned as stored levels.  Every level is in the report once."""
    states, term = whole_3121
    r = _cli(tmp_path, ["-terminalReport", "-deepTerminal"])
    print(r.stdout[-3000:], r.stderr)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rebased = [int(x) for x in re.findall(r"^Re-based\((\d+)\)", r.stdout, re.M)]
    probes = [int(x) for x in re.findall(r"^Probe\((\d+)\)", r.stdout, re.M)]
    later = [int(x) for x in re.findall(r"^Progress\((\d+)\)", r.stdout.split("Re-based(%d)" % rebased[-1])[1], re.M)]
    # (else this test is not about what its name says: a level examined as the probed level, then re-based under, then stored; and that level has terminal states)
    assert rebased and rebased[-1] + 1 in probes and rebased[-1] + 1 in later and term[rebased[-1]] > 0, (rebased, probes, later)
    top = len(states)
    assert "%d distinct states found" % sum(states) in r.stdout
    assert _report_line(r.stdout) == ([(lvl, term[lvl - 1]) for lvl in range(1, top + 1) if term[lvl - 1]], sum(term), sum(1 for t in term if t), top, 0)
    assert "counted, not listed" not in r.stdout and "Stuttering" not in r.stdout and "lower bounds" not in r.stdout
    assert ("Terminal states were examined through level %d" % top) in r.stdout


def test_attachment_refusals(vt):
    """where the deep passes are refused anyway: exact_ties checkers, and a state or an action constraint on either side of the attachment"""
    import step_reference as sr
    import where_reference as wr
    m = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
    sizes = dict(table_log2=16, frontier_words=1 << 18, frontier_states=1 << 13, pending_entries=1 << 14)
    mc = vt.ModelChecker(m, exact_ties=True, **sizes)
    with pytest.raises(vt.VsrmcError) as e:
        mc.deep_terminal_attach()
    assert e.value.code == -6 and "single-pass checker" in e.value.message
    mc.close()
    w = m.compile_where(wr.text_of(wr.SET_A))
    ws = m.compile_step(sr.text_of(sr.FIVE[:1]))
    for attach in (lambda c: c.constrain(w, wr.SET_A[0][0]), lambda c: c.action_constrain(ws, sr.FIVE[0][0])):
        mc = vt.ModelChecker(m, **sizes)
        attach(mc)
        with pytest.raises(vt.VsrmcError) as e:
            mc.deep_terminal_attach()
        assert e.value.code == -6 and "constraint is attached" in e.value.message, e.value.message
        mc.close()
        mc = vt.ModelChecker(m, **sizes)
        mc.deep_terminal_attach()
        with pytest.raises(vt.VsrmcError) as e:
            attach(mc)
        assert e.value.code == -6 and "terminal attachment" in e.value.message, e.value.message
        mc.close()
