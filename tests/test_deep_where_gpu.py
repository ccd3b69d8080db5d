"""A user's predicates on the levels beyond the record buffers (`-m gpu`): ModelChecker.deep_attach / deep_results / deep_where_states /
deep_step_pairs / deep_witness_trace and run(deep=True) — csrc/host_deep_where.hpp, k_probe_where (csrc/vsr_deep_where.hpp).

Every expected value comes from a route that is pinned elsewhere: the stored-level scans (where_scan / step_scan) of a second checker whose buffers hold
the whole space, the CPU oracle's levels, and the hand-written Python predicates of where_reference.py / step_reference.py over pycodec's unpack of the
oracle's records.  Every comparison is exact.  The state predicates are where_reference.SET_A (eight exports, LogDivergence among them; none reads an aux
variable, so that every copy of a state has the same bits), the step predicates step_reference.FIVE plus three of its set A."""
import collections

import numpy as np
import pytest

import step_reference as sr
import where_reference as wr

pytestmark = pytest.mark.gpu

STATE = wr.SET_A
STEP = sr.FIVE + [p for p in sr.SET_A if p[0] in ("ViewChanged", "BecameNormal", "Delivered")]
BIG = dict(table_log2=20, frontier_words=1 << 22, frontier_states=1 << 17, pending_entries=1 << 17)
Level = collections.namedtuple("Level", "level recs states fps generated")


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
    """(R, C, n, L, depth) -> (oracle params, python model, {level: Level}): the oracle's BFS once per space — records, their Python view, their
    fingerprints, `generated` of the step that produced the level; shared, never changed"""
    from oracle import pycodec, pyoracle as po
    cache = {}

    def get(key):
        if key not in cache:
            R, C, n, L, depth = key
            P = orc.Params(R, C, n, L)
            PM = po.Model(R, C, tuple("v%d" % (i + 1) for i in range(n)), L)
            b = orc.Bfs(P)
            init = orc.init_record(P)
            words, off, level, gen, out = init, np.array([0, len(init)], dtype=np.uint64), 1, 0, {}
            while True:
                recs = [words[int(off[i]): int(off[i + 1])] for i in range(len(off) - 1)]
                out[level] = Level(level, recs, [pycodec.unpack(PM, [int(x) for x in r]) for r in recs], [orc.fingerprint(P, r)[0] for r in recs], gen)
                if (depth is not None and level >= depth) or b.step() == 0:
                    break
                level += 1
                gen = b.info["generated"]
                words, off = b.frontier()
            b.close()
            cache[key] = (P, PM, out)
        return cache[key]
    return get


def _stored(vt, m, w_state, w_step, upto):
    """level -> (where_scan, where_states, step_scan, step_pairs) of a checker that stores every level"""
    mc = vt.ModelChecker(m, **BIG)
    out = {}
    while True:
        ws = mc.where_scan(w_state)
        st = mc.where_states()
        ss = mc.step_scan(w_step) if w_step is not None else None
        sp = mc.step_pairs() if w_step is not None else None
        out[mc.level] = (ws, st, ss, sp)
        if (upto is not None and mc.level >= upto) or mc.step()["n_new"] == 0:
            break
    mc.close()
    return out


def _python_hits(lv, preds):
    """the oracle's level through the Python predicates -> (count per predicate, min fingerprint per predicate, sorted [(fp, bits)] of the hits)"""
    count, mins, hits = [0] * len(preds), [None] * len(preds), []
    for s, fp in zip(lv.states, lv.fps):
        bits = wr.bits_of(preds, s)
        if bits:
            hits.append((int(fp), bits))
        for k in range(len(preds)):
            if (bits >> k) & 1:
                count[k] += 1
                mins[k] = int(fp) if mins[k] is None else min(mins[k], int(fp))
    return count, mins, sorted(hits)


def _check_state(r, mc, stored, lv, n_preds, probed, listed):
    ws, (fps, bits) = stored[0], stored[1]
    assert r["state"]["count"] == ws["count"] and r["state"]["min_fp"] == ws["min_fp"], (r["level"], r["kind"])
    count, mins, hits = _python_hits(lv, STATE)
    assert r["state"]["count"] == count and r["state"]["min_fp"] == mins, (r["level"], r["kind"])
    if not probed:
        assert r["state"]["n_states"] == ws["n_states"] == len(lv.recs)
    assert r["exact"] is True
    if listed:
        f, b = mc.deep_where_states(r["level"], probed=probed)
        assert [int(x) for x in f] == [int(x) for x in fps] and [int(x) for x in b] == [int(x) for x in bits], (r["level"], r["kind"])
        assert list(zip([int(x) for x in f], [int(x) for x in b])) == hits
        assert r["n_hit_states"] == len(hits)


def _check_step(r, mc, stored, nxt, listed):
    ss, (pf, po_, pb) = stored[2], stored[3]
    assert (r["step"]["n_states"], r["step"]["n_pairs"], r["step"]["n_err"]) == (ss["n_states"], ss["n_pairs"], ss["n_err"]), r["level"]
    assert r["step"]["count"] == ss["count"] and r["step"]["min_fp"] == ss["min_fp"], r["level"]
    if nxt is not None:
        assert r["step"]["n_pairs"] + r["step"]["n_err"] == nxt.generated, r["level"]
    if listed:
        f, o, b = mc.deep_step_pairs(r["level"])
        # (the ordinal caveat of include/vsrmc.h: an ordinal is a position in the bag of the record as THAT run holds it — the pairs of a parent are compared
        # as the multiset of their bits)
        assert sorted(zip([int(x) for x in f], [int(x) for x in b])) == sorted(zip([int(x) for x in pf], [int(x) for x in pb])), r["level"]
        assert r["n_hit_pairs"] == len(pf)


def _deepen_all(mc, stop_level=None):
    """deepen() until the space is exhausted (or stop_level is inserted) -> ([inserted dicts], {(level, probed): result, each as FIRST reported},
    {key: the pass that reported it})"""
    ins, seen, first_pass = [], {}, {}
    n_pass = 0
    while True:
        a, b = mc.deepen()
        n_pass += 1
        if a["n_new"] == 0:
            break
        ins.append(a)
        for r in mc.deep_results():
            key = (r["level"], r["kind"] == "probed")
            if key not in seen:
                seen[key] = r
                first_pass[key] = n_pass
            else:                                                   # reported once: a later pass regenerates the level and leaves its figures alone
                assert {k: v for k, v in r.items()} == {k: v for k, v in seen[key].items()}, key
        if stop_level is not None and a["level"] >= stop_level:
            break
    return ins, seen, first_pass


# ---------------------------------------------------------------------------------------------------------------------
# 1. a whole small space
# ---------------------------------------------------------------------------------------------------------------------
def test_whole_small_space_report_mode(vt, spaces):
    """(2,1,{v1,v2},2), the space of test_rolling_deep_search_exhausts_a_small_space: 2 073 states (27 levels by the oracle); three stored levels, then
    deepen() to exhaustion with both programs attached"""
    key = (2, 1, 2, 2, None)
    P, PM, levels = spaces(key)
    m = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
    w_state, w_step = m.compile_where(wr.text_of(STATE)), m.compile_step(sr.text_of(STEP))
    stored = _stored(vt, m, w_state, w_step, None)
    top = max(levels)
    assert sorted(stored) == sorted(levels) and sum(len(lv.recs) for lv in levels.values()) == 2073
    mc = vt.ModelChecker(m, table_log2=16, frontier_words=1 << 20, frontier_states=1 << 14, pending_entries=1 << 15)
    for _ in range(3):
        mc.step()
    mc.deep_attach(w_state, w_step)
    assert mc.deep_results() == []
    base = mc.level
    checked = collections.Counter()
    while True:
        a, b = mc.deepen()
        if a["n_new"] == 0:
            break
        assert a["viol_mask"] == 0 and len(levels[a["level"]].recs) == a["n_new"]
        new = [r for r in mc.deep_results() if (r["level"], r["kind"]) not in checked]
        for r in new:
            checked[(r["level"], r["kind"])] += 1
            lv = levels[r["level"]]
            _check_state(r, mc, stored[r["level"]], lv, len(STATE), r["kind"] == "probed", True)
            if r["kind"] == "probed":
                assert r["step"] is None and b is not None and b["level"] == r["level"]
            else:
                _check_step(r, mc, stored[r["level"]], levels.get(r["level"] + 1), True)
    got = collections.Counter(lv for lv, _ in checked)
    # every level beyond the base was scanned as a regenerated or inserted level, exactly once
    scanned = sorted(lv for (lv, kind) in checked if kind != "probed")
    assert scanned == list(range(base + 1, top + 1)), scanned
    assert all(n == 1 for n in checked.values())
    # ... and from the second pass on every pass reported the level after the one it inserted as the probed level
    probed = sorted(lv for (lv, kind) in checked if kind == "probed")
    assert probed == list(range(base + 3, top + 1)), probed
    assert got[top] == 2
    final = {(r["level"], r["kind"]): r for r in mc.deep_results()}
    assert final[(base + 1, "regenerated")]["kind"] == "regenerated" and final[(top, "inserted")]["state"]["n_states"] == len(levels[top].recs)
    hit = [k for k in range(len(STATE)) if any(r["state"]["count"][k] for r in final.values())]
    want_hit = [k for k in range(len(STATE)) if any(_python_hits(levels[lvl], STATE)[0][k] for lvl in range(base + 1, top + 1))]
    assert hit == want_hit and len(want_hit) >= 2, (hit, want_hit)  # (the oracle's: the predicates are not vacuous beyond the base)
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. more than one slice: the figures of a level accumulate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob", [None, ("VSRMC_STEP_SLICE", "7"), ("VSRMC_WHERE_LIST_CAP", "4"), ("VSRMC_DEEP_INSTANCE_CAP", "256"), ("VSRMC_STEP_LIST_CAP", "4")],
                         ids=["plain", "small-sub-slices", "state-list-of-4", "halve-and-retry", "pair-list-of-4"])
def test_levels_that_pass_in_several_slices(vt, spaces, knob, monkeypatch):
    """(3,1,{v1,v2},1), levels 8-14 beyond a base of 7, with record buffers so small that a pass takes several slices and sub-slices"""
    if knob:
        monkeypatch.setenv(*knob)
    if knob and knob[0] == "VSRMC_DEEP_INSTANCE_CAP":
        # a sub-slice sized by the library cannot overflow its list; one of 100 000 parents — every scratch slice whole — does whenever the slice has more than
        # 256 enabled instances, and is then run again in halves
        monkeypatch.setenv("VSRMC_STEP_SLICE", "100000")
    key = (3, 1, 2, 1, 15)
    P, PM, levels = spaces(key)
    m = vt.Model.from_constants(R=3, C_=1, n=2, L=1)
    w_state, w_step = m.compile_where(wr.text_of(STATE)), m.compile_step(sr.text_of(STEP))
    if knob and knob[0] in ("VSRMC_WHERE_LIST_CAP", "VSRMC_STEP_LIST_CAP"):
        monkeypatch.delenv(knob[0])                                 # (the stored scans keep their full lists)
    stored = _stored(vt, m, w_state, w_step, 15)
    if knob:
        monkeypatch.setenv(*knob)
    mc = vt.ModelChecker(m, table_log2=20, frontier_words=1 << 17, frontier_states=1 << 13, pending_entries=1 << 16)
    for _ in range(6):
        mc.step()
    assert mc.level == 7
    mc.deep_attach(w_state, w_step)
    ins, seen, _ = _deepen_all(mc, stop_level=14)
    shapes = [(a["words_new"] >> 32, a["words_new"] & 0xFFFFFFFF) for a in ins]
    print("slices, sub-slices per pass:", shapes)
    assert any(s >= 2 and t >= 2 for s, t in shapes), shapes       # else nothing here is about accumulation
    for lvl in range(8, 15):
        r = seen[(lvl, False)]
        assert r["kind"] in ("regenerated", "inserted")
        listed = knob is None or knob[0] != "VSRMC_WHERE_LIST_CAP"
        lv = levels[lvl]
        ws = stored[lvl][0]
        count, mins, hits = _python_hits(lv, STATE)
        assert r["state"]["count"] == ws["count"] == count and r["state"]["min_fp"] == ws["min_fp"] == mins, lvl
        assert r["state"]["n_states"] == len(lv.recs) and r["n_hit_states"] == len(hits)
        _check_step(r, mc, stored[lvl], levels.get(lvl + 1), False)
        if knob and knob[0] == "VSRMC_DEEP_INSTANCE_CAP" and lvl >= 12:
            # an instance list of 256 entries: a sub-slice of more than 256 enabled instances overflows it and is run again in halves — more launches of
            # k_step_list than an unhalved run of the same slices needs, and the same figures
            # (more pairs than 256 per scratch slice: some slice overflowed the list on its first launch; an unhalved run has one launch per slice)
            assert r["step"]["n_pairs"] > 256 * r["slices"] and r["step"]["slices"] > r["slices"], (lvl, r["step"], r["slices"])
        if lvl >= 10:
            p = seen[(lvl, True)]
            if p["exact"]:
                assert p["state"]["count"] == count and p["state"]["min_fp"] == mins, lvl
            else:                                                   # an overflowed list of copies: lower bounds, never reported as exact
                assert knob and knob[0] == "VSRMC_WHERE_LIST_CAP"
                assert all(a <= b for a, b in zip(p["state"]["count"], count)), lvl
        if listed:
            assert r["slices"] >= 1
    # the lists of the levels the last pass scanned
    last = max(lvl for (lvl, probed) in seen if not probed)
    if knob and knob[0] == "VSRMC_STEP_LIST_CAP":                   # the hit-pair list overflows: counts and minima stay exact (checked above), the list call says so
        n_hits = len(stored[last][3][0])
        assert n_hits > 4
        with pytest.raises(vt.VsrmcError) as e:
            mc.deep_step_pairs(last)
        assert e.value.code == -5 and ("has %d," % n_hits) in e.value.message, e.value.message
        _check_state(seen[(last, False)], mc, stored[last], levels[last], len(STATE), False, True)
    elif knob and knob[0] == "VSRMC_WHERE_LIST_CAP":
        count, mins, hits = _python_hits(levels[last], STATE)
        assert len(hits) > 4
        with pytest.raises(vt.VsrmcError) as e:
            mc.deep_where_states(last)
        assert e.value.code == -5 and ("has %d," % len(hits)) in e.value.message, e.value.message
    else:
        _check_state(seen[(last, False)], mc, stored[last], levels[last], len(STATE), False, True)
        _check_step(seen[(last, False)], mc, stored[last], levels.get(last + 1), True)
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. reach, in each kind of level
# ---------------------------------------------------------------------------------------------------------------------
def _norm(fixed, r):
    return tuple(int(x) for x in r[:fixed]) + tuple(sorted(int(x) for x in r[fixed:]))


def test_reach_in_a_probed_an_inserted_and_a_regenerated_level(vt, orc, spaces):
    key = (3, 1, 2, 1, 15)
    P, PM, levels = spaces(key)
    k_div = [p[0] for p in STATE].index("LogDivergence")
    F = min(lvl for lvl, lv in levels.items() if any(wr.log_divergence(s) for s in lv.states))
    want_fp = min(int(fp) for s, fp in zip(levels[F].states, levels[F].fps) if wr.log_divergence(s))
    print("LogDivergence first at level", F)
    assert 5 <= F <= 14
    m = vt.Model.from_constants(R=3, C_=1, n=2, L=1)
    w = m.compile_where("LogDivergence == " + wr.LOG_DIVERGENCE)
    fixed = int(m.layout.fixed_words)
    traces = []
    for base, kind in ((F - 3, "probed"), (F - 2, "inserted"), (F - 1, "regenerated")):
        for rerun in range(2 if kind == "probed" else 1):
            mc = vt.ModelChecker(m, table_log2=20, frontier_words=1 << 21, frontier_states=1 << 15, pending_entries=1 << 16)
            for _ in range(base - 1):
                mc.step()
            assert mc.level == base
            # pass 1 makes level base + 1 a seen-set-only level and writes no records; run() then attaches and its first advance() — the automatic scheme's
            # own deepen — regenerates base + 1, inserts base + 2 and probes base + 3: level F is the probed, the inserted or the regenerated one
            a, _b = mc.deepen()
            assert a["level"] == base + 1 and mc.depth != mc.level
            verdict = mc.run(reach=w, deep=True)
            assert mc.depth == base + 2
            assert verdict == "reached"
            wit = mc.witness
            assert (wit["level"], wit["fp"], wit["kind_of_level"], wit["name"]) == (F, want_fp, kind, "LogDivergence"), wit
            tr = mc.deep_witness_trace()
            assert len(tr) == F
            rec = orc.init_record(P)
            assert np.array_equal(tr[0][1], rec)
            for act, wd in tr[1:]:
                f = orc.fingerprint(P, wd)[0]
                nxt = [s for s in orc.successors(P, rec) if s["fp"] == f]
                assert nxt, "a state of the witness is not a successor of its predecessor (%s)" % act
                rec = nxt[0]["words"]
            from oracle import pycodec
            assert wr.log_divergence(pycodec.unpack(PM, [int(x) for x in tr[-1][1]]))
            assert orc.fingerprint(P, tr[-1][1])[0] == want_fp
            traces.append([_norm(fixed, r) for _, r in tr])
            mc.close()
    assert all(t == traces[0] for t in traces[1:])                 # the same behaviour in two runs and from all three bases


# ---------------------------------------------------------------------------------------------------------------------
# 4. a user's restatement of a built-in invariant, found where the built-in one is found
# ---------------------------------------------------------------------------------------------------------------------
def test_restated_invariant_is_violated_in_the_probed_level(vt, orc):
    P = orc.Params(3, 1, 2, 1, invariant_mask=2)
    ob = orc.Bfs(P)
    while not ob.info.get("viol_mask"):
        assert ob.step()
    assert ob.info["depth"] == 19
    words, off = ob.frontier()
    viol = min(orc.fingerprint(P, words[int(off[i]): int(off[i + 1])])[0] for i in range(len(off) - 1) if orc.invariants(P, words[int(off[i]): int(off[i + 1])]))
    ob.close()
    m = vt.Model.from_constants(R=3, C_=1, n=2, L=1, invariant_mask=0)
    never = m.compile_where(wr.ACK_TEXT.replace("OnMajority ==", "LOCAL OnMajorityHolds ==").replace("HasNotLost ==", "LOCAL HasNotLost ==")
                            .replace("CommittedDivergence ==", "LOCAL CommittedDivergence ==") + "\nNotOnMajority == ~OnMajorityHolds\n")
    assert never.names == ["NotOnMajority"]
    mc = vt.ModelChecker(m, table_log2=20, frontier_words=1 << 21, frontier_states=1 << 15, pending_entries=1 << 16)
    for _ in range(11):
        mc.step()
    assert mc.level == 12
    # (buffers that hold level 12 would let the automatic scheme re-base onto a later level and find the state in a stored one: here every unit of
    # progress is a deepen; run() through the scheme's own advance() is what the reach and the step tests do)
    mc.advance = lambda: (lambda a, b: ("deep", a, b))(*mc.deepen())
    assert mc.run(never=never, deep=True) == "violation"
    wit = mc.witness
    assert (wit["level"], wit["fp"], wit["kind_of_level"]) == (19, int(viol), "probed"), wit
    assert mc.depth == 18                                           # found by the probe of the pass that inserts 18
    tr = mc.deep_witness_trace()
    assert len(tr) == 19 and orc.fingerprint(P, tr[-1][1])[0] == viol and orc.invariants(P, tr[-1][1]) == 2
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. a step invariant beyond the buffers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2])
def test_step_invariant_beyond_the_buffers(vt, orc, n):
    """n = 2: SYMMETRY has two permutations, and the record the witness replays may be another member of the parent's orbit than the one the scratch
    slice held — the instance is found again on the replayed record"""
    from oracle import pycodec, pyoracle as po
    m = vt.Model.from_constants(R=3, C_=1, n=n, L=1, invariant_mask=0)
    PM = po.Model(3, 1, tuple("v%d" % (i + 1) for i in range(n)), 1)
    P = orc.Params(3, 1, n, 1, invariant_mask=0)
    w = m.compile_step("NotCommitMonotonic == ~(" + sr.COMMIT_MONOTONIC + ")")
    ref = vt.ModelChecker(m, **BIG)
    assert ref.run(step_never=w) == "violation"
    want = dict(ref.witness)
    ref.close()
    Pl = want["level"]
    print("~CommitMonotonic, %d value(s): parent level %d, action %s" % (n, Pl, want["action"]))
    assert 4 <= Pl <= 14
    for base, kind in ((Pl - 2, "inserted"), (Pl - 1, "regenerated")):
        mc = vt.ModelChecker(m, table_log2=20, frontier_words=1 << 21, frontier_states=1 << 15, pending_entries=1 << 16)
        for _ in range(base - 1):
            mc.step()
        # pass 1 makes level base + 1 a seen-set-only level and writes no records.  run() attaches; its first advance() regenerates base + 1 and inserts
        # base + 2: the parent level is the inserted one from base Pl - 2 and the regenerated one from base Pl - 1
        mc.deepen()
        assert mc.run(step_never=w, deep=True) == "violation"
        wit = mc.witness
        assert (wit["level"], wit["fp"], wit["kind_of_level"], wit["program"]) == (Pl, want["fp"], kind, "step"), (wit, want)
        tr = mc.deep_witness_trace()
        assert len(tr) == Pl + 1
        if n == 1:                                                  # (without SYMMETRY the replayed record is the stored one: the same instance)
            assert tr[-1][0] == want["action"]
        assert orc.fingerprint(P, tr[-2][1])[0] == want["fp"]
        p, c = (pycodec.unpack(PM, [int(x) for x in r]) for r in (tr[-2][1], tr[-1][1]))
        assert not sr.commit_monotonic(p, c, tr[-1][0])
        nxt = [x for x in orc.successors(P, tr[-2][1]) if x["fp"] == orc.fingerprint(P, tr[-1][1])[0]]
        assert nxt and vt.ACTION_NAMES[nxt[0]["action"]] == tr[-1][0]
        mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the analysis models
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["second", "third"])
def test_analysis_models(vt, which):
    """VR_STATE_TRANSFER / VR_APP_STATE on (3, {v1,v2} / {a,b}, 1): InStateTransfer, first at level 11, found in the probed level from a base of 8 with the
    stored run's fingerprint and a behaviour the Python oracle accepts; and the report of a state and a step program over the deep levels 9-11
    (k_probe_where<1>, <2> on levels 11 and 12) against a checker that stores them and the oracle's levels"""
    import step_models_reference as sm
    import where_models_reference as wm
    from oracle import orc2, orc3, pyoracle2, pyoracle3
    orc_, po = (orc2, pyoracle2) if which == "second" else (orc3, pyoracle3)
    values = ("v1", "v2") if which == "second" else ("a", "b")
    P = orc_.Params(3, 2, 1)
    PM = po.Model(3, values, 1)
    b = orc_.Bfs(P)
    init = orc_.init_record(P)
    words, off, level, levels = init, np.array([0, len(init)], dtype=np.uint64), 1, {}
    while True:
        recs = [words[int(off[i]): int(off[i + 1])] for i in range(len(off) - 1)]
        levels[level] = ([po.unpack(PM, [int(x) for x in r]) for r in recs], [int(orc_.fingerprint(P, r)[0]) for r in recs], b.info.get("generated", 0) if level > 1 else 0)
        if level >= 12:
            break
        assert b.step()
        level += 1
        words, off = b.frontier()
    b.close()

    def hits(lvl):
        f = [fp for s, fp in zip(levels[lvl][0], levels[lvl][1]) if wm.in_state_transfer(s)]
        return len(f), (min(f) if f else None)

    first = min(lvl for lvl in levels if hits(lvl)[0])
    assert first == 11
    want_fp = hits(11)[1]
    m = (vt.Model.second_model if which == "second" else vt.Model.third_model)(R=3, n=2, L=1)
    w = m.compile_predicates("InStateTransfer == " + wm.set_a(values)[0][1])
    w_step = m.compile_step_predicates("CommitMonotonic == " + sm.COMMIT_MONOTONIC + "\nEnters == " + sm.ENTERS)
    sizes = dict(table_log2=20, frontier_words=1 << 24, frontier_states=1 << 20, pending_entries=1 << 19)
    ref = vt.ModelChecker(m, **sizes)
    stored = {}
    while ref.level < 11:
        ref.step()
        if ref.level >= 9:
            stored[ref.level] = (ref.where_scan(w), ref.step_scan(w_step))
    assert stored[11][0]["min_fp"][0] == want_fp and stored[11][0]["count"][0] == hits(11)[0] and stored[10][0]["count"][0] == 0
    ref.close()
    # reach, in the probed level
    mc = vt.ModelChecker(m, **sizes)
    for _ in range(7):
        mc.step()
    assert mc.level == 8
    mc.deepen()
    assert mc.run(reach=w, deep=True) == "reached" and mc.depth == 10
    wit = mc.witness
    assert (wit["level"], wit["fp"], wit["kind_of_level"], wit["name"], wit["exact"]) == (11, want_fp, "probed", "InStateTransfer", True), wit
    tr = mc.deep_witness_trace()
    mc.close()
    assert len(tr) == 11 and tr[0][0] == "Initial predicate"
    states = [po.unpack(PM, [int(x) for x in r]) for _, r in tr]
    assert po.view_of(states[0]) == po.view_of(po.Init(PM))
    for s0, s1 in zip(states, states[1:]):                          # every consecutive pair is a (state, successor) of the Python oracle
        assert po.view_of(s1) in [po.view_of(t) for _, t in po.successors(PM, s0)]
    assert wm.in_state_transfer(states[-1]) and int(orc_.fingerprint(P, tr[-1][1])[0]) == want_fp
    # report, both programs, levels 9-11 scanned and 11-12 probed
    mc = vt.ModelChecker(m, **sizes)
    for _ in range(7):
        mc.step()
    mc.deep_attach(w, w_step)
    for _ in range(4):
        a, _b = mc.deepen()
    assert a["level"] == 12
    res = {(r["level"], r["kind"] == "probed"): r for r in mc.deep_results()}
    mc.close()
    for lvl in (9, 10, 11):
        r = res[(lvl, False)]
        ws, ss = stored[lvl]
        assert r["state"]["n_states"] == ws["n_states"] == len(levels[lvl][0]) and r["state"]["count"] == ws["count"] == [hits(lvl)[0]], lvl
        assert r["state"]["min_fp"] == ws["min_fp"] == [hits(lvl)[1]], lvl
        assert (r["step"]["n_states"], r["step"]["n_pairs"], r["step"]["n_err"], r["step"]["count"], r["step"]["min_fp"]) == (
            ss["n_states"], ss["n_pairs"], ss["n_err"], ss["count"], ss["min_fp"]), lvl
        assert r["step"]["n_pairs"] + r["step"]["n_err"] == levels[lvl + 1][2], lvl
        assert r["step"]["count"][0] > 0                            # (the program is not vacuous)
    for lvl in (11, 12):
        r = res[(lvl, True)]
        assert r["exact"] is True and r["state"]["count"] == [hits(lvl)[0]] and r["state"]["min_fp"] == [hits(lvl)[1]], lvl
    assert hits(12)[0] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. off means off
# ---------------------------------------------------------------------------------------------------------------------
def test_off_means_off(vt, orc):
    m = vt.Model.from_constants(R=3, C_=1, n=2, L=1, invariant_mask=2)
    w_state, w_step = m.compile_where(wr.text_of(STATE)), m.compile_step(sr.text_of(STEP))

    def run(mode):
        mc = vt.ModelChecker(m, table_log2=20, frontier_words=1 << 21, frontier_states=1 << 15, pending_entries=1 << 16)
        for _ in range(8):
            mc.step()
        if mode == "attached":
            mc.deep_attach(w_state, w_step)
        if mode == "detached":
            mc.deep_attach(w_state, w_step)
            mc.deep_attach(None, None)
        rows = []
        keep = ("level", "frontier", "generated", "n_new", "distinct", "total_generated", "deadlocks", "max_bag", "viol_fp", "viol_mask", "act_generated", "fp_xor",
                "fp_sum")
        while True:
            a, b = mc.deepen()
            rows.append(({k: a[k] for k in keep}, None if b is None else {k: b[k] for k in keep}))
            if mode != "attached":
                with pytest.raises(vt.VsrmcError) as e:             # a seen-set-only level is still refused by the stored-level scan
                    mc.where_scan(w_state)
                assert e.value.code == -6
            if a["viol_mask"] or (b is not None and b["viol_mask"]):
                break
        tr = mc.probe_trace()
        if mode != "attached":
            with pytest.raises(vt.VsrmcError):
                capi_levels(vt, mc)
        mc.close()
        return rows, [(a, [int(x) for x in r]) for a, r in tr]

    def capi_levels(vt, mc):
        import ctypes as C
        n = C.c_uint64()
        vt.capi.check(vt.load().vsrmc_checker_deep_levels(mc._h, None, None, 0, C.byref(n)))

    plain = run("plain")
    assert plain[0][-1][1]["level"] == 19 and plain[0][-1][1]["viol_mask"] == 2      # the violation of test_deep_search.py, found by the probe of the pass that inserts 18
    assert run("detached") == plain
    assert run("attached") == plain                                 # the search itself is untouched


# ---------------------------------------------------------------------------------------------------------------------
# 8. the command line
# ---------------------------------------------------------------------------------------------------------------------
def _cli(tmp_path, consts, text, args):
    import json as _json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = tmp_path / "VSR.cfg"
    subprocess.run([sys.executable, os.path.join(root, "tools", "make_cfg.py"), str(cfg)] + consts, check=True)
    pred = tmp_path / "predicates.txt"
    pred.write_text(text + "\n")
    # (-frontierGiB 0.0004: the smallest record buffers the command line takes, 2 236 states — level 11 of (3,1,{v1,v2},1) has 2 533)
    r = subprocess.run([os.path.join(root, "vsr_tlaplus_amd", "vsrmc"), "-config", str(cfg), "-noTLA", "-predicates", str(pred), "-tableLog2", "20", "-frontierGiB", "0.0004"]
                       + args, capture_output=True, text=True, timeout=300)
    rows = []
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            rows.append(_json.loads(line))
    return r, rows


def test_cli_queries_beyond_the_buffers(vt, orc, tmp_path):
    """The record buffers of the command line hold level 10 of (3,1,{v1,v2},1), where LogDivergence first holds: the query here is the restated
    AcknowledgedWritesExistOnMajority, first false at level 19 — eight levels beyond them — asked as -reach of its negation and as -invariant."""
    import re
    text = wr.ACK_TEXT + "\nNotOnMajority == ~OnMajority\n"
    for args, code, head in ((["-reach", "NotOnMajority"], 0, "State satisfying NotOnMajority found at depth 19"),
                             (["-invariant", "OnMajority"], 12, "Error: Invariant OnMajority is violated.")):
        r, _ = _cli(tmp_path, ["3", "1", "v1, v2", "1"], text, args + ["-deepPredicates"])
        out = r.stdout
        print(out[:1500], out[-600:], r.stderr)
        assert r.returncode == code, (r.returncode, r.stderr)
        virt = [int(x) for x in re.findall(r"^Virtual\((\d+)\)", out, re.M)]
        assert virt and min(virt) <= 12 and max(virt) == 18, virt    # left the record buffers long before; found by the probe of the pass that inserts 18
        assert "Progress(19)" not in out and head in out and "The behavior up to this point is:" in out
        assert len(re.findall(r"^State \d+: <", out, re.M)) == 19
        assert "Beyond the record buffers, states were examined through level 19." in out and "not examined" not in out
    # without the flag the same run never sees the state: the levels beyond the buffers are not examined, and the report says so
    r, _ = _cli(tmp_path, ["3", "1", "v1, v2", "1"], text, ["-reach", "NotOnMajority", "-maxDepth", "19"])
    assert r.returncode == 14 and "not examined" in r.stdout, (r.returncode, r.stdout[-800:])


def test_cli_where_report_rows_of_the_levels_beyond_the_buffers(vt, spaces, tmp_path):
    P, PM, levels = spaces((3, 1, 2, 1, 15))
    r, rows = _cli(tmp_path, ["3", "1", "v1, v2", "1"], wr.text_of(STATE), ["-whereReport", "-deepPredicates", "-json", "-maxDepth", "14"])
    print(r.stdout[-2500:], r.stderr)
    assert r.returncode == 0, (r.returncode, r.stderr)
    deep = [x for x in rows if x.get("stored") is False and "kind" in x]
    scanned = {x["level"]: x for x in deep if x["kind"] != "probed"}
    probed = {x["level"]: x for x in deep if x["kind"] == "probed"}
    virt = sorted(x["level"] for x in rows if x.get("stored") is False and "kind" not in x)
    assert len(virt) >= 3 and max(virt) == 14 and sorted(scanned) == virt and len(deep) == len(scanned) + len(probed), (virt, sorted(scanned))
    # the probed levels are the search's own (its "probed_level" lines: where the built-in invariants looked); a pass that starts from a stored level — the
    # first one, and the first one after a re-basing — inserts a level and probes nothing
    assert sorted(probed) == sorted(x["probed_level"] for x in rows if "probed_level" in x) and max(probed) == 15, (sorted(probed), virt)
    names = [p[0] for p in STATE]
    for lvl, x in list(scanned.items()) + list(probed.items()):
        count, _mins, _hits = _python_hits(levels[lvl], STATE)
        assert x["exact"] is True and [x["where"][nm] for nm in names] == count, (lvl, x)
    import re
    for line in r.stdout.splitlines():                              # no level is counted twice, re-based or not, and none is missing
        if line.startswith("Where report: Unsettled holds"):
            listed = [int(x) for x in re.findall(r"level (\d+):", line)]
            k_uns = names.index("Unsettled")
            assert listed == [lvl for lvl in range(1, 15) if _python_hits(levels[lvl], STATE)[0][k_uns]], listed
            want = sum(_python_hits(levels[lvl], STATE)[0][names.index("Unsettled")] for lvl in range(1, 15))
            assert ("holds in %d of %d states" % (want, sum(len(levels[lvl].recs) for lvl in range(1, 15)))) in line, line
            break
    else:
        raise AssertionError("no report line")
    assert "not examined" not in r.stdout and "Beyond the record buffers, states were examined through level 15." in r.stdout
