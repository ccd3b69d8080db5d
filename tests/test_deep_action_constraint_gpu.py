"""Action constraints on the levels beyond the record buffers (`-m gpu`): k_step_expand's insert, stored and probe modes through
ModelChecker.action_constrain(.., deep=True) / deepen / advance / run / check / probe / action_constraint_deep_results, the traces and the CLI's
-deepActionConstraint, against tests/action_constraint_reference.py::constrained_bfs — the Python BFS over the CPU oracles' successor function that skips
every transition a hand-written Python predicate forbids, and knows nothing of buffers.  A reference is computed once per space and shared.  Every pass is
compared with the reference's level: new states, `generated`, per-action counts, distinct, fingerprint xor / sum, and blocked / permitted / blocked per
action of the deep info."""
import os
import subprocess
import sys

import numpy as np
import pytest

import action_constraint_reference as ar
import step_models_reference as smr
import step_reference as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
EXAMPLE = os.path.join(ROOT, "tools", "action_constraints_example.txt")
SIZES = dict(table_log2=20, frontier_words=1 << 22, frontier_states=1 << 17, pending_entries=1 << 17)
SMALL = dict(frontier_words=1 << 15, frontier_states=1 << 12)          # the buffers of test_action_constraint_gpu.py's out-of-room test
LOG_NEVER_SHRINKS_MODELS = "LogNeverShrinks == " + smr.LOG_NEVER_SHRINKS
# key -> (model, R, C, n, L, text of the constraint, Python predicate, level cap)
CASES = {
    "quiet-2122": ("first", 2, 1, 2, 2, ar.TEXTS["QuietClient"], ar.quiet_client, None),
    "quiet-3121": ("first", 3, 1, 2, 1, ar.TEXTS["QuietClient"], ar.quiet_client, 14),
    "commit-3111": ("first", 3, 1, 1, 1, ar.TEXTS["CommitNeverDecreases"], sr.commit_monotonic, None),
    "true-2122": ("first", 2, 1, 2, 2, ar.TEXTS["True"], ar.always, None),
    "false-2122": ("first", 2, 1, 2, 2, ar.TEXTS["False"], ar.never, None),
    "shrinks-second": ("second", 3, 0, 2, 1, LOG_NEVER_SHRINKS_MODELS, smr.log_never_shrinks, 11),
    "shrinks-third": ("third", 3, 0, 2, 1, LOG_NEVER_SHRINKS_MODELS, smr.log_never_shrinks, 11),
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
            which, R, C, n, L, _text, fn, cap = CASES[key]
            cache[key] = ar.constrained_bfs(which, R, C, n, L, fn, max_levels=cap)
        return cache[key]
    return get


def _model(vt, key):
    which, R, C, n, L = CASES[key][:5]
    if which == "first":
        return vt.Model.from_constants(R=R, C_=C, n=n, L=L)
    return (vt.Model.second_model if which == "second" else vt.Model.third_model)(R=R, n=n, L=L)


def _checker(vt, key, deep=True, **kw):
    m = _model(vt, key)
    mc = vt.ModelChecker(m, device=0, **dict(SIZES, **kw))
    w = m.compile_step_predicates(CASES[key][5])
    mc.action_constrain(w, deep=deep)
    return m, mc, w


def _act_counts(vt, d):
    return {vt.ACTION_NAMES[a]: int(n) for a, n in enumerate(d["act_generated"]) if n and a > 0}


def _check_deep_info(mc, lv, kind):
    """the deep info of the passes into lv.level against the reference's step into that level"""
    di = mc.action_constraint_deep_results(lv.level)
    assert (di["level"], di["kind"]) == (lv.level, kind), di
    assert (di["pairs"], di["blocked"], di["permitted"]) == (lv.generated, lv.blocked, lv.generated - lv.blocked), (lv.level, di)
    assert di["blocked_act"] == lv.blocked_act, (lv.level, di["blocked_act"], lv.blocked_act)
    assert (di["blocked_min_fp"] is None) == (lv.blocked == 0)
    assert di["launches"] >= di["slices"] >= 1 or lv.generated == 0
    return di


def _check_inserted(vt, mc, a, lv, distinct, kind):
    """one inserted level (its vsrmc_level_info as a dict) against the reference's; -> the row the variants of one space must agree on"""
    x, s = ar.xor_sum(lv.new)
    print("level %d (%s): new %d generated %d (reference %d %d), blocked %d" % (lv.level, kind, a["n_new"], a["generated"], len(lv.new), lv.generated, lv.blocked))
    assert (a["n_new"], a["generated"], a["distinct"]) == (len(lv.new), lv.generated, distinct), (lv.level, a["n_new"], a["generated"], a["distinct"], distinct)
    assert _act_counts(vt, a) == lv.act_generated, lv.level
    if lv.new:
        assert a["level"] == lv.level and (a["fp_xor"], a["fp_sum"]) == (x, s), lv.level
    assert a["viol_mask"] == 0
    di = _check_deep_info(mc, lv, kind)
    return (lv.level, a["n_new"], a["generated"], tuple(a["act_generated"]), di["blocked"], tuple(sorted(di["blocked_act"].items())), x, s)


def _deepen_to_the_end(vt, mc, ref, base, stop_at=None):
    """step() to `base`, then deepen() until nothing is inserted (or level stop_at is); every pass against the reference -> rows, and per pass (level
    inserted, its slices, its re-listings, the launches of the whole pass, the gated kernels' launches among them)"""
    by_level = {lv.level: lv for lv in ref.levels}
    for _ in range(base - 1):
        mc.step()
    assert mc.level == base and mc.distinct == sum(len(lv.new) for lv in ref.levels[:base])
    distinct, level, rows, shapes = mc.distinct, base, [], []
    while (level + 1) in by_level and (stop_at is None or level < stop_at):
        a, p = mc.deepen()
        lv = by_level[level + 1]
        distinct += len(lv.new)
        kind = "inserted-recordless" if level == base else "inserted"
        rows.append(_check_inserted(vt, mc, a, lv, distinct, kind))
        di = mc.action_constraint_deep_results(lv.level)
        own = di["launches"]                                                # the gated kernels' own launches: of the inserted level, and of the probed one
        if p is not None and lv.new:                                        # (an empty inserted level has no sub-slice to probe from: no gated pass, no row)
            own += mc.action_constraint_deep_results(p["level"])["launches"]
        shapes.append((lv.level, di["slices"], di["relisted"], a["pending"], own))
        if level == base:
            assert p is None                                                # pass 1 probes nothing
        if not lv.new:
            assert a["level"] == level
            break
        level += 1
        nxt = by_level.get(level + 1)
        if p is not None and nxt is not None:                               # the probed level: its parents are the level just inserted
            assert (p["level"], p["generated"], p["viol_mask"]) == (nxt.level, nxt.generated, 0), p
            assert _act_counts(vt, p) == nxt.act_generated
            _check_deep_info(mc, nxt, "probed")
    return rows, shapes


def _blocked_targets(key, ref, level):
    """{fingerprint of a blocked successor: set of parent fingerprints} of the step out of `level`, recomputed from the oracle and the Python predicate"""
    import vsr_tlaplus_amd as vt
    which, R, C, n, L, _text, pred = CASES[key][:7]
    orc, unpack, make_pm = ar.oracle_of(which)
    P, PM = ar.params_of(which, R, C, n, L), make_pm(R, C, n, L)
    out = {}
    for pfp, rec in ref.levels[level - 1].new.items():
        pv = unpack(PM, [int(x) for x in rec])
        for s in orc.successors(P, rec):
            if not pred(pv, unpack(PM, [int(x) for x in s["words"]]), vt.ACTION_NAMES[s["action"]]):
                out.setdefault(s["fp"], set()).add(pfp)
    return out


def _max_instances(key, ref, level):
    """the most enabled instances of one state of `level`"""
    which, R, C, n, L = CASES[key][:5]
    orc = ar.oracle_of(which)[0]
    P = ar.params_of(which, R, C, n, L)
    return max(len(orc.successors(P, rec)) for rec in ref.levels[level - 1].new.values())


def _never_entering(key, ref, level):
    everything = set()
    for lv in ref.levels:
        everything |= set(lv.new)
    return {fp: ps for fp, ps in _blocked_targets(key, ref, level).items() if fp not in everything}


def _seen(vt, mc, fps):
    import ctypes as C
    f = np.array(sorted(fps), dtype=np.uint64)
    out = np.zeros(max(1, len(f)), dtype=np.uint8)
    from vsr_tlaplus_amd import capi
    capi.check(vt.load().vsrmc_checker_seen_batch(mc._h, C.c_void_p(f.ctypes.data), len(f), 510, C.c_void_p(out.ctypes.data)))
    return out[: len(f)].astype(bool)


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


# ---------------------------------------------------------------------------------------------------------------------
# 1. equals the reference from several bases; 6. regeneration is exact; 8. traces into deep levels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [4, 9, 14, 20])
def test_equals_the_reference_from_several_bases(vt, refs, base):
    key = "quiet-2122"
    ref = refs(key)
    assert (ref.states, ref.depth, ref.blocked, ref.rescued) == (1510, 27, 95, 5)
    m, mc, w = _checker(vt, key)
    rows, shapes = _deepen_to_the_end(vt, mc, ref, base)
    assert [r[0] for r in rows] == list(range(base + 1, 29))               # every level to the empty 28th came through a gated pass
    assert (mc.depth, mc.distinct) == (27, 1510)
    # 6. every descent (every pass but the first) regenerated its nested levels through k_expand: the pass launched more kernels than the gated passes into
    #    the level it inserted and the level it probed did.  A descent into level L regenerates L - base - 1 levels; that the regenerated levels are the
    #    recorded ones shows in the level inserted on top (count, generated, xor, sum are the reference's), not in a count of their own.
    assert shapes[0][3] == shapes[0][4]                                     # the first pass: gated launches only
    assert all(launches > own for _lv, _s, _r, launches, own in shapes[1:]), shapes
    assert mc.seen_set_load()[0] == 1510                                   # no blocked-only target holds a slot
    # the rescued states of the deep levels are in the seen-set at exactly their level
    for lvl in (11, 15, 16):
        resc = ref.levels[lvl - 1].rescued
        assert resc
        for fp in resc:
            hit = mc.lookup(fp)
            assert hit is not None and (hit[1] >> 55) == lvl, (lvl, fp, hit)
    # the never-entering targets of the steps out of levels 10-16 are not in it
    n_never = 0
    for lvl in range(10, 17):
        never = _never_entering(key, ref, lvl)
        assert never, lvl
        n_never += len(never)
        assert not _seen(vt, mc, never).any(), lvl
    assert n_never == 40
    # 8. behaviours into states of deep levels, the rescued ones among them: permitted steps only
    picked = 0
    for lvl in sorted({base + 1, base + 2, 11, 15, 16, 22, 27}):
        if lvl <= base:
            continue
        lv = ref.levels[lvl - 1]
        for fp in (sorted(lv.rescued) + sorted(lv.new)[:3])[:4]:
            tr = mc.trace_fp(lvl, fp)
            assert len(tr) == lvl
            _check_trace(tr, key, fp)
            picked += 1
    assert picked >= 8
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the automatic scheme leaves the buffers by itself
# ---------------------------------------------------------------------------------------------------------------------
def test_the_automatic_scheme_leaves_the_buffers_by_itself(vt, refs):
    key = "quiet-3121"
    ref = refs(key)
    assert (ref.states, ref.blocked, ref.rescued) == (15111, 2806, 28) and all(lv.rescued for lv in ref.levels[2:14])
    by_level = {lv.level: lv for lv in ref.levels}
    m, mc, w = _checker(vt, key, **SMALL)
    kinds, distinct = [], 1
    while mc.depth < 14:
        assert mc.room() != 2
        n_rebased = len(mc.rebased)
        kind, d, p = mc.advance()
        assert kind != "stopped", mc.stopped                                # what = 4 never occurs
        # a pass that starts from a stored level (the first one, or the one after a re-basing) inserts without records; every other one is a descent
        recordless = not kinds or kinds[-1] != "deep" or len(mc.rebased) > n_rebased
        kinds.append(kind)
        lv = by_level[d["level"]]
        distinct += len(lv.new)
        if kind == "level":
            assert (d["n_new"], d["generated"], d["distinct"]) == (len(lv.new), lv.generated, distinct), d["level"]
            assert np.array_equal(mc.level_fps(), ar.new_fps(lv)) and mc.action_constraint_results(lv.level)["blocked"] == lv.blocked
        else:
            _check_inserted(vt, mc, d, lv, distinct, "inserted-recordless" if recordless else "inserted")
            if p is not None and (lv.level + 1) in by_level:
                nxt = by_level[lv.level + 1]
                assert (p["level"], p["generated"]) == (nxt.level, nxt.generated)
                _check_deep_info(mc, nxt, "probed")                         # the probed level's blocked figure
    assert kinds.count("deep") >= 3, kinds
    print(kinds, mc.rebased)
    assert (mc.depth, mc.distinct) == (14, 15111) and mc.seen_set_load()[0] == 15111
    mc.close()
    for how in ("run", "check"):
        m, mc, w = _checker(vt, key, **SMALL)
        assert (mc.run(max_depth=14) if how == "run" else mc.check(max_depth=14)) == "max-depth"
        assert (mc.depth, mc.distinct) == (14, 15111)
        mc.close()
    # without the opt-in the same sizes end the run as before
    m, mc, w = _checker(vt, key, deep=False, **SMALL)
    assert mc.run(max_depth=14) == "constraint-out-of-room" and "not constrained" in mc.stopped
    mc.close()


def test_an_overflowed_stored_level_is_adopted(vt, refs):
    """k_step_expand keeps claiming after the buffers ran out and counts every claim in n_new: the level is complete in the seen-set, and advance() adopts it"""
    key = "quiet-3121"
    ref = refs(key)
    by_level = {lv.level: lv for lv in ref.levels}
    m, mc, w = _checker(vt, key, **SMALL)
    distinct = 1
    with pytest.raises(vt.VsrmcError):
        while True:
            d = mc.step()
            distinct += d["n_new"]
    base = mc.level
    assert 5 <= base <= 12 and distinct == sum(len(lv.new) for lv in ref.levels[:base])
    kind, d, p = mc.advance()
    lv = by_level[base + 1]
    distinct += len(lv.new)
    assert kind == "deep" and p is None
    _check_inserted(vt, mc, d, lv, distinct, "inserted-recordless")
    assert mc.seen_set_load()[0] == distinct
    kind, d, p = mc.advance()                                              # and the search rolls on from it: a descent regenerates the adopted level
    lv = by_level[base + 2]
    distinct += len(lv.new)
    assert kind == "deep"
    _check_inserted(vt, mc, d, lv, distinct, "inserted")
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. slices: several per deep pass, lists that overflow and are listed again; identical figures
# ---------------------------------------------------------------------------------------------------------------------
def test_slices_give_identical_figures(vt, refs, monkeypatch):
    key = "quiet-2122"
    ref = refs(key)
    rows, shape = {}, {}
    for variant, env in (("default", {}), ("sliced", dict(VSRMC_ACTION_LIST_CAP="64", VSRMC_ACTION_SLICE="64"))):
        for k in ("VSRMC_ACTION_SLICE", "VSRMC_ACTION_LIST_CAP"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m, mc, w = _checker(vt, key)
        rows[variant], shape[variant] = _deepen_to_the_end(vt, mc, ref, 9)
        mc.close()
    assert rows["sliced"] == rows["default"] and len(rows["default"]) == 19   # levels 10 .. 28, the empty one included
    # What the reference says about slices (a slice holds at most 64 INDICES of its source, holes included, and the list 64 entries, the knob's floor):
    #  - every pass into level L lists its parents in at least ceil(parents / 64) slices;
    #  - a slice MUST overflow, and be listed again in halves, where 64 parents cannot have fewer than 65 instances.  That is provable for the first pass
    #    only: its source is the dense stored base, so its first slice holds min(64, parents) parents, and these have at least generated - max(0, parents - 64) *
    #    (the most instances of one parent) instances.  A descent's parents arrive in regenerated sub-slices whose composition the reference does not know (on the MI355X levels
    #    11 - 17 re-listed as well; from level 18 on a pass sees a few records at a time: 128 listings for 110 parents), and the last levels have 3 - 48
    #    parents: no list of 64 can overflow there.  The figures are compared on every level.
    by_level = {lv.level: lv for lv in ref.levels}
    print("sliced (level, slices, relisted, launches, gated launches):", shape["sliced"])
    for lvl, slices, relisted, _launches, _own in shape["sliced"]:
        parents = len(by_level[lvl - 1].new)
        assert slices >= -(-parents // 64), (lvl, slices, parents)
    lv10, parents9 = by_level[10], len(by_level[9].new)
    most = _max_instances(key, ref, 9)
    assert lv10.generated - max(0, parents9 - 64) * most > 64, (parents9, lv10.generated, most)   # the first slice of pass 1 (63 parents, 116 instances) must overflow
    assert shape["sliced"][0][0] == 10 and shape["sliced"][0][2] >= 1 and shape["sliced"][0][1] >= 3, shape["sliced"][0]
    assert sum(r[2] for r in shape["sliced"]) > shape["sliced"][0][2]        # and descents re-listed too
    assert all(r[2] == 0 for r in shape["default"])


# ---------------------------------------------------------------------------------------------------------------------
# 4. re-basing: the levels shrink again, the newest seen-set-only level becomes the stored base
# ---------------------------------------------------------------------------------------------------------------------
def test_rebasing(vt, refs):
    key = "commit-3111"
    ref = refs(key)
    assert (ref.states, ref.depth, ref.blocked) == (42301, 24, 1640) and next(lv.level for lv in ref.levels if lv.blocked) == 13
    by_level = {lv.level: lv for lv in ref.levels}
    m, mc, w = _checker(vt, key, frontier_states=1 << 12)
    for _ in range(11):
        mc.step()
    assert mc.level == 12
    distinct, kinds, n_deep = mc.distinct, [], 0
    while True:
        assert mc.room() != 2
        n_rebased = len(mc.rebased)
        kind, d, p = mc.advance()
        assert kind != "stopped", mc.stopped
        recordless = not kinds or kinds[-1] != "deep" or len(mc.rebased) > n_rebased
        kinds.append(kind)
        lvl = d["level"] + (0 if d["n_new"] else 1)
        lv = by_level[lvl]
        distinct += len(lv.new)
        if len(mc.rebased) > n_rebased:
            rb = mc.rebased[-1]
            assert rb["n"] == len(by_level[rb["level"]].new), rb
        if kind == "level":
            assert (d["n_new"], d["generated"], d["distinct"]) == (len(lv.new), lv.generated, distinct), lvl
            assert mc.action_constraint_results(0)["blocked"] == lv.blocked
            if lv.new:
                assert np.array_equal(mc.level_fps(), ar.new_fps(lv)), lvl
        else:
            n_deep += 1
            _check_inserted(vt, mc, d, lv, distinct, "inserted-recordless" if recordless else "inserted")
        if d["n_new"] == 0:
            break
    assert len(mc.rebased) >= 1 and n_deep >= 3 and "level" in kinds[kinds.index("deep"):], (kinds, mc.rebased)   # stored levels again after a re-basing
    assert (mc.depth, mc.distinct) == (24, 42301) and mc.seen_set_load()[0] == 42301
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. True and False
# ---------------------------------------------------------------------------------------------------------------------
def test_true_equals_the_unconstrained_deep_run(vt, refs):
    m, mc, w = _checker(vt, "true-2122")
    plain = vt.ModelChecker(m, device=0, **SIZES)
    for _ in range(8):
        mc.step()
        plain.step()
    n = 0
    while True:
        (a, p), (b, q) = mc.deepen(), plain.deepen()
        for k in ("level", "n_new", "generated", "distinct", "fp_xor", "fp_sum", "max_bag", "act_generated", "viol_mask"):
            assert a[k] == b[k], (k, a[k], b[k])
        assert (p is None) == (q is None)
        if p is not None:
            assert (p["level"], p["generated"], p["viol_mask"]) == (q["level"], q["generated"], q["viol_mask"])
        if a["n_new"] == 0:
            break
        n += 1
        assert mc.action_constraint_deep_results(a["level"])["blocked"] == 0
    assert n >= 10 and mc.distinct == plain.distinct == refs("true-2122").states


def test_false_blocks_everything_at_the_base(vt, refs):
    m = _model(vt, "false-2122")
    plainref = refs("true-2122")
    mc = vt.ModelChecker(m, device=0, **SIZES)
    mc.action_constrain(m.compile_step_predicates(ar.TEXTS["False"]), deep=True)
    a, p = mc.deepen()                                                     # attached at the base (Init: an action constraint is attached at level 1 only)
    gen = plainref.levels[1].generated
    di = mc.action_constraint_deep_results(2)
    assert (a["n_new"], a["generated"], a["level"], a["distinct"]) == (0, gen, 1, 1) and p is None
    assert (di["blocked"], di["pairs"], di["permitted"], di["kind"]) == (gen, gen, 0, "inserted-recordless")
    assert mc.depth == 1 and mc.seen_set_load()[0] == 1
    mc.reset()
    assert mc.run() == "exhausted" and (mc.depth, mc.distinct) == (1, 1)


# ---------------------------------------------------------------------------------------------------------------------
# 7. violations (the hooks library, a child process)
# ---------------------------------------------------------------------------------------------------------------------
def test_forced_violations_in_a_child(vt):
    hooks = os.path.join(ROOT, "vsr_tlaplus_amd", "libvsrmc_hooks.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "deep_action_worker.py")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, VSRMC_LIB=hooks))
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------------
# 9. the analysis models through the deep path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["shrinks-second", "shrinks-third"])
def test_analysis_models(vt, refs, key):
    ref = refs(key)
    assert ref.blocked >= 20 and ref.states >= 10000 and sum(lv.blocked for lv in ref.levels[6:]) == ref.blocked
    m, mc, w = _checker(vt, key, frontier_words=1 << 24, frontier_states=1 << 18)
    rows, shapes = _deepen_to_the_end(vt, mc, ref, 6)
    assert [r[0] for r in rows] == [7, 8, 9, 10, 11] and all(launches > own for _lv, _s, _r, launches, own in shapes[1:])
    assert mc.seen_set_load()[0] == mc.distinct == ref.states
    mc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. five replicas: the harvest sample of (5,1,2,1) as level 1, TailUnchanged alone, level 2 record-less, level 3 by a descent (a child on the hooks library)
# ---------------------------------------------------------------------------------------------------------------------
def test_five_replicas_seeded(tmp_path):
    """The reference (tests/constrained_seeded_reference.py, imported by the worker) takes 6 s for the harvest and 29 s for the two steps on the CPU and
    blocks 3 969 and 7 291 transitions: the issue's condition for building the case holds.  Every figure is the reference's."""
    import json
    import constrained_seeded_reference as cs
    hooks = os.path.join(ROOT, "vsr_tlaplus_amd", "libvsrmc_hooks.so")
    out = os.path.join(str(tmp_path), "deep_action_seeded.json")
    env = {k: v for k, v in os.environ.items() if k not in ("VSRMC_ACTION_SLICE", "VSRMC_ACTION_LIST_CAP")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "deep_action_seeded_worker.py"), out], capture_output=True, text=True, timeout=300,
                       env=dict(env, VSRMC_LIB=hooks))
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    with open(out) as f:
        res = json.load(f)
    want = cs.MEASURED[(5, 1, 2, 1)]["level2"]                             # the step out of the seeds does not depend on the state constraint of case (c)
    assert res["seeds"] == 1500 and [row["level"] for row in res["rows"]] == [2, 3, 4]
    assert (res["level2"]["generated"], res["level2"]["blocked"], res["level2"]["new"]) == (want["generated"], want["blocked"], want["new"])
    assert res["rows"][0]["blocked"] == want["blocked"] and res["rows"][1]["blocked"] == res["level3"]["blocked"] > 0 and res["rows"][2]["blocked"] > 0
    print("child: %.1f s, of them %.1f s the reference, %.1f s with the device" % (res["seconds"], res["reference_seconds"], res["device_seconds"]))


# ---------------------------------------------------------------------------------------------------------------------
# 11. refusals, detach, reset; the CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_detach_and_reset(vt, refs, tmp_path):
    import ctypes as C
    import constraint_reference as cr
    from vsr_tlaplus_amd import capi
    lib = vt.load()
    m = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
    w = m.compile_step_predicates(ar.TEXTS["QuietClient"])
    con = m.compile_predicates(cr.TEXTS["True"])

    def refused(f, code, needle):
        with pytest.raises(vt.VsrmcError) as e:
            f()
        assert e.value.code == code and needle in e.value.message, (e.value.code, e.value.message)

    mc = vt.ModelChecker(m, device=0, **SIZES)
    assert lib.vsrmc_checker_action_constrain_deep(mc._h, 1) == -6 and "no action constraint attached" in lib.vsrmc_last_error().decode()
    # beside a state constraint, plain or deep, either order
    mc.constrain(con)
    refused(lambda: mc.action_constrain(w, deep=True), -6, "cannot judge states")
    assert mc._action_constraint is None
    mc.constrain(None)
    mc.constrain(con, deep=True)
    refused(lambda: mc.action_constrain(w, deep=True), -6, "vsrmc_checker_constrain_deep")
    mc.constrain(None)
    mc.action_constrain(w, deep=True)
    refused(lambda: mc.constrain(con), -6, "cannot judge states")
    refused(lambda: mc.constrain(con, deep=True), -6, "cannot judge states")
    # the attachments for the levels beyond the buffers, the other probes, checkpoints
    refused(lambda: mc.deep_attach(m.compile_predicates(cr.TEXTS["True"]), None), -6, "gate")
    refused(mc.deep_terminal_attach, -6, "gate")
    mc.step()
    assert lib.vsrmc_checker_action_constrain_deep(mc._h, 1) == -6 and "at level 1 only" in lib.vsrmc_last_error().decode()
    for name in ("vsrmc_checker_probe2", "vsrmc_checker_probe3"):
        infos = [capi.LevelInfo() for _ in range(3)]
        rc = getattr(lib, name)(mc._h, *[C.byref(i) for i in infos[: 2 if name.endswith("2") else 3]])
        assert rc == -6 and "does not gate" in lib.vsrmc_last_error().decode(), name
    refused(lambda: mc.save(str(tmp_path / "chk")), -6, "does not name it")
    # exact_ties and sharded checkers refuse the attachment itself
    mc4 = vt.ModelChecker(m, device=0, exact_ties=True, **SIZES)
    refused(lambda: mc4.action_constrain(w, deep=True), -6, "exact_ties")
    # reset keeps the attachment and the opt-in; detach gives the plain checker back
    ref = refs("quiet-2122")
    mc.reset()
    for _ in range(3):
        mc.step()
    a, p = mc.deepen()
    assert (a["level"], a["n_new"]) == (5, len(ref.levels[4].new))
    mc.reset()
    assert (mc.level, mc.distinct) == (1, 1)
    a, p = mc.deepen()
    assert (a["level"], a["n_new"]) == (2, len(ref.levels[1].new))
    mc.action_constrain(None)
    plain = refs("true-2122")
    mc.step()
    a, p = mc.deepen()
    assert (a["level"], a["n_new"], a["generated"]) == (3, len(plain.levels[2].new), plain.levels[2].generated)
    with pytest.raises(ValueError):
        mc.action_constraint_deep_results()
    # without the opt-in nothing changed
    mc2 = vt.ModelChecker(m, device=0, **SIZES)
    mc2.action_constrain(w)
    mc2.step()
    refused(mc2.deepen, -6, "not constrained")
    refused(mc2.probe, -6, "not constrained")
    refused(lambda: mc2.action_constraint_deep_results(3), -6, "vsrmc_checker_action_constrain_deep")


def test_probe_of_a_stored_checker(vt, refs):
    """probe(): the next level's candidates are the successors of permitted transitions; its deep info carries the blocked figure"""
    key = "quiet-2122"
    ref = refs(key)
    m, mc, w = _checker(vt, key)
    for _ in range(11):
        mc.step()
    p = mc.probe()
    nxt = ref.levels[12]
    assert (p["level"], p["generated"], p["viol_mask"]) == (13, nxt.generated, 0) and nxt.blocked > 0
    _check_deep_info(mc, nxt, "probed")
    assert mc.seen_set_load()[0] == mc.distinct                            # nothing was inserted


def _run_cli(args):
    return subprocess.run([CLI] + args + ["-noTLA", "-tableLog2", "18"], capture_output=True, text=True, timeout=300)


def test_cli_lines_totals_and_dumped_trace(vt, refs, tmp_path):
    from test_host_cpu import _cfg
    ref = refs("quiet-3121")
    cfg = _cfg(tmp_path, R=3, vals="v1, v2", L=1)
    args = ["-config", cfg, "-steps", EXAMPLE, "-actionConstraint", "QuietClient", "-deepActionConstraint", "-frontierGiB", "0.0005", "-maxDepth", "14"]
    r = _run_cli(args)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr)
    lines = r.stdout.splitlines()
    virt = [ln for ln in lines if ln.startswith("Virtual(")]
    prob = [ln for ln in lines if ln.startswith("Probe(")]
    stored = [ln for ln in lines if ln.startswith("ActionConstraint(")]
    assert len(virt) >= 3 and prob and stored, r.stdout[-3000:]
    by_level = {lv.level: lv for lv in ref.levels}
    for ln in virt:
        lv = by_level[int(ln[len("Virtual("):ln.index(")")])]
        assert ("%d states in the level" % len(lv.new)) in ln and ("; %d of %d transitions were not taken." % (lv.blocked, lv.generated)) in ln, ln
    for ln in prob:
        lvl = int(ln[len("Probe("):ln.index(")")])
        if lvl in by_level:
            assert ("%d of them by transitions not taken" % by_level[lvl].blocked) in ln, ln
    total = {}
    for lv in ref.levels:
        for a, n in lv.blocked_act.items():
            total[a] = total.get(a, 0) + n
    per = ", ".join("%s: %d" % (a, total[a]) for a in vt.ACTION_NAMES if a in total)
    assert ("ACTION_CONSTRAINT QuietClient: %d transitions were not taken (per action: %s)" % (ref.blocked, per)) in r.stdout, r.stdout[-1500:]
    assert ("%d distinct states found" % ref.states) in r.stdout
    # without the flag the run ends where the buffers do, as before
    r0 = _run_cli([a for a in args if a != "-deepActionConstraint"])
    assert r0.returncode == 4 and "not constrained" in r0.stdout and not any(ln.startswith("Virtual(") for ln in r0.stdout.splitlines())


def test_cli_dumped_trace_validates_with_the_opt_in_on(vt, refs, tmp_path):
    """-dumpTrace of a CLI run with -deepActionConstraint validates with -validateTrace.  The violator is a state of a STORED level: the CLI has no way to a
    violator beyond the buffers on these spaces (no reachable state of them fails a built-in invariant, -invariant NAME is examined on stored levels, and
    -deepPredicates is refused beside the flag).  The behaviours beyond the buffers, and their routing through the permitted-steps trace, are checked step by
    step with the Python predicate in test_equals_the_reference_from_several_bases and, for violators of an inserted and of a probed level, in
    deep_action_worker.py; this test pins that the flag leaves the stored path's report and dump as they were."""
    from test_host_cpu import _cfg
    cfg = _cfg(tmp_path, R=2, vals="v1, v2", L=2)
    preds = tmp_path / "preds.txt"
    preds.write_text(r"NothingCommitted == ~(\E r \in replicas : rep_commit_number[r] >= 1)" + "\n")
    out = str(tmp_path / "trace.tla")
    r = _run_cli(["-config", cfg, "-steps", EXAMPLE, "-actionConstraint", "QuietClient", "-deepActionConstraint", "-predicates", str(preds), "-invariant", "NothingCommitted",
                  "-dumpTrace", "tla", out, "-frontierGiB", "0.05"])
    assert r.returncode == 12 and "Error: Invariant NothingCommitted is violated." in r.stdout, r.stdout[-3000:] + r.stderr
    v = _run_cli(["-config", cfg, "-validateTrace", out])
    assert v.returncode == 0 and "The trace is a behaviour of the model." in v.stdout, v.stdout + v.stderr


def test_cli_flag_needs_the_action_constraint(vt, tmp_path):
    from test_host_cpu import _cfg
    cfg = _cfg(tmp_path, R=2, vals="v1, v2", L=2)
    r = _run_cli(["-config", cfg, "-deepActionConstraint"])
    assert r.returncode == 2 and "-deepActionConstraint needs -actionConstraint NAME" in r.stderr
