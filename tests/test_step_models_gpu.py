"""Step predicates on the two analysis models on the GPU (`-m gpu`): k_step_list<1|2> / k_step_apply<1|2> through Model.step_flags,
ModelChecker.step_scan / step_pairs / run(step_never=, step_reach=) / step_witness_trace and the CLI, against hand-written Python functions
f(parent, child, action) over pyoracle2 / pyoracle3's unpack of the CPU oracles' records and successors (tests/step_models_reference.py — the reference is
never the parser).  Every figure is recomputed from the oracle here.

Spaces: "222" = (2 replicas, 2 values, limit 2), exhausted; "321" = (3, 2, 1), parents of levels 1-12.  The Python reference walks every pair of "222" and of
levels 1-10 of "321" once per model (module-scoped, shared, never changed); of levels 11-12 it walks the directed subset of test 2, and every pair of level
12 once with one function, to find the steps on which a commit number decreases."""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import step_models_reference as sm
import where_models_reference as wm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
# (R, values, limit, levels walked (None = exhausted), levels walked pair by pair)
SPACES = {"321": (3, 2, 1, 12, 10), "222": (2, 2, 2, None, None)}
SIZES = dict(table_log2=20, frontier_words=1 << 22, frontier_states=1 << 17, pending_entries=1 << 17)
RUN_SIZES = dict(table_log2=20, frontier_words=1 << 24, frontier_states=1 << 20, pending_entries=1 << 19)
Level = collections.namedtuple("Level", "level words off recs states fps")
# per-level pair counts of "321" as the issue gives them; recomputed below
PAIRS_321 = {"second": [4, 18, 64, 207, 632, 1710, 4056, 8590, 16586, 29864], "third": [4, 18, 64, 207, 619, 1625, 3736, 7677, 14449, 25410]}


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


def _norm(fixed, r):
    return tuple(int(x) for x in r[:fixed]) + tuple(sorted(int(x) for x in r[fixed:]))


class Space:
    """one model's oracle BFS of one space: the levels, and per parent its oracle successors as (action name, normalised child record, child's Python
    view), computed when first asked for and kept"""

    def __init__(self, vt, which, key):
        self.orc, self.po = _oracle(which)
        R, n, L, depth, _ = SPACES[key]
        self.values = _values(which, n)
        self.P = self.orc.Params(R, n, L)
        self.PM = self.po.Model(R, self.values, L)
        self.fixed = self.P.fixed_words()
        self.actions = vt.ACTION_NAMES
        self.levels, self.generated = [], []
        self._succ, self._views, self._bits = {}, {}, {}
        b = self.orc.Bfs(self.P)
        level = 1
        init = self.orc.init_record(self.P)
        words, off = init, np.array([0, len(init)], dtype=np.uint64)
        while True:
            recs = [words[int(off[i]): int(off[i + 1])] for i in range(len(off) - 1)]
            self.levels.append(Level(level, words, off, recs, [self.po.unpack(self.PM, [int(x) for x in r]) for r in recs],
                                     [self.orc.fingerprint(self.P, r)[0] for r in recs]))
            n_new = b.step()
            self.generated.append(b.info["generated"])              # of the step that expands this level
            if (depth is not None and level >= depth) or n_new == 0:
                break
            level += 1
            words, off = b.frontier()
        b.close()

    def view(self, norm):
        if norm not in self._views:
            self._views[norm] = self.po.unpack(self.PM, list(norm))
        return self._views[norm]

    def succ(self, lv, i):
        if (lv.level, i) not in self._succ:
            row = []
            for s in self.orc.successors(self.P, lv.recs[i]):
                cn = _norm(self.fixed, s["words"])
                row.append((self.actions[s["action"]], cn, self.view(cn)))
            self._succ[(lv.level, i)] = row
        return self._succ[(lv.level, i)]

    def bits(self, tag, preds, lv, i):
        """the reference's verdicts on the pairs out of parent i: [bits], in the order of succ()"""
        if (tag, lv.level, i) not in self._bits:
            self._bits[(tag, lv.level, i)] = [sm.bits_of(preds, lv.states[i], c, a) for a, _cn, c in self.succ(lv, i)]
        return self._bits[(tag, lv.level, i)]


@pytest.fixture(scope="module")
def spaces(vt):
    cache = {}

    def get(which, key):
        if (which, key) not in cache:
            cache[(which, key)] = Space(vt, which, key)
        return cache[(which, key)]
    return get


def _model(vt, which, key):
    R, n, L = SPACES[key][:3]
    return (vt.Model.second_model if which == "second" else vt.Model.third_model)(R=R, n=n, L=L)


def _pairwise_levels(sp, key, upto=None):
    upto = upto or SPACES[key][4]
    return [lv for lv in sp.levels if upto is None or lv.level <= upto]


def _check_parents(vt, m, sp, w, tag, preds, lv, idx):
    """step_flags on the parents idx of one level against the reference: the rows are those of get_next_states (parent, ordinal, action, error) and
    per parent the same multiset of (child, action, bits)"""
    words = np.concatenate([lv.recs[i] for i in idx])
    off = np.cumsum([0] + [len(lv.recs[i]) for i in idx]).astype(np.uint64)
    n_succ = sum(len(sp.succ(lv, i)) for i in idx)
    nx = m.get_next_states(words, off, cap_succ=n_succ + 64)
    rows = m.step_flags(w, words, off)
    assert len(nx) == n_succ and rows.shape == (n_succ, 5), (tag, lv.level)
    got = [collections.Counter() for _ in idx]
    for row, s in zip(rows, nx):
        assert (int(row[0]), int(row[1]), int(row[2]), int(row[4])) == (s["parent"], s["ordinal"], s["action"], s["err"]) and s["err"] == 0, (tag, lv.level)
        got[s["parent"]][(_norm(sp.fixed, s["words"]), vt.ACTION_NAMES[s["action"]], int(row[3]))] += 1
    for k, i in enumerate(idx):
        want = collections.Counter((cn, a, b) for (a, cn, _c), b in zip(sp.succ(lv, i), sp.bits(tag, preds, lv, i)))
        assert got[k] == want, (tag, lv.level, i)
    return n_succ


# ---------------------------------------------------------------------------------------------------------------------
# 1. pair by pair
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sm.MODELS)
def test_step_flags_pair_by_pair(vt, spaces, which):
    for key in ("222", "321"):
        sp = spaces(which, key)
        m = _model(vt, which, key)
        levels = _pairwise_levels(sp, key)
        per_level = []
        for tag, preds in sm.sets(which):
            w = m.compile_step_predicates(sm.text_of(preds))
            assert w.names == [p[0] for p in preds] and w.step
            per_level = [_check_parents(vt, m, sp, w, tag, preds, lv, list(range(len(lv.recs)))) for lv in levels]
        print("step_flags %s model, %s: %d pairs out of %d levels" % (which, key, sum(per_level), len(levels)))
        if key == "321":
            assert per_level == PAIRS_321[which] and sum(per_level) == {"second": 61731, "third": 53809}[which]
        else:
            assert len(levels) == 27 and sum(len(lv.recs) for lv in levels) == 14735 and sum(per_level) == 20305
        assert per_level == sp.generated[: len(per_level)]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the directed subset of levels 11-12 of "321"
# ---------------------------------------------------------------------------------------------------------------------
def _directed(sp):
    """(level, [parent indices]) for levels 11 and 12: the parents with a replica in StateTransfer or a GetStateMsg / NewStateMsg in the bag (selected
    with the state-predicate reference), and the parents of the level-12 pairs on which a commit number decreases (found with the step reference).
    A replica enters StateTransfer out of a state that has neither, and on these spaces that selection holds no parent of a SendGetState step; the
    subset must hold one, so the level-12 parents out of which the oracle takes a SendGetState step are added."""
    from oracle import pyoracle2 as p2
    out = []
    lowering = []
    for lv in sp.levels[10:12]:
        pick = set(i for i, s in enumerate(lv.states)
                   if wm.in_state_transfer(s) or any(m["type"] in (p2.GetStateMsg, p2.NewStateMsg) for m, _ in wm.msgs(s)))
        if lv.level == 12:
            for i, s in enumerate(lv.states):
                for a, _cn, c in sp.succ(lv, i):
                    if not sm.commit_monotonic(s, c, a):
                        lowering.append((i, a))
                        pick.add(i)
                    if a == "SendGetState":                         # (see the docstring: the selection above holds no parent of such a step)
                        pick.add(i)
        out.append((lv, sorted(pick)))
    return out, lowering


@pytest.fixture(scope="module")
def directed(spaces):
    cache = {}

    def get(which):
        if which not in cache:
            cache[which] = _directed(spaces(which, "321"))
        return cache[which]
    return get


@pytest.mark.parametrize("which", sm.MODELS)
def test_directed_subset_of_levels_11_and_12(vt, spaces, directed, which):
    sp = spaces(which, "321")
    m = _model(vt, which, "321")
    subset, lowering = directed(which)
    # the figures of the issue: the commit number decreases on four pairs of VR_STATE_TRANSFER.tla, all ReceiveSV out of level 12, on none of VR_APP_STATE.tla
    assert [a for _i, a in lowering] == (["ReceiveSV"] * 4 if which == "second" else []), lowering
    actions = collections.Counter(a for lv, idx in subset for i in idx for a, _cn, _c in sp.succ(lv, i))
    print("directed subset, %s model: %s parents, actions %s" % (which, [len(idx) for _lv, idx in subset], dict(actions)))
    assert actions["SendGetState"] >= 1 and actions["ReceiveGetState"] >= 1 and actions["ReceiveNewState"] >= 1    # from the oracle alone
    for tag, preds in sm.sets(which):
        w = m.compile_step_predicates(sm.text_of(preds))
        for lv, idx in subset:
            _check_parents(vt, m, sp, w, tag, preds, lv, idx)


# ---------------------------------------------------------------------------------------------------------------------
# 3. both verdicts, over the pairs of tests 1 and 2 together: the reference alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sm.MODELS)
def test_both_verdicts(spaces, directed, which):
    seen = collections.defaultdict(set)
    false_on = collections.Counter()
    by_action = collections.defaultdict(collections.Counter)
    walked = []
    for key in ("222", "321"):
        sp = spaces(which, key)
        walked += [(sp, lv, range(len(lv.recs))) for lv in _pairwise_levels(sp, key)]
    sp = spaces(which, "321")
    walked += [(sp, lv, idx) for lv, idx in directed(which)[0]]
    for sp, lv, idx in walked:
        for tag, preds in sm.sets(which):
            for i in idx:
                for (a, _cn, _c), bits in zip(sp.succ(lv, i), sp.bits(tag, preds, lv, i)):
                    for k, p in enumerate(preds):
                        v = (bits >> k) & 1
                        seen[(tag, p[0])].add(v)
                        if not v:
                            false_on[(tag, p[0])] += 1
                        elif p[0] in ("EntersStateTransfer", "LeavesStateTransfer", "NewStateAppears", "HeldDvcsDropped") and tag in ("A",):
                            by_action[p[0]][a] += 1
    print("both verdicts, %s model: false on %s; true by action %s" % (which, dict(false_on), {k: dict(v) for k, v in by_action.items()}))
    for p in sm.SET_A[which]:
        assert seen[("A", p[0])] == {0, 1}, p[0]
    assert sum(1 for p in sm.SET_B if seen[("B", p[0])] == {0, 1}) >= 7
    # the properties that hold throughout, pair by pair in sets without that condition
    assert false_on[("C", "CommittedPrefixStable")] == 0 and false_on[("C", "ViewMonotonic")] == 0
    if which == "third":
        assert false_on[("T", "AppPrefixStable")] == 0 and false_on[("C", "CommitMonotonic")] == 0
    # which actions do it (the issue's list): a replica enters StateTransfer by SendGetState only, a NewStateMsg key appears by ReceiveGetState only
    assert set(by_action["EntersStateTransfer"]) == {"SendGetState"} and set(by_action["NewStateAppears"]) == {"ReceiveGetState"}
    assert set(by_action["LeavesStateTransfer"]) <= {"ReceiveHigherSVC", "ReceiveSV", "ReceiveNewState"}


# ---------------------------------------------------------------------------------------------------------------------
# 4. the neighbour word: primed variables of replica r + 1 on steps taken by r (a block of these models is one or two words)
# 5. the primed bag
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sm.MODELS)
def test_neighbour_word_and_primed_bag(vt, spaces, which):
    bag = [p for p in sm.SET_A["second"] if p[0] in ("NewDvcShorterThanCommit", "CountGoesDown", "NewStateAppears")]
    assert len(bag) == 3
    acted = collections.Counter()
    seen = collections.defaultdict(set)
    for key in ("222", "321"):
        sp = spaces(which, key)
        R = SPACES[key][0]
        m = _model(vt, which, key)
        for tag, preds in (("N", sm.neighbour(which)), ("P", bag)):
            w = m.compile_step_predicates(sm.text_of(preds))
            for lv in _pairwise_levels(sp, key, 8 if key == "321" else None):
                _check_parents(vt, m, sp, w, tag, preds, lv, list(range(len(lv.recs))))
                for i in range(len(lv.recs)):
                    for (a, _cn, c), bits in zip(sp.succ(lv, i), sp.bits(tag, preds, lv, i)):
                        for k, p in enumerate(preds):
                            seen[p[0]].add((bits >> k) & 1)
                        if tag == "N":
                            for r in sm.actor(lv.states[i], c):
                                acted[(a, r < R)] += 1                 # r < R: the word after r's block is replica r + 1's; r = R: replica 1 is read far away
    print("neighbour word, %s model: acting replicas %s" % (which, dict(acted)))
    # condition, from the reference alone: every predicate reads every replica's primed variables, so a pair whose acting replica is r < R reads a
    # variable of r + 1 beside the rewritten block — for the actions the predicates name and for the others
    for a in ("SendDVC", "TimerSendSVC", "ReceivePrepareOkMsg", "ReceiveSV") + (("ExecuteOp", "ReceiveMatchingDVC") if which == "third" else ()):
        assert acted[(a, True)] >= 1 and acted[(a, False)] >= 1, a
    assert seen["OneViewRaised"] == {0, 1} and seen["PeersKept"] == {0, 1}
    if which == "third":
        assert seen["OneHeldChanged"] == {0, 1} and seen["OthersAppKept"] == {0, 1}
    assert seen["NewDvcShorterThanCommit"] == {0, 1} and seen["CountGoesDown"] == {0, 1}     # an appended entry's log; a patched entry's count


# ---------------------------------------------------------------------------------------------------------------------
# 6. the level scan inside a search
# ---------------------------------------------------------------------------------------------------------------------
def _strip(t):
    return {k: v for k, v in t.items() if not k.endswith("_ms") and k != "slices"}


def _worker(which, key, depth, **env):
    R, n, L = SPACES[key][:3]
    e = dict(os.environ)
    e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "step_models_scan_worker.py"), which] + [str(x) for x in (R, n, L, depth or 0)], env=e,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("STEP_SCAN "))[len("STEP_SCAN "):])


@pytest.mark.parametrize("which", sm.MODELS)
@pytest.mark.parametrize("key", ["222", "321"])
def test_step_scan_inside_a_search(vt, spaces, which, key):
    sp = spaces(which, key)
    m = _model(vt, which, key)
    preds = sm.SET_A[which]
    w = m.compile_step_predicates(sm.text_of(preds))
    mc = vt.ModelChecker(m, **SIZES)
    ob = sp.orc.Bfs(sp.P)
    levels = _pairwise_levels(sp, key)
    mine = []
    for lv in levels:
        t = mc.step_scan(w)
        assert _strip(t) == _strip(mc.step_scan(w))                  # any number of times, nothing changes
        assert (t["level"], t["n_states"], t["n_err"]) == (lv.level, len(lv.recs), 0)
        count = [0] * 8
        hits = [[] for _ in range(8)]                               # per predicate: (parent fingerprint, action) of the pairs that satisfy it
        pairs = collections.Counter()
        for i in range(len(lv.recs)):
            for (a, _cn, _c), bits in zip(sp.succ(lv, i), sp.bits("A", preds, lv, i)):
                if bits:
                    pairs[(int(lv.fps[i]), bits)] += 1
                for k in range(8):
                    if (bits >> k) & 1:
                        count[k] += 1
                        hits[k].append((int(lv.fps[i]), a))
        n_pairs = sum(len(sp.succ(lv, i)) for i in range(len(lv.recs)))
        assert t["n_pairs"] == n_pairs == sp.generated[lv.level - 1] and t["count"] == count, lv.level
        fps, _ords, bits = mc.step_pairs()
        assert collections.Counter((int(a), int(b)) for a, b in zip(fps, bits)) == pairs, lv.level
        for k in range(8):
            if hits[k]:
                fp = min(x[0] for x in hits[k])
                assert t["min_fp"][k] == fp and mc.find_fp(fp) == t["min_index"][k], (lv.level, k)
                assert vt.ACTION_NAMES[t["min_action"][k]] in set(a for f, a in hits[k] if f == fp), (lv.level, k)   # the witness's action
            else:
                assert t["min_fp"][k] is None and t["min_ordinal"][k] is None and t["min_action"][k] is None
        assert np.array_equal(mc.level_fps(), ob.level_fps(lv.level))   # the scan left the level as it was
        mine.append(_strip(t))
        d = mc.step()
        nn = ob.step()
        assert d["n_new"] == nn and d["generated"] == ob.info["generated"] == t["n_pairs"], lv.level
    mc.close()
    ob.close()
    # ... and in processes of their own under other slice sizes: identical in every figure that does not depend on how a level stores a record (the
    # witness's action is that of the parent's smallest ordinal with the bit, and an ordinal names a position in the bag as that process stored it)
    def invariant(row):
        return {k: row[k] for k in ("level", "n_states", "n_pairs", "n_err", "count", "min_fp")}
    for slice_ in (1, 7):
        other = _worker(which, key, len(levels), VSRMC_STEP_SLICE=slice_)
        assert len(other) == len(mine)
        for a, b in zip(mine, other):
            assert b["slices"] >= -(-a["n_states"] // slice_)
            assert invariant(a) == invariant(b), (slice_, a["level"])


# ---------------------------------------------------------------------------------------------------------------------
# 7. run(step_never=..) and the CLI
# ---------------------------------------------------------------------------------------------------------------------
def _first_level(sp, fn, upto):
    """the first level with a pair on which fn is false, its smallest parent fingerprint among them and the actions of that parent's such pairs"""
    for lv in sp.levels[:upto]:
        bad = [(int(lv.fps[i]), a) for i in range(len(lv.recs)) for a, _cn, c in sp.succ(lv, i) if not fn(lv.states[i], c, a)]
        if bad:
            fp = min(x[0] for x in bad)
            return lv, fp, set(a for f, a in bad if f == fp), len(bad)
    return None, None, set(), 0


@pytest.mark.parametrize("which", sm.MODELS)
def test_run_stops_at_the_step_that_shortens_a_log(vt, spaces, which):
    sp = spaces(which, "321")
    lv, fp, acts, _n = _first_level(sp, sm.log_never_shrinks, 10)
    assert lv is not None and lv.level == 9 and acts == {"ReceiveSV"}   # the issue's figure, from the oracle
    m = _model(vt, which, "321")
    w = m.compile_step_predicates("LogShrinks == ~(" + sm.LOG_NEVER_SHRINKS + ")")
    mc = vt.ModelChecker(m, **RUN_SIZES)
    assert mc.run(step_never=w) == "violation"
    wit = mc.witness
    assert mc.level == lv.level and wit["level"] == lv.level and wit["name"] == "LogShrinks" and wit["kind"] == "violation"
    assert wit["action"] in acts and wit["fp"] == fp
    tr = mc.step_witness_trace()
    mc.close()
    assert len(tr) == lv.level + 1 and tr[0][0] == "Initial predicate" and tr[-1][0] == wit["action"]
    for (_a0, r0), (a1, r1) in zip(tr, tr[1:]):                     # every consecutive pair is an oracle successor, under the action named
        assert any(vt.ACTION_NAMES[s["action"]] == a1 and _norm(sp.fixed, s["words"]) == _norm(sp.fixed, r1) for s in sp.orc.successors(sp.P, r0))
    assert int(sp.orc.fingerprint(sp.P, tr[-2][1])[0]) == fp
    parent, child = (sp.po.unpack(sp.PM, [int(x) for x in r]) for r in (tr[-2][1], tr[-1][1]))
    assert not sm.log_never_shrinks(parent, child, tr[-1][0])
    mc = vt.ModelChecker(m, **RUN_SIZES)                              # step_reach reports the same pair as "reached"
    assert mc.run(step_reach=w) == "reached" and mc.witness["fp"] == fp and mc.witness["kind"] == "reached"
    mc.close()
    m2 = _model(vt, which, "222")
    mc = vt.ModelChecker(m2, **SIZES)
    assert mc.run(step_never=m2.compile_step_predicates("Lost == ~(" + sm.COMMITTED_PREFIX_STABLE + ")")) == "exhausted" and mc.witness is None
    mc.close()


def _run_cli(args):
    return subprocess.run([CLI] + args + ["-noTLA", "-tableLog2", "20", "-frontierGiB", "0.1"], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("which", sm.MODELS)
def test_cli_step_invariant_step_reach_and_step_report(vt, spaces, which, tmp_path):
    if which == "second":
        from test_model2_host_cpu import _cfg
    else:
        from test_model3_host_cpu import _cfg
    sp = spaces(which, "321")
    cfg = _cfg(tmp_path, R=3, vals=", ".join(sp.values), L=1)
    example = os.path.join(ROOT, "tools", "steps_model%d_example.txt" % (2 if which == "second" else 3))
    lv, _fp, acts, n_bad = _first_level(sp, sm.log_never_shrinks, 10)
    if which == "second":                                           # -stepInvariant, its trace through -validateTrace, and the -json line
        out = str(tmp_path / "step.tla")
        r = _run_cli(["-config", cfg, "-steps", example, "-stepInvariant", "LogNeverShrinks", "-maxDepth", "11", "-dumpTrace", "tla", out])
        assert r.returncode == 12, r.stdout + r.stderr
        assert "Error: Action property LogNeverShrinks is violated." in r.stdout and "Error: The behavior up to this point is:" in r.stdout
        blocks = [ln for ln in r.stdout.splitlines() if ln.startswith("State ") and ": <" in ln]
        assert len(blocks) == lv.level + 1 and blocks[0] == "State 1: <Initial predicate>" and blocks[-1] == "State %d: <%s>" % (lv.level + 1, next(iter(acts)))
        assert "no_progress_ctr" in r.stdout and "rep_client_table" not in r.stdout          # the model's own printer
        v = _run_cli(["-config", cfg, "-validateTrace", out])
        assert v.returncode == 0 and ("%d states read" % (lv.level + 1)) in v.stdout and "The trace is a behaviour of the model." in v.stdout, v.stdout + v.stderr
        rj = _run_cli(["-config", cfg, "-steps", example, "-stepInvariant", "LogNeverShrinks", "-maxDepth", "11", "-json"])
        hit = [json.loads(ln) for ln in rj.stdout.splitlines() if ln.startswith("{") and "action_property_violated" in ln]
        assert rj.returncode == 12 and len(hit) == 1 and hit[0]["action_property_violated"] == "LogNeverShrinks" and hit[0]["level"] == lv.level
        assert hit[0]["action"] in acts
    else:                                                           # -stepReach of a helper's negation: exit 0, "Step satisfying"
        f = tmp_path / "steps.txt"
        f.write_text(open(example).read() + "\nLogShrinks == ~LogNeverShrinks\n")
        r = _run_cli(["-config", cfg, "-steps", str(f), "-stepReach", "LogShrinks", "-maxDepth", "11"])
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("Step satisfying LogShrinks found at depth %d (%d of the level's %d transitions satisfy it)." % (lv.level, n_bad, sp.generated[lv.level - 1])) in r.stdout
        assert ("The last step is %s of State %d." % (next(iter(acts)), lv.level)) in r.stdout and "rep_app_state" in r.stdout
        r3 = _run_cli(["-config", cfg, "-steps", str(f), "-stepReach", "LogShrinks", "-maxDepth", str(lv.level - 1)])
        assert r3.returncode == 14, r3.stdout + r3.stderr
    # the report: per-level totals of the example's properties, no stop
    names = [ln.split("==")[0].strip() for ln in open(example) if "==" in ln and not ln.startswith("\\*")]
    per_level = {}
    for x in sp.levels[:10]:
        c = collections.Counter()
        for i in range(len(x.recs)):
            for a, _cn, ch in sp.succ(x, i):
                c["pairs"] += 1
                for nm in names:
                    c[nm] += sm.EXAMPLE[nm](x.states[i], ch, a)
        per_level[x.level] = c
    r4 = _run_cli(["-config", cfg, "-steps", example, "-stepReport", "-json", "-maxDepth", "10"])
    assert r4.returncode == 0, r4.stdout + r4.stderr
    got = {}
    for row in (json.loads(ln) for ln in r4.stdout.splitlines() if ln.startswith("{")):
        assert row["steps"]["errors"] == 0
        got[row["level"] if row.get("expanded") is False else row["level"] - 1] = row["steps"]
    assert sorted(got) == sorted(per_level)
    for lvl, c in per_level.items():
        assert got[lvl]["pairs"] == c["pairs"] and {nm: got[lvl]["count"][nm] for nm in names} == {nm: c[nm] for nm in names}, lvl
    # error exits: a name the file does not export, a file that does not compile (the model's own refusal, with the file's name and the position)
    assert _run_cli(["-config", cfg, "-steps", example, "-stepReach", "Shrinks"]).returncode == 2
    bad = tmp_path / "bad.txt"
    bad.write_text("A == UNCHANGED messages\n")
    r5 = _run_cli(["-config", cfg, "-steps", str(bad), "-stepReport"])
    assert r5.returncode == 1 and "bad.txt:1:" in r5.stderr and "UNCHANGED messages" in r5.stderr


# ---------------------------------------------------------------------------------------------------------------------
# 8. a program from a wrong entry or model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sm.MODELS)
def test_step_scan_refuses_a_program_from_a_wrong_entry_or_model(vt, which):
    m = _model(vt, which, "222")
    w = m.compile_step_predicates("aux_svc' >= aux_svc")
    mc = vt.ModelChecker(m, **SIZES)
    with pytest.raises(vt.VsrmcError) as e:
        mc.step_pairs()
    assert e.value.code == -6
    other = _model(vt, "third" if which == "second" else "second", "222")
    vsr = vt.Model.from_constants(R=2, C_=1, n=2, L=2, symmetry=False)
    for prog in (vsr.compile_step("aux_svc' >= aux_svc"), vsr.compile_step_predicates("aux_svc' >= aux_svc"), other.compile_step_predicates("aux_svc' >= aux_svc"),
                 _model(vt, which, "321").compile_step_predicates("aux_svc' >= aux_svc")):
        with pytest.raises(vt.VsrmcError) as e:
            mc.step_scan(prog)
        assert e.value.code == -1 and "compiled for another model" in e.value.message
    with pytest.raises(vt.VsrmcError) as e:
        mc.step_scan(m.compile_predicates("TRUE"))                   # a state program
    assert e.value.code == -1 and "vsrmc_step_compile" in e.value.message
    with pytest.raises(vt.VsrmcError) as e:
        mc.where_scan(w)                                            # and the reverse
    assert e.value.code == -1 and "step program" in e.value.message
    for _ in range(5):
        mc.step()
    t = mc.step_scan(w)
    assert t["level"] == 6 and t["count"] == [t["n_pairs"]] and t["n_err"] == 0
    mc.deepen()
    with pytest.raises(vt.VsrmcError) as e:
        mc.step_scan(w)
    assert e.value.code == -6 and "seen-set only" in e.value.message
    mc.close()
    vmc = vt.ModelChecker(vsr, **SIZES)                              # an analysis model's program on a VSR.tla checker
    with pytest.raises(vt.VsrmcError) as e:
        vmc.step_scan(w)
    assert e.value.code == -1 and "compiled for another model" in e.value.message
    vmc.close()
