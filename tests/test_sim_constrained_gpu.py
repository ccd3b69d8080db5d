"""Random walks under a state constraint and / or an action constraint on the GPU (`-m gpu`): k_simulate_constrained through Model.simulate_constrained
and the command line.  The counts of the report mode are compared, exactly, with the iteration contract restated in Python (tests/sim_constrained_model.py:
successors from Model.get_next_states, the generator and the tried set written out) under hand-written Python predicates over the oracle's unpack of
every state and pair (constraint_reference.py, action_constraint_reference.py and the predicate references — the reference is never the parser).  Every
case first asserts on the MODEL's figures that it is not vacuous.  100 walkers: the second wave has 36 walkers and 28 idle lanes; two rounds: the tried
sets cross a launch."""
import os
import re
import subprocess

import pytest

import action_constraint_reference as ar
import constraint_reference as cr
import deep_predicates_reference as dp
import sim_constrained_model as scm
import step_models_reference as smr
import step_reference as sr
import where_reference as wr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
TOOLS = os.path.join(ROOT, "tools")
KW = dict(n_walkers=100, seed=11, max_rounds=2)
FLOOR = 100                                                          # blocked / pruned tries the model must show where a constraint of the kind is attached


@pytest.fixture(scope="module")
def vt():
    import vsr_tlaplus_amd as vt
    assert vt.load().vsrmc_device_count() >= 1, "no HIP device visible"
    return vt


def _named(name, texts, fn):
    """(name, body, function) as the reference sets hold them, from a `Name == body` text"""
    text = texts[name] if isinstance(texts, dict) else texts
    assert text.startswith(name + " == ")
    return (name, text[len(name) + 4:], fn)


VIEWS_BELOW_3 = ("ViewsBelow3", r"\A r \in replicas : rep_view_number[r] < 3", cr.views_below(3))
VIEWS_BELOW_2 = ("ViewsBelow2", r"\A r \in replicas : rep_view_number[r] < 2", cr.views_below(2))
REPLICA3_NORMAL = _named("Replica3Normal", cr.TEXTS, cr.replica3_normal)
NOT_ALL_IN_VC = _named("NotAllInViewChange", cr.TEXTS, cr.not_all_in_view_change)
INIT_ONLY = _named("InitOnly", cr.TEXTS, cr.init_only)
NO_STATE_TRANSFER = _named("NoStateTransfer", cr.TEXTS, cr.no_state_transfer)
QUIET_CLIENT = _named("QuietClient", ar.TEXTS, ar.quiet_client)
TIMERS_IN_VIEW_1 = _named("TimersInView1", ar.TEXTS, ar.timers_in_view_1)
COMMIT_NEVER_DECREASES = _named("CommitNeverDecreases", ar.TEXTS, ar.commit_never_decreases)
STEP_TRUE, STEP_FALSE = _named("True", ar.TEXTS, ar.always), _named("False", ar.TEXTS, ar.never)
STATE_TRUE = _named("True", cr.TEXTS, lambda s: True)
NARROW_NETWORK = _named("NarrowNetwork", cr.TEXTS, cr.narrow_network)
UNSETTLED, VIEW_CHANGED = wr.SET_A[4], sr.SET_A[0]
UNCHANGED_APP_2 = [p for p in smr.SET_3 if p[0] == "UnchangedApp2"][0]
LOG_DIVERGENCE = ("LogDivergence", wr.LOG_DIVERGENCE, wr.log_divergence)
COMMITTED_PREFIX_STABLE = ("CommittedPrefixStable", sr.COMMITTED_PREFIX_STABLE, sr.committed_prefix_stable)
ROW1_UNCHANGED = [p for p in dp.STEP_C2 if p[0] == "Row1Unchanged"][0]
LOG_NEVER_SHRINKS_3 = [p for p in smr.SET_A["third"] if p[0] == "LogNeverShrinks"][0]


def _setup(vt, which, R, C, n, L):
    """-> (Model, unpack(words) of the CPU oracle's codec)"""
    if which == "third":
        from oracle import pyoracle3
        PM = pyoracle3.Model(R, tuple("abc"[:n]), L)
        return vt.Model.third_model(R=R, n=n, L=L), lambda words: pyoracle3.unpack(PM, words)
    from oracle import pycodec, pyoracle as po
    policy = dict(assume_commit_number=True) if C == 2 else {}
    PM = po.Model(R, C, tuple("v%d" % (i + 1) for i in range(n)), L, **policy)
    return vt.Model.from_constants(R=R, C_=C, n=n, L=L, **policy), lambda words: pycodec.unpack(PM, words)


def _index(preds, con):
    return None if con is None else [p[0] for p in preds].index(con)


def _both(vt, space, max_depth, state_preds=(), state_con=None, step_preds=(), step_con=None, rounds=2, **kw):
    """the model's figures and the kernel's, for one attachment; con: the NAME of the constraint among the predicates of its program"""
    m, unpack = _setup(vt, *space)
    want = scm.model_counts(vt.ACTION_NAMES, m, unpack, 100, max_depth, 11, 64 * rounds, state_preds=list(state_preds), state_bits=wr.bits_of,
                            state_con=_index(state_preds, state_con), step_preds=list(step_preds), step_bits=sr.bits_of, step_con=_index(step_preds, step_con))
    ws = m.compile_predicates(wr.text_of(state_preds)) if state_preds else None
    wp = m.compile_step_predicates(wr.text_of(step_preds)) if step_preds else None
    r = m.simulate_constrained(state=ws, constraint=state_con, step=wp, action_constraint=step_con, stop=False, max_depth=max_depth,
                               **dict(KW, max_rounds=rounds, **kw))
    print("simulate_constrained %s depth %d, state %s / %s, step %s / %s: model steps %d walks %d blocked %d pruned %d stuck %d, largest enabled count %d; "
          "kernel steps %d walks %d blocked %d pruned %d stuck %d" %
          (space, max_depth, [p[0] for p in state_preds], state_con, [p[0] for p in step_preds], step_con, want["steps"], want["walks"], want["blocked"],
           want["pruned"], want["stuck"], want["max_enabled"], r["steps"], r["walks"], r["blocked"], r["pruned"], r["stuck"]))
    return m, want, r


def _assert_equal(r, want, state_preds, step_preds, rounds=2):
    assert (r["found"], r["rounds"], r["init_pruned"]) == (0, rounds, False)
    got = {k: r[k] for k in ("steps", "walks", "blocked", "pruned", "stuck", "n_states", "n_pairs")}
    assert got == {k: want[k] for k in got}
    assert [r["count_state"][p[0]] for p in state_preds] == want["cs"]
    assert [r["count_step"][p[0]] for p in step_preds] == want["cp"]
    assert r["steps"] + r["walks"] + r["blocked"] + r["pruned"] == 64 * rounds * 100


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact counts against the model
# ---------------------------------------------------------------------------------------------------------------------
CASES = {
    "replica3-normal": dict(space=("first", 3, 1, 2, 1), max_depth=12, state_preds=[REPLICA3_NORMAL], state_con="Replica3Normal"),
    "quiet-client": dict(space=("first", 3, 1, 2, 1), max_depth=12, step_preds=[QUIET_CLIENT], step_con="QuietClient"),
    # TimersInView1 with ViewsBelow3 is what one would pair first, but with StartViewOnTimerLimit = 1 no timer fires outside view 1 and no view reaches 3:
    # the model shows 0 blocked and 0 pruned at depth 12 (kept below as a case of its own: constraints that never bite change nothing).  NarrowNetwork (two
    # nested message loops in the constraint) with QuietClient bites on both sides; LogDivergence and CommittedPrefixStable are the report queries, Unsettled
    # and ViewChanged two more that take both verdicts at this depth
    "both-with-queries": dict(space=("first", 3, 1, 2, 1), max_depth=12, state_preds=[LOG_DIVERGENCE, UNSETTLED, NARROW_NETWORK], state_con="NarrowNetwork",
                              step_preds=[COMMITTED_PREFIX_STABLE, VIEW_CHANGED, QUIET_CLIENT], step_con="QuietClient"),
    "two-replicas": dict(space=("first", 2, 1, 1, 1), max_depth=30, state_preds=[NARROW_NETWORK], state_con="NarrowNetwork", step_preds=[QUIET_CLIENT],
                         step_con="QuietClient"),
    "five-replicas": dict(space=("first", 5, 1, 2, 1), max_depth=40, state_preds=[REPLICA3_NORMAL], state_con="Replica3Normal"),
    "two-clients": dict(space=("first", 3, 2, 3, 1), max_depth=40, step_preds=[ROW1_UNCHANGED], step_con="Row1Unchanged"),
    # of the example files of the analysis models, NoStateTransfer / NobodyEntersStateTransfer never bite at depth 16 (nobody enters StateTransfer that early)
    # and ViewsBelow2 leaves LogNeverShrinks nothing to block (logs shrink in view changes only): ViewsBelow2 of the example file, with UnchangedApp2 of
    # step_models_reference.py — replica 2 never executes — which reads rep_app_state', the op only VR_APP_STATE has
    "app-state": dict(space=("third", 3, 0, 2, 1), max_depth=16, state_preds=[VIEWS_BELOW_2], state_con="ViewsBelow2",
                      step_preds=[UNCHANGED_APP_2], step_con="UnchangedApp2"),
}
# pairings that never bite, by the model: the constraints are evaluated on every try and change nothing
IDLE_CASES = {
    "timers-views": dict(space=("first", 3, 1, 2, 1), max_depth=12, state_preds=[LOG_DIVERGENCE, VIEWS_BELOW_3], state_con="ViewsBelow3",
                         step_preds=[COMMITTED_PREFIX_STABLE, TIMERS_IN_VIEW_1], step_con="TimersInView1"),
    "app-state-example-files": dict(space=("third", 3, 0, 2, 1), max_depth=16, state_preds=[NO_STATE_TRANSFER], state_con="NoStateTransfer",
                                    step_preds=[LOG_NEVER_SHRINKS_3], step_con="LogNeverShrinks"),
}


@pytest.fixture(scope="module")
def case_runs(vt):
    """every case is run once; the identity test looks at the same results"""
    memo = {}

    def get(key):
        if key not in memo:
            memo[key] = _both(vt, **CASES[key])
        return memo[key]
    return get


@pytest.mark.parametrize("key", sorted(CASES))
def test_counts_equal_the_model(vt, case_runs, key):
    """(5,1,2,1): broadcasts append R - 1 bag entries and use every Delta slot, replica blocks have four words — the whole undo log.  (3,2,3,1): the policy
    assume_commit_number, a constraint of the two-client sets.  (3,{a,b},1) of VR_APP_STATE: the instantiation <2000>, the constraints of the example files
    of the analysis models."""
    case = CASES[key]
    _m, want, r = case_runs(key)
    if case.get("step_con"):
        assert want["blocked"] >= FLOOR, want["blocked"]             # by the Python model, which does not run the kernel under test
    if case.get("state_con"):
        assert want["pruned"] >= FLOOR, want["pruned"]
    assert want["steps"] >= FLOOR and want["max_enabled"] <= scm.TRIED_BITS
    _assert_equal(r, want, case.get("state_preds", ()), case.get("step_preds", ()))


@pytest.mark.parametrize("key", sorted(IDLE_CASES))
def test_counts_equal_the_model_where_a_constraint_hardly_bites(vt, key):
    case = IDLE_CASES[key]
    _m, want, r = _both(vt, **case)
    assert want["blocked"] + want["pruned"] < 2 * FLOOR and want["steps"] >= FLOOR
    _assert_equal(r, want, case["state_preds"], case["step_preds"])


# ---------------------------------------------------------------------------------------------------------------------
# 2. directed cases
# ---------------------------------------------------------------------------------------------------------------------
def test_action_constraint_never(vt):
    """every walk is start, one blocked try per enabled instance of Init, stuck"""
    m, want, r = _both(vt, ("first", 3, 1, 2, 1), 12, step_preds=[STEP_FALSE], step_con="False")
    e = len(want["walkers"].rows[want["walkers"].init])
    assert e >= 2 and want["stuck"] >= FLOOR
    _assert_equal(r, want, (), [STEP_FALSE])
    assert (r["steps"], r["pruned"], r["n_pairs"], r["count_step"]["False"]) == (0, 0, 0, 0) and r["walks"] == r["stuck"] + 100
    assert 0 <= r["blocked"] - r["stuck"] * e <= 100 * e              # the walks the end of the round cut


def test_state_constraint_init_only(vt):
    """the same through apply and undo: every try moves into a successor of Init and is put back — a word the undo log missed would change Init's guards,
    and with them the number of tries per walk"""
    m, want, r = _both(vt, ("first", 3, 1, 2, 1), 12, state_preds=[INIT_ONLY], state_con="InitOnly")
    e = len(want["walkers"].rows[want["walkers"].init])
    assert e >= 2 and want["stuck"] >= FLOOR
    _assert_equal(r, want, [INIT_ONLY], ())
    assert (r["steps"], r["blocked"]) == (0, 0) and r["walks"] == r["stuck"] + 100 == r["n_states"] == r["count_state"]["InitOnly"]
    assert 0 <= r["pruned"] - r["stuck"] * e <= 100 * e
    # five replicas: four-word replica blocks, broadcasts out of Init
    m5, want5, r5 = _both(vt, ("first", 5, 1, 2, 1), 12, state_preds=[INIT_ONLY], state_con="InitOnly")
    _assert_equal(r5, want5, [INIT_ONLY], ())
    assert r5["steps"] == 0 and r5["stuck"] >= FLOOR


def test_always_equals_simulate_where(vt):
    """TRUE for both constraints: nothing is blocked or pruned, and the walks are those of the untouched kernel with the same programs, seed and rounds"""
    m, _unpack = _setup(vt, "first", 3, 1, 2, 1)
    state_preds, step_preds = wr.SET_A[:7] + [STATE_TRUE], sr.SET_B[:7] + [STEP_TRUE]   # (sr.SET_A reads the aux variables: refused beside a constraint)
    ws, wp = m.compile_predicates(wr.text_of(state_preds)), m.compile_step_predicates(wr.text_of(step_preds))
    kw = dict(stop=False, n_walkers=100, max_depth=12, seed=11, max_rounds=4)
    a = m.simulate_where(state=ws, step=wp, **kw)
    b = m.simulate_constrained(state=ws, constraint="True", step=wp, action_constraint="True", **kw)
    assert (b["blocked"], b["pruned"], b["stuck"]) == (0, 0, 0)
    for k in ("steps", "walks", "n_states", "n_pairs", "count_state", "count_step", "rounds", "found"):
        assert a[k] == b[k], k
    assert a["steps"] > 0 and sum(a["count_state"].values()) > a["n_states"] and sum(a["count_step"].values()) > a["n_pairs"]
    # each program alone: the instantiations with the other one compiled out
    b1 = m.simulate_constrained(state=ws, constraint="True", **kw)
    b2 = m.simulate_constrained(step=wp, action_constraint="True", **kw)
    assert (b1["steps"], b1["walks"], b1["count_state"], b1["n_pairs"]) == (a["steps"], a["walks"], a["count_state"], 0)
    assert (b2["steps"], b2["walks"], b2["count_step"], b2["n_states"]) == (a["steps"], a["walks"], a["count_step"], 0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. identities and determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_identities_and_determinism(vt, case_runs):
    m, want, r = case_runs("both-with-queries")
    assert r["steps"] + r["walks"] + r["blocked"] + r["pruned"] == 64 * 2 * 100
    assert r["n_states"] == r["steps"] + r["walks"] and r["n_pairs"] == r["steps"]
    assert r["count_state"]["NarrowNetwork"] == r["n_states"] and r["count_step"]["QuietClient"] == r["n_pairs"]
    assert 0 < r["count_state"]["Unsettled"] < r["n_states"] and 0 < r["count_step"]["ViewChanged"] < r["n_pairs"]
    case = CASES["both-with-queries"]
    ws, wp = m.compile_predicates(wr.text_of(case["state_preds"])), m.compile_step_predicates(wr.text_of(case["step_preds"]))
    run = lambda **kw: m.simulate_constrained(state=ws, constraint="NarrowNetwork", step=wp, action_constraint="QuietClient", stop=False, max_depth=12,  # noqa: E731
                                              **dict(KW, **kw))
    strip = lambda d: {k: v for k, v in d.items() if k != "seconds"}   # noqa: E731
    assert strip(run()) == strip(r)
    other = run(seed=12)
    assert strip(other) != strip(r) and other["steps"] + other["walks"] + other["blocked"] + other["pruned"] == 64 * 2 * 100
    # one launch more continues the same walks: the tried sets and the records are kept between launches
    longer = run(max_rounds=3)
    assert longer["steps"] > r["steps"] and longer["n_states"] == longer["steps"] + longer["walks"]


# ---------------------------------------------------------------------------------------------------------------------
# 4. semantics: the model without the steps that lower a commit number
# ---------------------------------------------------------------------------------------------------------------------
def _query(text, name, negate=False):
    """what the command line compiles for -reach NAME / -invariant NAME: the file with every definition made LOCAL, then the one exported query"""
    return re.sub(r"(?m)^(?!LOCAL\b)(\w+\s*==)", r"LOCAL \1", text) + "\nQuery0 == " + ("~" if negate else "") + name + "\n"


def test_commit_never_decreases_removes_the_violation(vt):
    """(3,1,1,1), stop mode: without a constraint ~CommitMonotonic is hit (test_sim_where_gpu.py: a walk that ends in ReceiveSV); with CommitNeverDecreases
    attached no walk takes such a step, in at least as many rounds"""
    m, _unpack = _setup(vt, "first", 3, 1, 1, 1)
    text = _query(open(os.path.join(TOOLS, "steps_example.txt")).read(), "CommitMonotonic", negate=True)
    kw = dict(stop=True, n_walkers=1 << 14, max_depth=40, seed=3)
    plain = m.simulate_where(step=m.compile_step_predicates(text), max_seconds=20.0, **kw)
    assert plain["found"] == 4 and plain["hit"] == ["Query0"] and plain["trace"][-1][0] == "ReceiveSV"
    # (a program of its own: the example file also defines a predicate over aux_svc, which no constraint's program may read)
    wp = m.compile_step_predicates("Query0 == ~(" + sr.COMMIT_MONOTONIC + ")\n" + ar.TEXTS["CommitNeverDecreases"] + "\n")
    r = m.simulate_constrained(step=wp, action_constraint="CommitNeverDecreases", max_rounds=max(4, plain["rounds"]), **kw)
    print("CommitNeverDecreases on (3,1,1,1): unconstrained hit after %d rounds; constrained: found %d in %d rounds, %d steps, %d blocked" %
          (plain["rounds"], r["found"], r["rounds"], r["steps"], r["blocked"]))
    assert r["found"] == 0 and r["rounds"] >= 4 and r["blocked"] > 0 and r["count_step"]["Query0"] == 0 and r["count_step"]["CommitNeverDecreases"] == r["n_pairs"]


# ---------------------------------------------------------------------------------------------------------------------
# 5. witnesses stay in the model
# ---------------------------------------------------------------------------------------------------------------------
def test_reach_witness_stays_in_the_model(vt):
    """-reach under Replica3Normal on (3,1,2,1).  The query that comes to mind, LogDivergence, has no witness there: the constrained BFS exhausts that model
    (4 924 states, depth 25) without one — see the test below.  TwoNormalViews has: replicas 1 and 2 go to view 2 while replica 3 stays Normal in view 1."""
    m, unpack = _setup(vt, "first", 3, 1, 2, 1)
    two_normal_views = wr.SET_A[2]
    text = "Query0 == " + two_normal_views[1] + "\n" + cr.TEXTS["Replica3Normal"] + "\n"   # -reach TwoNormalViews -walkConstraint Replica3Normal
    r = m.simulate_constrained(state=m.compile_predicates(text), constraint="Replica3Normal", stop=True, n_walkers=1 << 14, max_depth=40, seed=3, max_seconds=20.0)
    print("reach TwoNormalViews under Replica3Normal: found %d after %d rounds, %d steps, %d pruned; the walk has %d states" %
          (r["found"], r["rounds"], r["steps"], r["pruned"], len(r["trace"] or [])))
    assert r["found"] == 3 and r["hit"] == ["Query0"] and r["pruned"] > 0
    tr = m.replay(r["ordinals"])                                     # vsrmc_model_replay
    assert len(tr) == r["viol_steps"] + 1 >= 5 and tr[0][0] == "Initial predicate"
    views = [unpack([int(x) for x in rec]) for _, rec in tr]
    assert all(cr.replica3_normal(s) for s in views)
    assert [two_normal_views[2](s) for s in views] == [False] * (len(tr) - 1) + [True]
    chk = m.check_trace([rec for _, rec in tr])                      # every step is a generated successor
    assert chk["ok"] and len(chk["ords"]) == len(r["ordinals"])


def test_log_divergence_under_replica3_normal_agrees_with_the_constrained_bfs(vt):
    """-reach LogDivergence under Replica3Normal on (3,1,2,1): the constrained BFS (k_constrain, §9h) exhausts the model and meets no such state, so a walk
    that reported one would have left the model.  The walks meet none either, in 4 rounds of 2^14 walkers to depth 40, while pruning; without the constraint
    the same walks do reach it (test_sim_where_gpu.py)."""
    m, _unpack = _setup(vt, "first", 3, 1, 2, 1)
    w = m.compile_predicates("Query0 == " + wr.LOG_DIVERGENCE + "\n" + cr.TEXTS["Replica3Normal"] + "\n")
    mc = vt.ModelChecker(m, device=0, table_log2=20, frontier_words=1 << 22, frontier_states=1 << 17, pending_entries=1 << 17)
    mc.constrain(w, "Replica3Normal")
    assert mc.run(reach=m.compile_predicates("Query0 == " + wr.LOG_DIVERGENCE)) == "exhausted" and mc.distinct == 4924
    kw = dict(stop=True, n_walkers=1 << 14, max_depth=40, seed=3, max_rounds=4)
    r = m.simulate_constrained(state=w, constraint="Replica3Normal", **kw)
    assert (r["found"], r["rounds"], r["count_state"]["Query0"]) == (0, 4, 0) and r["pruned"] > 0 and r["count_state"]["Replica3Normal"] == r["n_states"]
    free = m.simulate_where(state=m.compile_predicates("Query0 == " + wr.LOG_DIVERGENCE), stop=True, n_walkers=1 << 14, max_depth=40, seed=3, max_seconds=20.0)
    assert free["found"] == 3


# ---------------------------------------------------------------------------------------------------------------------
# 6. hits on pruned states
# ---------------------------------------------------------------------------------------------------------------------
def test_invariant_violated_on_a_pruned_state(vt):
    """under Replica3Normal no in-model state has every replica in ViewChange: the states that violate NotAllInViewChange are successors of in-model states,
    pruned on arrival.  pruned_stop_mask reports them, with the step into the pruned state at the end of the walk"""
    m, unpack = _setup(vt, "first", 3, 1, 2, 1)
    text = "LOCAL " + cr.TEXTS["NotAllInViewChange"] + "\nViolated == ~NotAllInViewChange\n" + cr.TEXTS["Replica3Normal"] + "\n"
    w = m.compile_predicates(text)
    assert list(w.names) == ["Violated", "Replica3Normal"]
    kw = dict(state=w, constraint="Replica3Normal", stop=True, n_walkers=4096, max_depth=12, seed=3)
    r = m.simulate_constrained(pruned_stop=["Violated"], max_seconds=20.0, **kw)
    print("NotAllInViewChange on a pruned state: found %d after %d rounds, walk of %d steps" % (r["found"], r["rounds"], r["viol_steps"]))
    assert r["found"] == 3 and r["hit"] == ["Violated"] and r["viol_steps"] >= 1
    views = [unpack([int(x) for x in rec]) for _, rec in r["trace"]]
    assert len(views) == r["viol_steps"] + 1
    assert all(cr.replica3_normal(s) and cr.not_all_in_view_change(s) for s in views[:-1])
    assert not cr.replica3_normal(views[-1]) and not cr.not_all_in_view_change(views[-1])
    assert m.check_trace([rec for _, rec in r["trace"]])["ok"]
    quiet = m.simulate_constrained(pruned_stop=0, max_rounds=r["rounds"], **kw)
    assert (quiet["found"], quiet["rounds"], quiet["count_state"]["Violated"]) == (0, r["rounds"], 0) and quiet["pruned"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. the command line
# ---------------------------------------------------------------------------------------------------------------------
def _cli(args):
    return subprocess.run([CLI] + args + ["-noTLA"], capture_output=True, text=True, timeout=300)


CLOSING = r"Walk constraints: (\d+) tries blocked by the action constraint, (\d+) tries pruned by the state constraint, (\d+) walks ended stuck .*; (\d+) steps taken\."


def test_cli_prints_the_counts_of_the_api(vt, tmp_path):
    from test_host_cpu import _cfg
    cfg = _cfg(tmp_path, R=3, vals="v1, v2", L=1)
    m, _unpack = _setup(vt, "first", 3, 1, 2, 1)
    sim = ["-config", cfg, "-simulate", "-simRounds", "2", "-walkers", "100", "-depth", "12", "-seed", "11"]
    api = dict(stop=False, max_depth=12, **KW)
    # -walkConstraint, counted over the file's own exports
    con = os.path.join(TOOLS, "constraints_example.txt")
    want = m.simulate_constrained(state=m.compile_predicates(open(con).read()), constraint="Replica3Normal", **api)
    r = _cli(sim + ["-predicates", con, "-walkConstraint", "Replica3Normal", "-whereReport"])
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = {nm: (int(a), int(b)) for nm, a, b in re.findall(r"Where report: (\w+) holds in (\d+) of (\d+) states", r.stdout)}
    assert got == {nm: (cnt, want["n_states"]) for nm, cnt in want["count_state"].items()} and len(got) == 4
    assert [int(x) for x in re.search(CLOSING, r.stdout).groups()] == [0, want["pruned"], want["stuck"], want["steps"]] and want["pruned"] >= FLOOR
    # -walkActionConstraint
    act = os.path.join(TOOLS, "action_constraints_example.txt")
    want = m.simulate_constrained(step=m.compile_step_predicates(open(act).read()), action_constraint="QuietClient", **api)
    r = _cli(sim + ["-steps", act, "-walkActionConstraint", "QuietClient", "-stepReport"])
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = {nm: (int(a), int(b)) for nm, a, b in re.findall(r"Step report: (\w+) holds on (\d+) of (\d+) pairs", r.stdout)}
    assert got == {nm: (cnt, want["n_pairs"]) for nm, cnt in want["count_step"].items()} and len(got) == 3
    assert [int(x) for x in re.search(CLOSING, r.stdout).groups()] == [want["blocked"], 0, want["stuck"], want["steps"]] and want["blocked"] >= FLOOR
    # no query at all: the built-in invariants on the constrained walks; both flags together with a query
    r = _cli(sim + ["-predicates", con, "-walkConstraint", "Replica3Normal"])
    assert r.returncode == 0 and "Simulation stopped" in r.stdout and re.search(CLOSING, r.stdout), (r.stdout, r.stderr)
    r = _cli(sim + ["-predicates", con, "-walkConstraint", "Replica3Normal", "-invariant", "NotAllInViewChange", "-steps", act, "-walkActionConstraint", "QuietClient",
                    "-walkers", "4096", "-simRounds", "40"])
    print("cli -walkConstraint Replica3Normal -walkActionConstraint QuietClient -invariant NotAllInViewChange: " + r.stdout.strip().splitlines()[-1])
    assert r.returncode == 12 and "Error: Invariant NotAllInViewChange is violated." in r.stdout and "Error: The behavior up to this point is:" in r.stdout
