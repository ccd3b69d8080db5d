"""Simulation with state / step predicates on the GPU (`-m gpu`): k_simulate_where through Model.simulate_where and the command line.  The counts of the
report mode are compared, exactly, with the iteration contract restated in Python (tests/sim_where_model.py: successors from Model.get_next_states, the
generator written out) and hand-written Python predicates over the oracle's unpack of every state stood on and pair taken (where_reference.py,
step_reference.py and their *_models_* neighbours — the reference is never the parser).  Walks that stop are checked to be behaviours by the CPU oracle."""
import os
import re
import subprocess

import pytest

import deep_predicates_reference as dp
import sim_where_model as sm
import step_models_reference as smr
import step_reference as sr
import where_models_reference as wm
import where_reference as wr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
TOOLS = os.path.join(ROOT, "tools")


@pytest.fixture(scope="module")
def vt():
    import vsr_tlaplus_amd as vt
    assert vt.load().vsrmc_device_count() >= 1, "no HIP device visible"
    return vt


@pytest.fixture(scope="module")
def orc():
    from oracle import orc
    return orc


def _query(text, name, negate=False):
    """what the command line compiles for -reach NAME / -invariant NAME: the file with every definition made LOCAL, then the one exported query"""
    return re.sub(r"(?m)^(?!LOCAL\b)(\w+\s*==)", r"LOCAL \1", text) + "\nQuery0 == " + ("~" if negate else "") + name + "\n"


def _check_walk_with_oracle(orc, P, trace):
    """Init, then one oracle successor after the other, under the action the trace names"""
    norm = lambda w: tuple(int(x) for x in orc.normalise(P, w))   # noqa: E731
    assert norm(trace[0][1]) == norm(orc.init_record(P)) and trace[0][0] == "Initial predicate"
    for t in range(len(trace) - 1):
        hits = [s for s in orc.successors(P, trace[t][1]) if norm(s["words"]) == norm(trace[t + 1][1])]
        assert hits and any(orc.ACTIONS[h["action"]] == trace[t + 1][0] for h in hits), t


def _model_counts(vt, m, unpack, state_preds, state_bits, step_preds, step_bits, n_walkers, max_depth, seed, iterations):
    """the sums the contract gives: bits of every state stood on and every pair taken, through the Python predicates"""
    W = sm.Walkers(m, n_walkers, max_depth, seed)
    views, sb, pb = {}, {}, {}

    def view(key):
        if key not in views:
            views[key] = unpack(list(key))
        return views[key]
    cs, cp = [0] * len(state_preds), [0] * len(step_preds)
    n_states = n_pairs = n_mixed = 0
    for events in W.iterate(iterations):
        kinds = set(ev[0] for ev in events)
        n_mixed += len(kinds) == 2
        for ev in events:
            key = ev[1] if ev[0] == "start" else ev[2]
            if key not in sb:
                sb[key] = state_bits(state_preds, view(key))
            n_states += 1
            for k in range(len(state_preds)):
                cs[k] += (sb[key] >> k) & 1
            if ev[0] == "step":
                pk = (ev[1], ev[2], ev[3])
                if pk not in pb:
                    pb[pk] = step_bits(step_preds, view(ev[1]), view(ev[2]), vt.ACTION_NAMES[ev[3]])
                n_pairs += 1
                for k in range(len(step_preds)):
                    cp[k] += (pb[pk] >> k) & 1
    return dict(cs=cs, cp=cp, n_states=n_states, n_pairs=n_pairs, steps=W.steps, walks=W.walks, mixed=n_mixed)


def _assert_report_equals_model(r, want, state_preds, step_preds, n_walkers):
    print("simulate_where report: steps %d walks %d; state %s; step %s; model: iterations with starts and steps together %d" %
          (r["steps"], r["walks"], r["count_state"], r["count_step"], want["mixed"]))
    assert (r["found"], r["rounds"]) == (0, 1)
    assert (r["steps"], r["walks"], r["n_states"], r["n_pairs"]) == (want["steps"], want["walks"], want["n_states"], want["n_pairs"])
    assert r["n_states"] == 64 * n_walkers == r["steps"] + r["walks"] and r["n_pairs"] == r["steps"]
    assert [r["count_state"][p[0]] for p in state_preds] == want["cs"]
    assert [r["count_step"][p[0]] for p in step_preds] == want["cp"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact counts against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R, C, n, L, max_depth", [(3, 1, 2, 1, 12), (2, 1, 1, 1, 30), (5, 1, 2, 1, 40), (4, 1, 2, 1, 40), (3, 2, 3, 1, 40)])
def test_report_counts_equal_the_model(vt, R, C, n, L, max_depth):
    """100 walkers: the second wave has 36 walkers and 28 idle lanes, which must count nothing.  (2,1,1,1) has 76 states and its walks end in terminal
    states at different times: lanes of one wave start and step in the same iteration.  At five and four replicas (replica blocks of four words, broadcasts
    that append R - 1 bag entries to the walker's record in place) the walks run 40 steps deep, far enough to hold DoViewChanges, and a second pair of
    programs — the R >= 4 sets of deep_predicates_reference.py — is counted over the same walks.  (3,2,3,1), under the policy assume_commit_number: two clients,
    and the second pair of programs is the two-client sets — both rows of the client tables, client_id = 2 in logs and messages, the row ReceivePrepareMsg
    rewrites for the other client — over walks of 40 steps."""
    from oracle import pycodec, pyoracle as po
    policy = dict(assume_commit_number=True) if C == 2 else {}
    m = vt.Model.from_constants(R=R, C_=C, n=n, L=L, **policy)
    PM = po.Model(R, C, tuple("v%d" % (i + 1) for i in range(n)), L, **policy)
    ws, wp = m.compile_predicates(wr.text_of(wr.SET_A)), m.compile_step_predicates(sr.text_of(sr.SET_A))
    want = _model_counts(vt, m, lambda words: pycodec.unpack(PM, words), wr.SET_A, wr.bits_of, sr.SET_A, sr.bits_of, 100, max_depth, 11, 64)
    r = m.simulate_where(state=ws, step=wp, stop=False, n_walkers=100, max_depth=max_depth, seed=11, max_rounds=1)
    _assert_report_equals_model(r, want, wr.SET_A, sr.SET_A, 100)
    assert sum(want["cs"]) > 0 and sum(want["cp"]) > 0
    if (R, n) == (2, 1):
        assert want["mixed"] > 0
    # each program alone (the instantiations with the other one compiled out) counts the same
    r1 = m.simulate_where(state=ws, stop=False, n_walkers=100, max_depth=max_depth, seed=11, max_rounds=1)
    r2 = m.simulate_where(step=wp, stop=False, n_walkers=100, max_depth=max_depth, seed=11, max_rounds=1)
    assert r1["count_state"] == r["count_state"] and (r1["n_states"], r1["n_pairs"], r1["steps"], r1["walks"]) == (6400, 0, r["steps"], r["walks"])
    assert r2["count_step"] == r["count_step"] and (r2["n_states"], r2["n_pairs"], r2["steps"], r2["walks"]) == (0, r["steps"], r["steps"], r["walks"])
    if R >= 4:
        ws4, wp4 = m.compile_predicates(dp.text_of(dp.STATE)), m.compile_step_predicates(dp.text_of(dp.STEP))
        want4 = _model_counts(vt, m, lambda words: pycodec.unpack(PM, words), dp.STATE, wr.bits_of, dp.STEP, sr.bits_of, 100, max_depth, 11, 64)
        r4 = m.simulate_where(state=ws4, step=wp4, stop=False, n_walkers=100, max_depth=max_depth, seed=11, max_rounds=1)
        _assert_report_equals_model(r4, want4, dp.STATE, dp.STEP, 100)
        assert (want4["steps"], want4["walks"]) == (want["steps"], want["walks"]) and want["walks"] > 100      # the same walks; walkers start again at max_depth
        held = want4["cs"][[p[0] for p in dp.STATE].index(dp.SIM_STATE_MUST_HIT)]
        grew = want4["cp"][[p[0] for p in dp.STEP].index(dp.SIM_STEP_MUST_HIT)]
        print("simulate_where (%d,%d,%d,%d): n_walkers 100, max_depth %d, seed 11, max_rounds 1; the model stands on %d states in which a DoViewChange is held "
              "and takes %d pairs on which the held set grew" % (R, C, n, L, max_depth, held, grew))
        assert held >= 1 and grew >= 1                                 # by the Python model, which does not run the kernel under test
    if C == 2:
        ws2, wp2 = m.compile_predicates(dp.text_of(dp.STATE_C2)), m.compile_step_predicates(dp.text_of(dp.STEP_C2))
        want2 = _model_counts(vt, m, lambda words: pycodec.unpack(PM, words), dp.STATE_C2, wr.bits_of, dp.STEP_C2, sr.bits_of, 100, max_depth, 11, 64)
        r2c = m.simulate_where(state=ws2, step=wp2, stop=False, n_walkers=100, max_depth=max_depth, seed=11, max_rounds=1)
        _assert_report_equals_model(r2c, want2, dp.STATE_C2, dp.STEP_C2, 100)
        assert (want2["steps"], want2["walks"]) == (want["steps"], want["walks"]) and want["walks"] > 100
        pending = want2["cs"][[p[0] for p in dp.STATE_C2].index(dp.SIM_C2_STATE_MUST_HIT)]
        appended = want2["cp"][[p[0] for p in dp.STEP_C2].index(dp.SIM_C2_STEP_MUST_HIT)]
        print("simulate_where (%d,%d,%d,%d): the model stands on %d states in which a request of client 2 is pending and takes %d pairs that append an entry of "
              "client 2" % (R, C, n, L, pending, appended))
        rewritten = [want2["cp"][[p[0] for p in dp.STEP_C2].index(nm)] for nm in ("Row2RewrittenByClient1", "Row1RewrittenByClient2")]
        print("... and %d + %d pairs on which ReceivePrepareMsg rewrites the row of the client whose entry it did not append" % tuple(rewritten))
        assert pending >= 1 and appended >= 1 and min(rewritten) >= 1  # by the Python model, which does not run the kernel under test


# ---------------------------------------------------------------------------------------------------------------------
# 2. identities and determinism
# ---------------------------------------------------------------------------------------------------------------------
IDENTITIES = r"""T == TRUE
P == \E r \in replicas : rep_status[r] # Normal
Q == \E m \in DOMAIN messages : messages[m] >= 1
NotP == ~P
PorQ == P \/ Q
PandQ == P /\ Q
"""
ID_KW = dict(n_walkers=4096, max_depth=40, max_rounds=2)


@pytest.fixture(scope="module")
def identity_run(vt):
    m = vt.Model.from_constants(R=2, C_=1, n=2, L=2)                # 2 073 states with terminal ones among them: the walks of a seed end at their own times
    return m, m.simulate_where(state=m.compile_predicates(IDENTITIES), stop=False, seed=5, **ID_KW)


def test_identities_and_determinism(vt, identity_run):
    m, r = identity_run
    c = r["count_state"]
    print("identities: %s of %d states" % (c, r["n_states"]))
    assert r["found"] == 0 and r["rounds"] == 2
    assert c["T"] == r["n_states"] == 64 * 2 * 4096 == r["steps"] + r["walks"]
    assert c["P"] + c["NotP"] == r["n_states"]
    assert c["PorQ"] + c["PandQ"] == c["P"] + c["Q"]
    assert 0 < c["P"] < r["n_states"] and 0 < c["Q"] < r["n_states"] and 0 < c["PandQ"] < c["PorQ"]
    w = m.compile_predicates(IDENTITIES)
    again = m.simulate_where(state=w, stop=False, seed=5, **ID_KW)
    strip = lambda d: {k: v for k, v in d.items() if k != "seconds"}   # noqa: E731
    assert strip(again) == strip(r)
    other = m.simulate_where(state=w, stop=False, seed=6, **ID_KW)
    assert other["steps"] != r["steps"] and other["n_states"] == r["n_states"]
    # the same over pairs
    p = m.simulate_where(step=m.compile_step_predicates("T == TRUE\nV == " + sr.VIEW_MONOTONIC + "\nNotV == ~V"), stop=False, seed=5, **ID_KW)
    assert p["steps"] == r["steps"] and p["count_step"]["T"] == p["n_pairs"] == p["steps"]
    assert p["count_step"]["V"] + p["count_step"]["NotV"] == p["n_pairs"]


# ---------------------------------------------------------------------------------------------------------------------
# 3. -reach by simulation
# ---------------------------------------------------------------------------------------------------------------------
def test_reach_log_divergence(vt, orc):
    """(3,1,2,1): the BFS meets the first LogDivergence state at level 10, so no walk can get there in fewer than nine steps"""
    from oracle import pycodec, pyoracle as po
    m = vt.Model.from_constants(R=3, C_=1, n=2, L=1)
    PM = po.Model(3, 1, ("v1", "v2"), 1)
    text = open(os.path.join(TOOLS, "predicates_example.txt")).read()
    r = m.simulate_where(state=m.compile_predicates(_query(text, "LogDivergence")), stop=True, n_walkers=1 << 14, max_depth=40, seed=3, max_seconds=20.0)
    print("reach LogDivergence by simulation: found %d after %.3f s, %d rounds, %d steps; the walk has %d states" %
          (r["found"], r["seconds"], r["rounds"], r["steps"], len(r["trace"] or [])))
    assert r["found"] == 3 and r["hit"] == ["Query0"] and r["viol_mask"] == 1
    tr = r["trace"]
    assert len(tr) == r["viol_steps"] + 1 >= 10
    _check_walk_with_oracle(orc, orc.Params(3, 1, 2, 1), tr)
    verdicts = [wr.log_divergence(pycodec.unpack(PM, [int(x) for x in rec])) for _, rec in tr]
    assert verdicts == [False] * (len(tr) - 1) + [True]


def test_reach_unsettled(vt, orc):
    """a certain case: 1 444 of the 2 073 states of (2,1,2,2) are unsettled, from level 2 on"""
    from oracle import pycodec, pyoracle as po
    m = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
    PM = po.Model(2, 1, ("v1", "v2"), 2)
    r = m.simulate_where(state=m.compile_predicates("Unsettled == " + wr.SET_A[4][1]), stop=True, n_walkers=256, max_depth=40, seed=3, max_seconds=20.0)
    assert r["found"] == 3 and r["hit"] == ["Unsettled"] and r["rounds"] == 1
    tr = r["trace"]
    assert len(tr) == r["viol_steps"] + 1 >= 2
    _check_walk_with_oracle(orc, orc.Params(2, 1, 2, 2), tr)
    assert [wr.unsettled(pycodec.unpack(PM, [int(x) for x in rec])) for _, rec in tr] == [False] * (len(tr) - 1) + [True]
    # Init itself: found 3 with no step at all
    r0 = m.simulate_where(state=m.compile_predicates("T == TRUE"), stop=True, n_walkers=64, max_depth=40, seed=3, max_seconds=20.0)
    assert (r0["found"], r0["viol_steps"], r0["ordinals"]) == (3, 0, []) and len(r0["trace"]) == 1


# ---------------------------------------------------------------------------------------------------------------------
# 4. -stepInvariant by simulation
# ---------------------------------------------------------------------------------------------------------------------
def test_step_invariant_commit_monotonic(vt, orc):
    """(3,1,1,1): every pair of that space on which CommitMonotonic is false is a ReceiveSV"""
    from oracle import pycodec, pyoracle as po
    m = vt.Model.from_constants(R=3, C_=1, n=1, L=1)
    PM = po.Model(3, 1, ("v1",), 1)
    text = open(os.path.join(TOOLS, "steps_example.txt")).read()
    r = m.simulate_where(step=m.compile_step_predicates(_query(text, "CommitMonotonic", negate=True)), stop=True, n_walkers=1 << 14, max_depth=40, seed=3,
                         max_seconds=20.0)
    print("stepInvariant CommitMonotonic by simulation: found %d after %.3f s, %d rounds; the walk has %d states" %
          (r["found"], r["seconds"], r["rounds"], len(r["trace"] or [])))
    assert r["found"] == 4 and r["hit"] == ["Query0"]
    tr = r["trace"]
    assert len(tr) == r["viol_steps"] + 1 >= 2 and tr[-1][0] == "ReceiveSV"
    _check_walk_with_oracle(orc, orc.Params(3, 1, 1, 1), tr)
    views = [pycodec.unpack(PM, [int(x) for x in rec]) for _, rec in tr]
    verdicts = [sr.commit_monotonic(views[t], views[t + 1], tr[t + 1][0]) for t in range(len(tr) - 1)]
    assert verdicts == [True] * (len(tr) - 2) + [False]


# ---------------------------------------------------------------------------------------------------------------------
# 5. never true
# ---------------------------------------------------------------------------------------------------------------------
def test_a_predicate_that_never_holds_stops_nothing(vt):
    """(2,1,2,2) is exhausted at 2 073 states without one LogDivergence state"""
    m = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
    r = m.simulate_where(state=m.compile_predicates("LogDivergence == " + wr.LOG_DIVERGENCE), stop=True, n_walkers=4096, max_depth=40, seed=3, max_rounds=4)
    assert (r["found"], r["rounds"], r["count_state"]["LogDivergence"], r["trace"]) == (0, 4, 0, None)
    assert r["n_states"] == 64 * 4 * 4096
    both = m.compile_predicates("LogDivergence == " + wr.LOG_DIVERGENCE + "\nStaleStartView == " + wr.SET_A[0][1])
    r = m.simulate_where(state=both, stop=False, n_walkers=4096, max_depth=40, seed=3, max_rounds=4)
    assert r["found"] == 0 and r["count_state"]["LogDivergence"] == 0 and r["count_state"]["StaleStartView"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. the analysis models
# ---------------------------------------------------------------------------------------------------------------------
def test_model2_reach_in_state_transfer(vt):
    from oracle import orc2, pyoracle2
    m = vt.Model.second_model(R=3, n=2, L=1)
    PM = pyoracle2.Model(3, ("v1", "v2"), 1)
    text = open(os.path.join(TOOLS, "predicates_model2_example.txt")).read()
    r = m.simulate_where(state=m.compile_predicates(_query(text, "InStateTransfer")), stop=True, n_walkers=1 << 14, max_depth=40, seed=3, max_seconds=20.0)
    print("model 2, reach InStateTransfer by simulation: found %d after %.3f s, %d rounds; the walk has %d states" %
          (r["found"], r["seconds"], r["rounds"], len(r["trace"] or [])))
    assert r["found"] == 3 and r["hit"] == ["Query0"]
    tr = r["trace"]
    _check_walk_with_oracle(orc2, orc2.Params(3, 2, 1), tr)
    assert [wm.in_state_transfer(pyoracle2.unpack(PM, [int(x) for x in rec])) for _, rec in tr] == [False] * (len(tr) - 1) + [True]


def test_model3_report_counts_equal_the_model(vt):
    from oracle import pyoracle3
    m = vt.Model.third_model(R=3, n=2, L=1)
    PM = pyoracle3.Model(3, ("a", "b"), 1)
    state_preds = wm.set_a(("a", "b"))[:5] + wm.SET_A3
    step_preds = smr.SET_A["third"]
    assert len(state_preds) == 8 and len(step_preds) == 8
    ws, wp = m.compile_predicates(wm.text_of(state_preds)), m.compile_step_predicates(smr.text_of(step_preds))
    want = _model_counts(vt, m, lambda words: pyoracle3.unpack(PM, words), state_preds, wm.bits_of, step_preds, smr.bits_of, 100, 16, 11, 64)
    r = m.simulate_where(state=ws, step=wp, stop=False, n_walkers=100, max_depth=16, seed=11, max_rounds=1)
    _assert_report_equals_model(r, want, state_preds, step_preds, 100)
    assert sum(want["cs"]) > 0 and sum(want["cp"]) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. the command line
# ---------------------------------------------------------------------------------------------------------------------
def _cli(args):
    return subprocess.run([CLI] + args + ["-noTLA"], capture_output=True, text=True, timeout=300)


def test_cli_reach_and_step_invariant_on_the_readme_configuration(vt, tmp_path):
    from test_host_cpu import _cfg
    cfg = _cfg(tmp_path, R=3, vals="v1, v2, v3", L=3)
    sim = ["-config", cfg, "-simulate", "-depth", "60", "-walkers", "16384", "-seed", "2", "-maxSeconds", "30"]
    r = _cli(sim + ["-predicates", os.path.join(TOOLS, "predicates_example.txt"), "-reach", "LogDivergence"])
    print("cli -reach LogDivergence: " + r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr)
    assert "State satisfying LogDivergence found at depth" in r.stdout and "\nThe behavior up to this point is:\n" in r.stdout and "Error:" not in r.stdout
    assert "State 1: <Initial predicate>" in r.stdout
    r = _cli(sim + ["-predicates", os.path.join(TOOLS, "predicates_example.txt"), "-invariant", "AckedWriteOnMajority"])
    print("cli -invariant AckedWriteOnMajority: " + r.stdout.strip().splitlines()[-1])
    assert r.returncode == 12 and "Error: Invariant AckedWriteOnMajority is violated." in r.stdout and "Error: The behavior up to this point is:" in r.stdout
    r = _cli(sim + ["-steps", os.path.join(TOOLS, "steps_example.txt"), "-stepInvariant", "CommittedPrefixStable"])
    print("cli -stepInvariant CommittedPrefixStable: " + r.stdout.strip().splitlines()[-1])
    assert r.returncode == 12, (r.stdout[-2000:], r.stderr)
    assert "Error: Action property CommittedPrefixStable is violated." in r.stdout and "Error: The behavior up to this point is:" in r.stdout
    last = re.findall(r"State (\d+): <(\w+)>", r.stdout)[-1]
    m = re.search(r"The last step is (\w+) of State (\d+)\.", r.stdout)
    assert m and m.group(1) == last[1] and int(m.group(2)) == int(last[0]) - 1


def test_cli_report_prints_the_counts_of_the_api(vt, tmp_path, identity_run):
    from test_host_cpu import _cfg
    _m, want = identity_run
    cfg = _cfg(tmp_path, R=2, vals="v1, v2", L=2)
    preds = tmp_path / "identities.txt"
    preds.write_text(IDENTITIES)
    r = _cli(["-config", cfg, "-simulate", "-simRounds", "2", "-whereReport", "-predicates", str(preds), "-walkers", "4096", "-depth", "40", "-seed", "5"])
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = {nm: (int(a), int(b)) for nm, a, b in re.findall(r"Where report: (\w+) holds in (\d+) of (\d+) states", r.stdout)}
    assert got == {nm: (cnt, want["n_states"]) for nm, cnt in want["count_state"].items()}


# ---------------------------------------------------------------------------------------------------------------------
# 8. the old entry point
# ---------------------------------------------------------------------------------------------------------------------
def test_simulate_is_what_it_was(vt, orc):
    m = vt.Model.from_constants(R=3, C_=1, n=3, L=3)
    r = m.simulate(n_walkers=1 << 17, max_depth=60, seed=2, max_seconds=40.0)
    assert r["found"] == 1 and r["viol_mask"] == 1 and sorted(r) == ["found", "ordinals", "seconds", "steps", "trace", "viol_mask", "walks"]
    _check_walk_with_oracle(orc, orc.Params(3, 1, 3, 3), r["trace"])
    assert [orc.invariants(orc.Params(3, 1, 3, 3), rec) for _, rec in r["trace"]] == [0] * (len(r["trace"]) - 1) + [1]
    m = vt.Model.from_constants(R=2, C_=1, n=1, L=1)
    r = m.simulate(n_walkers=4096, max_depth=30, seed=1, max_seconds=1.0)
    assert r["found"] == 0 and r["steps"] > 0 and r["walks"] > 0 and r["trace"] is None
