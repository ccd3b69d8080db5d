"""Random walks under constraints, host side (`-m "not gpu"`): every refusal of vsrmc_simulate_constrained comes before a device is looked at — the
calls run in a process that sees no device at all — as does the result for an Init that fails the state constraint, which the host evaluates itself;
the command line's usage errors for -walkConstraint / -walkActionConstraint; the header, the binding and the library agree; the Python model of the
contract (tests/sim_constrained_model.py) on a scripted successor table.  What the walks compute is checked on the GPU (test_sim_constrained_gpu.py)."""
import ctypes as C
import os
import subprocess

import pytest

import action_constraint_reference as ar
import constraint_reference as cr
import sim_constrained_model as scm
import sim_where_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
TOOLS = os.path.join(ROOT, "tools")
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


# ---- the API: one child process without a device runs every refused call and prints what it got ---------------------------------------------------
REFUSALS = r'''
import vsr_tlaplus_amd as vt
m = vt.Model.from_constants(R=3, C_=1, n=2, L=2)
other = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
third = vt.Model.third_model(R=3, n=2, L=2)
S = m.compile_predicates("T == TRUE\nQ == rep_status[3] = Normal")
P = m.compile_step_predicates("T == TRUE\nQ == aux_svc' = aux_svc")
AUX_S = m.compile_predicates("A == aux_svc < 2")
AUX_P = m.compile_step_predicates("A == \\A v \\in Values : v \\in DOMAIN aux_client_acked' => v \\in DOMAIN aux_client_acked")
AUX_Q = m.compile_predicates("A == aux_svc < 2\nT == TRUE")
calls = [
    ("neither", dict()),
    ("neither", dict(state=S, step=P)),
    ("no-program", dict(constraint=0)),
    ("index", dict(state=S, constraint=2)),
    ("index", dict(state=S, constraint=-2)),
    ("index", dict(step=P, action_constraint=5)),
    ("kind", dict(state=P, constraint=0)),
    ("kind", dict(step=S, action_constraint=0)),
    ("model", dict(state=other.compile_predicates("T == TRUE"), constraint=0)),
    ("model", dict(state=third.compile_predicates("T == TRUE"), constraint=0)),
    ("model", dict(state=S, constraint=0, step=other.compile_step_predicates("T == TRUE"))),
    ("aux", dict(state=AUX_S, constraint=0)),
    ("aux", dict(step=AUX_P, action_constraint=0)),
    ("aux", dict(state=AUX_Q, constraint="T")),
    ("depth", dict(state=S, constraint=0, max_depth=0)),
    ("depth", dict(state=S, constraint=0, max_depth=513)),
    ("walkers", dict(state=S, constraint=0, n_walkers=0)),
]
for tag, kw in calls:
    try:
        if tag == "no-program":
            import ctypes
            from vsr_tlaplus_amd import capi
            r = capi.SimConstrainedResult()
            capi.check(capi.load().vsrmc_simulate_constrained(m._h, 0, None, 0, None, -1, 0, 0, 64, 10, 1, 1.0, 1, ctypes.byref(r)))
        else:
            m.simulate_constrained(max_rounds=1, **kw)
        print(tag, "ACCEPTED")
    except vt.VsrmcError as e:
        print(tag, e.code, e.message)
# Init out of the model: evaluated on the host, nothing launched, no device looked at
N = m.compile_predicates(r"InitOnly == (\A m \in DOMAIN messages : FALSE) /\ (\A r \in replicas : rep_view_number[r] = 1)" + "\nNotInit == ~InitOnly\nT == TRUE")
r = m.simulate_constrained(state=N, constraint="NotInit", max_rounds=3, n_walkers=100, max_depth=12)
print("init", r["init_pruned"], r["found"], r["walks"], r["steps"], r["rounds"], r["n_states"], r["pruned"], r["blocked"], r["stuck"], r["trace"])
for which, mm in (("second", vt.Model.second_model(R=3, n=2, L=1)), ("third", third)):
    r = mm.simulate_constrained(state=mm.compile_predicates("F == FALSE"), constraint=0, max_rounds=1)
    print("init-" + which, r["init_pruned"], r["found"], r["walks"])
'''


@pytest.fixture(scope="module")
def refusal_lines(vt):
    env = dict(os.environ, PYTHONPATH=ROOT, **NO_DEVICE)
    r = subprocess.run(["python3", "-c", REFUSALS], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    return [ln.split(" ", 2) for ln in r.stdout.strip().splitlines()]


@pytest.mark.parametrize("tag, needle", [
    ("neither", "neither a state constraint nor an action constraint"),
    ("no-program", "exports no predicate of index state_constraint"),
    ("index", "exports no predicate of index"),
    ("kind", "program"),
    ("model", "compiled for another model"),
    ("aux", "aux_svc or aux_client_acked"),
    ("depth", "max_depth outside 1..512"),
    ("walkers", "no walkers"),
])
def test_refusals_come_before_any_device_call(refusal_lines, tag, needle):
    """VSRMC_E_ARG with the message of the refusal, not VSRMC_E_HIP: the process has no device"""
    mine = [ln for ln in refusal_lines if ln[0] == tag]
    assert mine, refusal_lines
    for ln in mine:
        assert ln[1] == "-1" and needle in ln[2], ln


def test_a_constraint_of_the_wrong_kind_names_the_kind(refusal_lines):
    kinds = [ln[2] for ln in refusal_lines if ln[0] == "kind"]
    assert len(kinds) == 2 and "a step program" in kinds[0] and "was given as the state program" in kinds[0]
    assert "a state program" in kinds[1] and "was given as the step program" in kinds[1]


def test_an_aux_reading_query_beside_a_clean_constraint_is_still_refused(refusal_lines):
    """the rule of the attach calls: it is the PROGRAM that must not read the aux variables (the op codes show it), three programs here"""
    assert len([ln for ln in refusal_lines if ln[0] == "aux"]) == 3


def test_init_out_of_the_model_is_a_result_not_an_error(refusal_lines):
    init = [ln for ln in refusal_lines if ln[0] == "init"]
    assert len(init) == 1
    assert (init[0][1] + " " + init[0][2]).split() == ["True", "0", "0", "0", "0", "0", "0", "0", "0", "None"]
    for which in ("second", "third"):
        ln = [x for x in refusal_lines if x[0] == "init-" + which]
        assert len(ln) == 1 and (ln[0][1] + " " + ln[0][2]).split() == ["True", "0", "0"], ln


# ---- header, binding, library ----------------------------------------------------------------------------------------------------------------------
def test_the_result_struct_has_the_layout_of_the_header(vt):
    from vsr_tlaplus_amd import capi
    r, w = capi.SimConstrainedResult, capi.SimWhereResult
    for name, _ in w._fields_:
        assert getattr(r, name).offset == getattr(w, name).offset, name
    assert (r.blocked.offset, r.pruned.offset, r.stuck.offset, r.init_pruned.offset) == (2240, 2248, 2256, 2264) and C.sizeof(r) == 2272
    hdr = open(os.path.join(ROOT, "include", "vsrmc.h")).read()
    assert "#define VSRMC_SIM_ERR_TRIED_WIDTH 40" in hdr and "vsrmc_simulate_constrained(" in hdr and "[TLC-RECALLED]" in hdr.split("k_simulate_constrained")[1][:400]
    assert hasattr(C.CDLL(capi.LIB_PATH), "vsrmc_simulate_constrained")


# ---- the command line, as far as it gets without a device -----------------------------------------------------------------------------------------
def _cli(args):
    return subprocess.run([CLI] + args + ["-noTLA"], capture_output=True, text=True, timeout=120, env=dict(os.environ, **NO_DEVICE))


@pytest.fixture()
def cfg(vt, tmp_path):
    from test_host_cpu import _cfg
    return _cfg(tmp_path, R=3, vals="v1, v2", L=1)


CON, ACT = os.path.join(TOOLS, "constraints_example.txt"), os.path.join(TOOLS, "action_constraints_example.txt")


@pytest.mark.parametrize("flags, needle", [
    (["-predicates", CON, "-walkConstraint", "Replica3Normal"], "belong to -simulate"),
    (["-steps", ACT, "-walkActionConstraint", "QuietClient"], "belong to -simulate"),
    (["-simulate", "-walkConstraint", "Replica3Normal"], "-walkConstraint NAME needs -predicates FILE"),
    (["-simulate", "-walkActionConstraint", "QuietClient"], "-walkActionConstraint NAME needs -steps FILE"),
    (["-simulate", "-predicates", CON, "-walkConstraint", ""], "-walkConstraint needs a NAME"),
    (["-simulate", "-steps", ACT, "-walkActionConstraint", ""], "-walkActionConstraint needs a NAME"),
    (["-simulate", "-predicates", CON, "-walkConstraint", "NoSuchName"], "exports no predicate NoSuchName"),
    (["-simulate", "-steps", ACT, "-walkActionConstraint", "NoSuchName"], "exports no predicate NoSuchName"),
    (["-simulate", "-predicates", CON, "-walkConstraint", "Replica3Normal", "-json"], "cannot be combined with -json"),
])
def test_cli_usage_errors(cfg, flags, needle):
    r = _cli(["-config", cfg] + flags)
    assert r.returncode == 2 and needle in r.stderr and "Running Random Simulation" not in r.stdout, (r.stdout, r.stderr)


def test_cli_refuses_an_aux_reading_constraint_without_a_device(cfg, tmp_path):
    p = tmp_path / "aux.txt"
    p.write_text("FewRounds == aux_svc < 2\n")
    r = _cli(["-config", cfg, "-simulate", "-simRounds", "1", "-predicates", str(p), "-walkConstraint", "FewRounds"])
    assert r.returncode == 1 and "aux_svc or aux_client_acked" in r.stderr, (r.stdout, r.stderr)
    s = tmp_path / "auxstep.txt"
    s.write_text("SvcKept == UNCHANGED aux_svc\n")
    r = _cli(["-config", cfg, "-simulate", "-simRounds", "1", "-steps", str(s), "-walkActionConstraint", "SvcKept", "-stepReport"])
    assert r.returncode == 1 and "aux_svc or aux_client_acked" in r.stderr, (r.stdout, r.stderr)


def test_cli_init_out_of_the_model_needs_no_device(cfg, tmp_path):
    p = tmp_path / "notinit.txt"
    p.write_text(cr.TEXTS["InitOnly"] + "\nNotInit == ~InitOnly\n")
    r = _cli(["-config", cfg, "-simulate", "-simRounds", "1", "-predicates", str(p), "-walkConstraint", "NotInit"])
    assert r.returncode == 0 and "The initial state fails the constraint NotInit" in r.stdout and "0 tries blocked" in r.stdout, (r.stdout, r.stderr)


def test_cli_keeps_the_old_refusals_and_points_to_the_new_flags(cfg):
    r = _cli(["-config", cfg, "-simulate", "-predicates", CON, "-constraint", "Replica3Normal"])
    assert r.returncode == 2 and "a random walk (-simulate) is not constrained: use -walkConstraint NAME" in r.stderr
    r = _cli(["-config", cfg, "-simulate", "-steps", ACT, "-actionConstraint", "QuietClient"])
    assert r.returncode == 2 and "a random walk (-simulate) is not constrained: use -walkActionConstraint NAME" in r.stderr
    h = subprocess.run([CLI, "-help"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and "-walkConstraint NAME" in h.stdout and "-walkActionConstraint NAME" in h.stdout


# ---- the model helper on a scripted successor table -----------------------------------------------------------------------------------------------
class _Scripted(scm.ConstrainedWalkers):
    """the successor rows come from a table instead of Model.get_next_states: keys are one-word tuples"""

    def __init__(self, table, init, n_walkers, max_depth, seed, **kw):
        self.m, self.n, self.max_depth, self.device = None, n_walkers, max_depth, 0
        self.rng = sm.splitmix64_stream(seed, n_walkers)
        self.init = init
        self.cur, self.depth, self.ords = [None] * n_walkers, [0] * n_walkers, [[] for _ in range(n_walkers)]
        self.rows = dict(table)
        self.steps = self.walks = 0
        self.state_ok, self.step_ok = kw.get("state_ok"), kw.get("step_ok")
        self.tried = [set() for _ in range(n_walkers)]
        self.blocked = self.pruned = self.stuck = self.max_enabled = 0

    def _expand(self, keys):
        pass


def test_model_outcomes_on_a_scripted_table():
    """a: three instances into b, c, d; b, c, d: one instance back into a.  Action constraint: never into b; state constraint: d is out of the model.  From a the
    only acceptable successor is c, and it is reached within three tries whatever is drawn; never twice the same refused instance"""
    a, b, c, d = (0,), (1,), (2,), (3,)
    table = {a: [(0, 5, b), (1, 6, c), (2, 7, d)], b: [(0, 8, a)], c: [(0, 8, a)], d: [(0, 8, a)]}
    W = _Scripted(table, a, 50, 1000, 7, state_ok=lambda k: k != d, step_ok=lambda p, ch, act: ch != b)
    per_walker = [[] for _ in range(50)]
    for events in W.iterate(200):
        for i, ev in enumerate(events):
            per_walker[i].append(ev)
    assert W.steps + W.walks + W.blocked + W.pruned == 200 * 50 and W.walks == 50 and W.stuck == 0 and W.max_enabled == 3
    assert W.blocked > 100 and W.pruned > 100
    for evs in per_walker:
        assert evs[0] == ("start", a)
        refused = []
        for ev in evs[1:]:
            if ev[0] == "step":
                assert ev[2] in (c, a) and len(refused) <= 2
                refused = []
            else:
                assert (ev[0], ev[2]) in (("blocked", b), ("pruned", d)) and ev[2] not in refused
                refused.append(ev[2])
    # the first draw of walker 0 by hand: seed 7 -> splitmix64 -> xorshift64*; three untried instances, pick = draw % 3
    x = sm.splitmix64_stream(7, 1)[0]
    _x, draw = sm.xorshift64star(x)
    assert per_walker[0][1][4] == draw % 3
    # everything refused: every walk is start, one refusal per instance, then stuck
    W = _Scripted(table, a, 10, 1000, 7, step_ok=ar.never)
    n = sum(len(events) for events in W.iterate(4 * 7 + 2))
    assert n == 300 and (W.steps, W.pruned) == (0, 0) and W.walks == 10 * 8 and W.stuck == 10 * 7 and W.blocked == 10 * (3 * 7 + 1)
