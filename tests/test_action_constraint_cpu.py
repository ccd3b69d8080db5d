"""Action constraints, the part that needs no device (`-m "not gpu"`): the reference itself (tests/action_constraint_reference.py) — a TRUE constraint is
the plain search, a predicate of the successor alone keeps what the state constraint of the same text keeps, floors on the blocked / rescued counts of
the spaces the GPU tests use so that an empty case cannot pass there; the CLI's usage errors, refused before any device call; the example files compile
for their models and what the compiler refuses; the header, the binding and the library agree."""
import ctypes as C
import os
import re
import subprocess

import pytest

import action_constraint_reference as ar
import constraint_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
SYMBOLS = ["vsrmc_checker_action_constrain_attach", "vsrmc_checker_action_constraint_info", "vsrmc_checker_seen_set_load"]


@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------
def test_reference_true_is_the_plain_search(vt):
    t = ar.constrained_bfs("first", 2, 1, 2, 2, ar.always)
    plain = cr.constrained_bfs("first", 2, 1, 2, 2, lambda s: True, with_unconstrained=False)
    assert t.blocked == 0 and t.rescued == 0 and t.states == plain.in_model >= 1000 and t.depth == plain.depth
    for a, b in zip(t.levels, plain.levels):
        assert set(a.new) == set(b.kept) and a.generated == b.generated, a.level
    assert not t.levels[-1].new and len(t.levels) == len(plain.levels) + 1                # (this reference records the last, empty step as well)
    assert all(sum(lv.act_generated.values()) == lv.generated for lv in t.levels)


def test_reference_primed_only_predicate_equals_the_state_constraint(vt):
    """NarrowNetwork with every variable primed, as an action constraint, against the state constraint of the same text: the same kept sets from level 2 on
    (Init satisfies it, so from level 1 on here)"""
    a = ar.constrained_bfs("first", 2, 1, 2, 2, ar.primed(cr.narrow_network))
    s = cr.constrained_bfs("first", 2, 1, 2, 2, cr.narrow_network, with_unconstrained=False)
    assert a.states == s.in_model >= 100 and a.blocked >= 20
    for la, ls in zip(a.levels, s.levels):
        assert set(la.new) == set(ls.kept), la.level
    assert a.rescued == 0                                                                  # (a blocked target fails the predicate by every edge)


def test_reference_quiet_client_bites(vt):
    r = ar.constrained_bfs("first", 2, 1, 2, 2, ar.quiet_client)
    plain = ar.constrained_bfs("first", 2, 1, 2, 2, ar.always)
    print("(2,1,{v1,v2},2) QuietClient: %d of %d states, %d generated, %d blocked, depth %d, %d rescued, %.2f s"
          % (r.states, plain.states, r.generated, r.blocked, r.depth, r.rescued, r.seconds))
    assert r.states < plain.states and r.blocked >= 50 and r.rescued >= 5 and r.depth >= 20
    assert all(set(lv.blocked_act) <= {"ReceiveClientRequest"} for lv in r.levels)
    # a rescued state is in the model although an edge into it was blocked; a per-state filter would have lost it
    assert all(set(lv.rescued) <= set(lv.new) for lv in r.levels)
    reached = set(fp for lv in r.levels for fp in lv.new)
    assert reached <= set(fp for lv in plain.levels for fp in lv.new)
    r2 = ar.constrained_bfs("first", 3, 1, 2, 1, ar.quiet_client, max_levels=11)
    print("(3,1,{v1,v2},1) QuietClient, 11 levels: %d states, %d blocked, %d rescued, largest level %d, %.2f s"
          % (r2.states, r2.blocked, r2.rescued, max(len(lv.new) for lv in r2.levels), r2.seconds))
    assert r2.blocked >= 100 and r2.rescued >= 10 and max(len(lv.new) for lv in r2.levels) > 256   # more than one block of k_step_expand
    assert r2.seconds < 20.0


def test_reference_false_and_timers(vt):
    f = ar.constrained_bfs("first", 2, 1, 2, 2, ar.never)
    assert f.states == 1 and len(f.levels) == 2 and f.levels[1].blocked == f.levels[1].generated > 0
    t = ar.constrained_bfs("first", 2, 1, 2, 2, ar.timers_in_view_1)
    assert 50 <= t.states < 1000 and t.blocked > 0 and all(set(lv.blocked_act) <= {"TimerSendSVC"} for lv in t.levels)


def test_reference_with_a_state_constraint_as_well(vt):
    r = ar.constrained_bfs("first", 3, 1, 2, 1, ar.quiet_client, max_levels=11, state_constraint=cr.replica3_normal)
    assert r.blocked > 0 and sum(len(lv.pruned) for lv in r.levels) > 0 and r.states >= 100
    assert all(not (set(lv.new) & set(lv.pruned)) for lv in r.levels)


# ---- the CLI's refusals, before any device call ---------------------------------------------------------------------------------------------------
def test_cli_refusals_before_any_device_call(vt, tmp_path):
    from test_host_cpu import _cfg
    cfg = _cfg(tmp_path, R=2, vals="v1, v2", L=2)
    steps = os.path.join(ROOT, "tools", "action_constraints_example.txt")
    preds = os.path.join(ROOT, "tools", "predicates_example.txt")
    base = [CLI, "-config", cfg, "-noTLA", "-steps", steps, "-actionConstraint", "QuietClient"]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")          # a device call would fail differently: the refusals come first
    for extra, needle in ((["-gpus", "2"], "-actionConstraint runs on one GPU"),
                          (["-simulate"], "a random walk (-simulate) is not constrained"),
                          (["-deepPredicates", "-predicates", preds, "-whereReport"], "cannot be combined with -deepPredicates"),
                          (["-probeLast"], "cannot be combined with -probeLast / -probe2At / -probe3At"),
                          (["-probe2At", "5"], "cannot be combined with -probeLast / -probe2At / -probe3At"),
                          (["-probe3At", "5"], "cannot be combined with -probeLast / -probe2At / -probe3At"),
                          (["-checkpoint", str(tmp_path / "chk")], "cannot be combined with -checkpoint / -recover"),
                          (["-recover", str(tmp_path / "chk")], "cannot be combined with -checkpoint / -recover"),
                          (["-audit"], "cannot be combined with -audit")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 2 and ("Error: " in r.stderr and needle in r.stderr), (extra, r.returncode, r.stderr, r.stdout[-300:])
    r = subprocess.run([CLI, "-config", cfg, "-noTLA", "-actionConstraint", "QuietClient"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 2 and "-actionConstraint NAME needs -steps FILE" in r.stderr
    r = subprocess.run(base[:-1] + ["NoSuchName"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 2 and "exports no predicate NoSuchName" in r.stderr
    # an ACTION_CONSTRAINT section in a cfg stays refused
    bad = tmp_path / "b"
    bad.mkdir()
    cfg2 = _cfg(bad, R=2, vals="v1, v2", L=2, extra="ACTION_CONSTRAINT QuietClient")
    r = subprocess.run([CLI, "-config", cfg2, "-noTLA"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "ACTION_CONSTRAINT" in (r.stderr + r.stdout)
    assert "-actionConstraint NAME" in subprocess.run([CLI, "-help"], capture_output=True, text=True, timeout=60).stdout


# ---- what compiles and what does not ----------------------------------------------------------------------------------------------------------------
def test_examples_compile_and_compile_time_refusals(vt):
    m = vt.Model.from_constants(R=3, C_=1, n=2, L=2)
    w = m.compile_step_predicates(open(os.path.join(ROOT, "tools", "action_constraints_example.txt")).read())
    assert w.names == ["QuietClient", "CommitNeverDecreases", "TimersInView1"] and w.describe()["step"] == 1
    for k, text in ar.TEXTS.items():
        assert m.compile_step_predicates(text).names == [k]
    models_text = open(os.path.join(ROOT, "tools", "action_constraints_models_example.txt")).read()
    for mk in (vt.Model.second_model, vt.Model.third_model):
        assert mk(R=3, n=2, L=2).compile_step_predicates(models_text).names == ["LogNeverShrinks", "NobodyEntersStateTransfer"]
    # a primed variable is a step program's: the state compiler refuses it (and vsrmc_checker_action_constrain_attach refuses a state program)
    with pytest.raises(vt.VsrmcError):
        m.compile_predicates(ar.TEXTS["CommitNeverDecreases"])
    # under SYMMETRY a value literal is refused, primed or not: every accepted action constraint is symmetric
    with pytest.raises(vt.VsrmcError):
        m.compile_step_predicates(r"A == \A r \in replicas : \A i \in DOMAIN rep_log'[r] : rep_log'[r][i] = v1")


def test_header_binding_and_library_agree(vt):
    hdr = open(os.path.join(ROOT, "include", "vsrmc.h")).read()
    from vsr_tlaplus_amd import capi
    lib = C.CDLL(capi.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in capi.SYMBOLS and hasattr(lib, name), name
    assert "VSRMC_ACTION_SLICE" in hdr and "VSRMC_ACTION_LIST_CAP" in hdr                  # the test knobs are documented where the others are
    # the struct of the binding has the size of the header's: 2 x int32, 21 + 16 counters... counted from the header's own text
    body = re.search(r"typedef struct vsrmc_action_constraint_info \{(.*?)\} vsrmc_action_constraint_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n64 = 0
    for decl in re.findall(r"(?:uint64_t|double)\s+([^;]+);", body):
        for name in decl.split(","):
            dim = re.search(r"\[(\d+)\]", name)
            n64 += int(dim.group(1)) if dim else 1
    assert C.sizeof(capi.ActionConstraintInfo) == 8 + 8 * n64
