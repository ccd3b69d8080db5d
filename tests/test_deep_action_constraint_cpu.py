"""Action constraints on the levels beyond the record buffers, the part that needs no device (`-m "not gpu"`): the floors of the reference
(tests/action_constraint_reference.py::constrained_bfs) on the spaces test_deep_action_constraint_gpu.py uses, as constants checked against the reference, so
that no GPU test can pass on an empty reference; the CLI's usage errors around -deepActionConstraint, refused before any device call; the header, the
binding and the library agree on the two new entry points."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import action_constraint_reference as ar
import step_reference as sr
import test_deep_action_constraint_gpu as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
SYMBOLS = ["vsrmc_checker_action_constrain_deep", "vsrmc_checker_action_constraint_deep_info"]
QUIET_2122_NEW = [1, 2, 3, 6, 12, 21, 33, 48, 63, 75, 86, 98, 109, 115, 120, 120, 110, 99, 91, 88, 72, 48, 32, 25, 20, 10, 3]
QUIET_2122_BLOCKED = [0, 0, 2, 0, 0, 0, 1, 0, 2, 3, 6, 8, 8, 8, 4, 9, 14, 9, 7, 3, 5, 4, 2, 0, 0, 0, 0]   # per step INTO levels 1 ..
QUIET_2122_NEVER = [0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 5, 5, 5, 3, 7, 12, 9, 7, 3, 5, 4, 2, 0, 0, 0, 0, 0]    # never-entering blocked targets of the step OUT of levels 1 ..
QUIET_3121_NEW = [1, 3, 8, 24, 68, 163, 332, 596, 967, 1434, 1942, 2452, 3076, 4045]
COMMIT_3111_NEW = [1, 3, 8, 24, 68, 163, 332, 595, 968, 1457, 2027, 2621, 3287, 4171, 5229, 5989, 5842, 4636, 2895, 1377, 478, 113, 16, 1]


@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


# ---- the reference's floors ---------------------------------------------------------------------------------------------------------------------
def test_floor_quiet_client_2122_whole_space():
    r = ar.constrained_bfs("first", 2, 1, 2, 2, ar.quiet_client)
    assert (r.states, r.depth, r.blocked, r.rescued) == (1510, 27, 95, 5)
    assert [len(lv.new) for lv in r.levels] == QUIET_2122_NEW + [0]
    assert [lv.blocked for lv in r.levels] == QUIET_2122_BLOCKED + [0]
    assert [lv.level for lv in r.levels if lv.rescued] == [3, 7, 11, 15, 16]
    never = [len(T._never_entering("quiet-2122", r, lvl)) for lvl in range(1, 28)]
    assert never == QUIET_2122_NEVER and all(1 <= n <= 12 for n in never[7:22])     # from level 8 through the step out of level 22
    # the bases of the GPU test leave deep levels that block, rescue and have never-entering targets above each of them
    for base in (4, 9, 14, 20):
        assert sum(QUIET_2122_BLOCKED[base:]) > 0 and len(QUIET_2122_NEW) - base >= 7
    assert sum(never[9:16]) == 40


def test_floor_quiet_client_3121_first_14_levels():
    r = ar.constrained_bfs("first", 3, 1, 2, 1, ar.quiet_client, max_levels=14)
    assert (r.states, r.blocked, r.rescued) == (15111, 2806, 28)
    assert [len(lv.new) for lv in r.levels] == QUIET_3121_NEW
    assert all(lv.rescued for lv in r.levels[2:14])                                 # at least one rescued state in every level 3 - 14
    assert len(T._never_entering("quiet-3121", r, 13)) == 918


def test_floor_commit_never_decreases_3111_whole_space():
    r = ar.constrained_bfs("first", 3, 1, 1, 1, sr.commit_monotonic)
    assert (r.states, r.depth, r.blocked) == (42301, 24, 1640)
    assert [len(lv.new) for lv in r.levels] == COMMIT_3111_NEW + [0]
    assert next(lv.level for lv in r.levels if lv.blocked) == 13                    # the first block is in the step into level 13
    assert all(COMMIT_3111_NEW[i] > COMMIT_3111_NEW[i + 1] for i in range(15, 23))  # the levels shrink from level 17 on: a re-basing occurs


# ---- the CLI's usage errors: refused before any device call -------------------------------------------------------------------------------------
@pytest.fixture()
def files(tmp_path):
    cfg = tmp_path / "VSR.cfg"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_cfg.py"), str(cfg), "3", "1", "v1, v2", "1"], check=True)
    return str(cfg), os.path.join(ROOT, "tools", "constraints_example.txt"), os.path.join(ROOT, "tools", "action_constraints_example.txt")


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)


ACT = ["-steps", "S", "-actionConstraint", "QuietClient", "-deepActionConstraint"]


@pytest.mark.parametrize("extra, needle", [
    (["-deepActionConstraint"], "-deepActionConstraint needs -actionConstraint NAME"),
    (["-steps", "S", "-deepActionConstraint"], "-deepActionConstraint needs -actionConstraint NAME"),
    (ACT + ["-predicates", "P", "-constraint", "Replica3Normal"], "cannot be combined with -constraint"),
    (ACT + ["-predicates", "P", "-constraint", "Replica3Normal", "-deepConstraint"], "cannot be combined with -actionConstraint"),
    (ACT + ["-predicates", "P", "-invariant", "NotAllInViewChange", "-deepPredicates"], "cannot be combined with -deepPredicates"),
    (ACT + ["-deepTerminal"], "cannot be combined with -deepTerminal"),
    (ACT + ["-probeLast"], "-probeLast / -probe2At / -probe3At: those passes do not gate"),
    (ACT + ["-probe2At", "5"], "-probeLast / -probe2At / -probe3At: those passes do not gate"),
    (ACT + ["-probe3At", "5"], "-probeLast / -probe2At / -probe3At: those passes do not gate"),
    (ACT + ["-checkpoint", "C"], "-checkpoint / -recover"),
    (ACT + ["-recover", "C"], "-checkpoint / -recover"),
    (ACT + ["-audit"], "cannot be combined with -audit"),
    (ACT + ["-simulate"], "a random walk (-simulate) is not constrained"),
    (ACT + ["-gpus", "2"], "-actionConstraint runs on one GPU"),
    (["-steps", "S", "-actionConstraint", "QuietClient", "-probeLast"], "the levels beyond the record buffers are not constrained"),   # without the opt-in: as before
])
def test_cli_refuses_the_flag_where_it_cannot_honour_it(vt, files, tmp_path, extra, needle):
    cfg, pred, steps = files
    args = [pred if a == "P" else steps if a == "S" else str(tmp_path / "chk") if a == "C" else a for a in extra]
    r = _run(["-config", cfg, "-noTLA"] + args)
    assert r.returncode == 2 and needle in r.stderr, (r.returncode, r.stderr)
    assert "lowered" not in r.stdout and "Finished computing" not in r.stdout        # before the model is printed, let alone a checker created


def test_cli_help_names_the_option(vt):
    r = _run(["--help"])
    assert r.returncode == 0 and "-deepActionConstraint" in r.stdout and "-actionConstraint NAME" in r.stdout


# ---- header, binding, library -------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree(vt):
    from vsr_tlaplus_amd import capi
    header = open(os.path.join(ROOT, "include", "vsrmc.h")).read()
    lib = vt.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.SYMBOLS and getattr(lib, name) is not None
    # struct vsrmc_action_constraint_deep_info: two int32, 27 uint64, three doubles; vsrmc_action_constraint_info keeps its layout
    assert C.sizeof(capi.ActionConstraintDeepInfo) == 8 + 27 * 8 + 3 * 8
    assert C.sizeof(capi.ActionConstraintInfo) == 8 + 28 * 8 + 3 * 8
    m = re.search(r"typedef struct vsrmc_action_constraint_deep_info \{(.*?)\} vsrmc_action_constraint_deep_info;", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = re.findall(r"\b([a-z_]+)(?:\[16\])?(?=[,;])", body)
    assert names == [f for f, _t in capi.ActionConstraintDeepInfo._fields_], names


def test_python_signature_takes_the_opt_in(vt):
    import inspect
    sig = inspect.signature(vt.ModelChecker.action_constrain)
    assert list(sig.parameters) == ["self", "step_where", "name", "deep"] and sig.parameters["deep"].default is False
    assert hasattr(vt.ModelChecker, "action_constraint_deep_results")
