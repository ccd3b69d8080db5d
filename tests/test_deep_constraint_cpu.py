"""State constraints on the levels beyond the record buffers, the part that needs no device (`-m "not gpu"`): the reference (tests/constraint_reference.py)
on the spaces test_deep_constraint_gpu.py uses — its exact per-level figures on the main space, so that the GPU tests' expectations are the reference's and
not the library's, and floors where a case could otherwise be empty; the CLI's usage errors around -deepConstraint, refused before any device call; the
header, the binding and the library agree."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import constraint_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
SYMBOLS = ["vsrmc_checker_constrain_deep", "vsrmc_checker_constraint_deep_info", "vsrmc_checker_constraint_pruned_level"]
KEPT = [1, 2, 4, 8, 14, 21, 29, 40, 56, 72, 92, 119, 159, 211, 277, 361, 473, 588, 654, 632, 515, 339, 178, 66, 13]
PRUNED = [0, 1, 2, 5, 11, 21, 33, 48, 68, 93, 117, 145, 179, 214, 227, 212, 176, 136, 100, 68, 36, 12, 2, 0, 0]


@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


@pytest.fixture(scope="module")
def main_space():
    return cr.constrained_bfs("first", 3, 1, 2, 1, cr.replica3_normal, with_unconstrained=False)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------
def test_reference_main_space_level_by_level(main_space):
    r = main_space
    assert (r.in_model, r.pruned_total, r.depth) == (4924, 1906, 25)
    assert [len(lv.kept) for lv in r.levels] == KEPT and [len(lv.pruned) for lv in r.levels] == PRUNED
    assert all(PRUNED[i] for i in range(1, 23))                        # every level from 2 to 23 prunes something: a missed filter anywhere changes a figure
    peak = KEPT.index(max(KEPT)) + 1
    assert peak == 19 and all(KEPT[i] > KEPT[i + 1] for i in range(18, 24))   # the levels shrink after 19: small buffers re-base
    assert all(lv.generated > 0 for lv in r.levels[1:])
    # the bases of the GPU tests leave at least three levels to insert, and the levels above them prune
    for base in (6, 8, 9, 12, 17):
        assert sum(1 for i in range(base, 25) if PRUNED[i]) >= 3 and PRUNED[base] > 4
    # more pruned states per level than a list of 4 holds, on most levels above base 12
    assert sum(1 for i in range(12, 25) if PRUNED[i] > 4) >= 8


def test_reference_invariant_fails_among_the_pruned_states_of_a_level_above_the_bases(main_space):
    orc, unpack, make_pm = cr.oracle_of("first")
    PM = make_pm(3, 1, 2, 1)
    first = next(lv.level for lv in main_space.levels
                 if any(not cr.not_all_in_view_change(unpack(PM, [int(x) for x in rec])) for rec in lv.pruned.values()))
    print("NotAllInViewChange under Replica3Normal: first violated among the pruned states of level", first)
    assert first >= 4                                                  # bases first - 1, first - 2, first - 3 (Init itself) exist
    assert all(cr.not_all_in_view_change(unpack(PM, [int(x) for x in rec])) for lv in main_space.levels for rec in lv.kept.values())


def test_reference_built_in_violation_is_above_bases_10_and_16():
    r = cr.constrained_bfs("first", 3, 1, 2, 1, cr.r3normal_commit_below2, max_levels=19, with_unconstrained=False)
    orc = cr.oracle_of("first")[0]
    P = cr.params_of("first", 3, 1, 2, 1, invariant_mask=3)
    bad = [(lv.level, kind) for lv in r.levels for kind, d in (("kept", lv.kept), ("pruned", lv.pruned)) for rec in d.values() if orc.invariants(P, rec)]
    assert bad and all(b == (19, "pruned") for b in bad)
    assert len(r.levels) == 19 and all(lv.kept for lv in r.levels[:18])  # level 18 has in-model states: the violator is the successor of one


def test_reference_second_model_prunes_in_levels_11_and_12():
    r = cr.constrained_bfs("second", 3, 0, 2, 1, cr.no_state_transfer, max_levels=12, with_unconstrained=False)
    assert len(r.levels) == 12 and [len(lv.pruned) for lv in r.levels[10:]] == [4, 6]
    assert all(lv.kept for lv in r.levels)


# ---- the CLI's usage errors: refused before any device call -------------------------------------------------------------------------------------
@pytest.fixture()
def files(tmp_path):
    cfg = tmp_path / "VSR.cfg"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_cfg.py"), str(cfg), "3", "1", "v1, v2", "1"], check=True)
    return str(cfg), os.path.join(ROOT, "tools", "constraints_example.txt"), os.path.join(ROOT, "tools", "action_constraints_example.txt")


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)


CON = ["-predicates", "P", "-constraint", "Replica3Normal", "-deepConstraint"]


@pytest.mark.parametrize("extra, needle", [
    (["-deepConstraint"], "-deepConstraint needs -constraint NAME"),
    (["-predicates", "P", "-deepConstraint"], "-deepConstraint needs -constraint NAME"),
    (CON + ["-steps", "S", "-actionConstraint", "X"], "cannot be combined with -actionConstraint"),
    (CON + ["-invariant", "NotAllInViewChange", "-deepPredicates"], "cannot be combined with -deepPredicates"),
    (CON + ["-deepTerminal"], "cannot be combined with -deepTerminal"),
    (CON + ["-probe2At", "5"], "-probe2At / -probe3At: those passes do not filter"),
    (CON + ["-probe3At", "5"], "-probe2At / -probe3At: those passes do not filter"),
    (CON + ["-checkpoint", "C"], "-checkpoint / -recover"),
    (CON + ["-recover", "C"], "-checkpoint / -recover"),
    (CON + ["-audit"], "cannot be combined with -audit"),
    (CON + ["-simulate"], "a random walk (-simulate) is not constrained"),
    (CON + ["-gpus", "2"], "-constraint runs on one GPU"),
])
def test_cli_refuses_deep_constraint_where_it_cannot_honour_it(vt, files, tmp_path, extra, needle):
    cfg, pred, steps = files
    args = [pred if a == "P" else steps if a == "S" else str(tmp_path / "chk") if a == "C" else a for a in extra]
    r = _run(["-config", cfg, "-noTLA"] + args)
    assert r.returncode == 2 and needle in r.stderr, (r.returncode, r.stderr)
    assert "lowered" not in r.stdout and "Finished computing" not in r.stdout        # before the model is printed, let alone a checker created


def test_cli_help_names_the_option(vt):
    r = _run(["--help"])
    assert r.returncode == 0 and "-deepConstraint" in r.stdout and "-constraint NAME" in r.stdout


# ---- header, binding, library -------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree(vt):
    from vsr_tlaplus_amd import capi
    header = open(os.path.join(ROOT, "include", "vsrmc.h")).read()
    lib = vt.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.SYMBOLS and getattr(lib, name) is not None
    # struct vsrmc_constraint_deep_info: four int32, four uint64; vsrmc_constraint_info keeps its layout
    assert C.sizeof(capi.ConstraintDeepInfo) == 4 * 4 + 4 * 8
    assert C.sizeof(capi.ConstraintInfo) == 8 + 8 * 8 + 2 * 64 + 8
    m = re.search(r"typedef struct vsrmc_constraint_deep_info \{(.*?)\} vsrmc_constraint_deep_info;", header, re.S)
    assert m and [f for f, _t in capi.ConstraintDeepInfo._fields_] == re.findall(r"\b(level|kind|filtered|list_overflowed|slices|launches|regen_records|regen_pruned)\b(?=[,;])", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))


def test_python_signature_takes_the_opt_in(vt):
    import inspect
    sig = inspect.signature(vt.ModelChecker.constrain)
    assert list(sig.parameters) == ["self", "where", "name", "deep"] and sig.parameters["deep"].default is False
