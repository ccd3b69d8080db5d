"""State constraints, the part that needs no device (`-m "not gpu"`): the reference itself (tests/constraint_reference.py) on the spaces the GPU tests
use — floors on its kept / pruned / "satisfying but never reached" counts, so that an empty case cannot pass there, and its time bounds; the CLI's usage
errors, refused before any device call; the example files compile for their models; the header, the binding and the library agree."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import constraint_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
SYMBOLS = ["vsrmc_checker_constrain_attach", "vsrmc_checker_constraint_info", "vsrmc_checker_constraint_pruned"]


@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------
def test_reference_narrow_network_on_2122():
    r = cr.constrained_bfs("first", 2, 1, 2, 2, cr.narrow_network)
    print("(2,1,{v1,v2},2) NarrowNetwork: %d levels, %d in model, %d pruned, %d satisfying, %d of them never reached, %.2f s"
          % (len(r.levels), r.in_model, r.pruned_total, len(r.satisfying), len(r.unreachable), r.seconds))
    assert r.in_model >= 100 and r.pruned_total >= 20 and len(r.unreachable) >= 100 and r.depth >= 10
    assert r.in_model + len(r.unreachable) == len(r.satisfying)        # every state the constrained search reaches satisfies the constraint and is reachable
    assert all(not (set(lv.kept) & set(lv.pruned)) for lv in r.levels)
    assert sum(1 for lv in r.levels if lv.pruned) >= 3
    assert r.seconds < 2.0                                             # (0.2 s: both searches of a space of 2 073 states)


def test_reference_replica3_normal_on_3121_and_3111():
    r = cr.constrained_bfs("first", 3, 1, 2, 1, cr.replica3_normal, with_unconstrained=False)
    print("(3,1,{v1,v2},1) Replica3Normal: %d levels, %d in model, %d pruned, largest level %d, %.2f s"
          % (len(r.levels), r.in_model, r.pruned_total, max(len(lv.kept) for lv in r.levels), r.seconds))
    assert r.in_model >= 1000 and r.pruned_total >= 500 and r.depth >= 15
    assert max(len(lv.kept) for lv in r.levels) > 256                  # more than one block of k_constrain
    assert r.seconds < 5.0                                             # (about a second)
    r1 = cr.constrained_bfs("first", 3, 1, 1, 1, cr.replica3_normal, with_unconstrained=False)
    assert r1.in_model >= 100 and r1.pruned_total >= 100 and r1.depth >= 10


def test_reference_degenerate_constraints():
    t = cr.constrained_bfs("first", 2, 1, 2, 2, lambda s: True)
    assert t.pruned_total == 0 and not t.unreachable and t.in_model == len(t.satisfying) >= 1000
    one = cr.constrained_bfs("first", 2, 1, 2, 2, cr.init_only, with_unconstrained=False)
    assert one.in_model == 1 and one.depth == 1 and len(one.levels) == 2 and len(one.levels[1].pruned) >= 2 and not one.levels[1].kept
    none = cr.constrained_bfs("first", 2, 1, 2, 2, lambda s: False, with_unconstrained=False)
    assert none.in_model == 0 and len(none.levels) == 1 and len(none.levels[0].pruned) == 1


def test_reference_invariant_first_fails_on_a_pruned_state():
    """test 6 of the GPU suite: NotAllInViewChange first fails, under Replica3Normal, on an out-of-model state"""
    r = cr.constrained_bfs("first", 3, 1, 2, 1, cr.replica3_normal, with_unconstrained=False)
    orc, unpack, make_pm = cr.oracle_of("first")
    PM = make_pm(3, 1, 2, 1)
    first_kept = first_pruned = None
    for lv in r.levels:
        if first_kept is None and any(not cr.not_all_in_view_change(unpack(PM, [int(x) for x in rec])) for rec in lv.kept.values()):
            first_kept = lv.level
        if first_pruned is None and any(not cr.not_all_in_view_change(unpack(PM, [int(x) for x in rec])) for rec in lv.pruned.values()):
            first_pruned = lv.level
    print("NotAllInViewChange under Replica3Normal: first violated in the model at level %s, among the pruned states at level %s" % (first_kept, first_pruned))
    assert first_pruned is not None and (first_kept is None or first_pruned <= first_kept)


def test_reference_built_in_violation_on_a_pruned_state():
    """the built-in case of the GPU suite: under R3NormalCommitBelow2 the first violator of AcknowledgedWritesExistOnMajority is a pruned state of level 19"""
    r = cr.constrained_bfs("first", 3, 1, 2, 1, cr.r3normal_commit_below2, max_levels=19, with_unconstrained=False)
    orc = cr.oracle_of("first")[0]
    P = cr.params_of("first", 3, 1, 2, 1, invariant_mask=3)
    bad = [(lv.level, kind, fp, orc.invariants(P, rec)) for lv in r.levels for kind, d in (("kept", lv.kept), ("pruned", lv.pruned)) for fp, rec in d.items()
           if orc.invariants(P, rec)]
    print("built-in violators under R3NormalCommitBelow2:", bad, "in model", r.in_model)
    assert bad and all(b[:2] == (19, "pruned") and b[3] == 2 for b in bad) and r.in_model >= 1000
    assert r.seconds < 5.0


@pytest.mark.parametrize("which", ["second", "third"])
def test_reference_no_state_transfer_on_the_analysis_models(which):
    r = cr.constrained_bfs(which, 3, 0, 2, 1, cr.no_state_transfer, max_levels=12, with_unconstrained=False)
    print("%s model (3,{2 values},1) NoStateTransfer, 12 levels: %d in model, %d pruned, %.2f s" % (which, r.in_model, r.pruned_total, r.seconds))
    assert r.in_model >= 10000 and r.pruned_total >= 5 and len(r.levels) == 12
    assert r.seconds < 60.0


# ---- the CLI's usage errors: refused before any device call -------------------------------------------------------------------------------------
@pytest.fixture()
def files(tmp_path):
    cfg = tmp_path / "VSR.cfg"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_cfg.py"), str(cfg), "3", "1", "v1, v2", "1"], check=True)
    return str(cfg), os.path.join(ROOT, "tools", "constraints_example.txt")


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("extra, needle", [
    (["-constraint", "Replica3Normal"], "needs -predicates FILE"),
    (["-predicates", "P", "-constraint", "Replica3Normal", "-gpus", "2"], "-constraint runs on one GPU"),
    (["-predicates", "P", "-constraint", "Replica3Normal", "-simulate"], "a random walk (-simulate) is not constrained"),
    (["-predicates", "P", "-constraint", "Replica3Normal", "-invariant", "NotAllInViewChange", "-deepPredicates"], "-deepPredicates"),
    (["-predicates", "P", "-constraint", "Replica3Normal", "-probeLast"], "-probeLast / -probe2At / -probe3At"),
    (["-predicates", "P", "-constraint", "Replica3Normal", "-probe2At", "5"], "-probeLast / -probe2At / -probe3At"),
    (["-predicates", "P", "-constraint", "Replica3Normal", "-probe3At", "5"], "-probeLast / -probe2At / -probe3At"),
    (["-predicates", "P", "-constraint", "Replica3Normal", "-checkpoint", "C"], "-checkpoint / -recover"),
    (["-predicates", "P", "-constraint", "Replica3Normal", "-recover", "C"], "-checkpoint / -recover"),
])
def test_cli_refuses_constraint_where_it_cannot_honour_it(vt, files, tmp_path, extra, needle):
    cfg, pred = files
    args = [pred if a == "P" else str(tmp_path / "chk") if a == "C" else a for a in extra]
    r = _run(["-config", cfg, "-noTLA"] + args)
    assert r.returncode == 2 and "-constraint" in r.stderr and needle in r.stderr, (r.returncode, r.stderr)
    assert "lowered" not in r.stdout and "Finished computing" not in r.stdout        # before the model is printed, let alone a checker created


def test_cli_help_names_the_option(vt):
    r = _run(["--help"])
    assert r.returncode == 0 and "-constraint NAME" in r.stdout


# ---- the example files compile for their models -------------------------------------------------------------------------------------------------
def test_example_files_compile(vt):
    text = open(os.path.join(ROOT, "tools", "constraints_example.txt")).read()
    w = vt.Model.from_constants(R=3, C_=1, n=2, L=1).compile_predicates(text)
    assert w.names == ["NarrowNetwork", "Replica3Normal", "ViewsBelow3", "NotAllInViewChange"] and not w.step
    text = open(os.path.join(ROOT, "tools", "constraints_models_example.txt")).read()
    for make in (vt.Model.second_model, vt.Model.third_model):
        w = make(R=3, n=2, L=1).compile_predicates(text)
        assert w.names == ["NoStateTransfer", "ViewsBelow2", "NoGetStateToAny"]
    # the texts the GPU tests compile are the ones the example files hold
    for name in ("NarrowNetwork", "Replica3Normal", "NotAllInViewChange", "R3NormalCommitBelow2"):
        w = vt.Model.from_constants(R=3, C_=1, n=2, L=1).compile_predicates(cr.TEXTS[name])
        assert w.names == [name]


# ---- header, binding, library -------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree(vt):
    from vsr_tlaplus_amd import capi
    header = open(os.path.join(ROOT, "include", "vsrmc.h")).read()
    lib = vt.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.SYMBOLS and getattr(lib, name) is not None
    # struct vsrmc_constraint_info: two int32, eight uint64, two arrays of eight uint64, one double
    assert C.sizeof(capi.ConstraintInfo) == 8 + 8 * 8 + 2 * 64 + 8
    assert "VSRMC_CONSTRAIN_GRID" in header
