"""Predicates beyond the record buffers, the part that needs no device (`-m "not gpu"`): the CLI refuses -deepPredicates where it cannot honour it,
before any device call; the header declares what the library exports; the ctypes structures have the sizes the header's have."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
DEEP_SYMBOLS = ["vsrmc_checker_deep_attach", "vsrmc_checker_deep_levels", "vsrmc_checker_deep_result", "vsrmc_checker_deep_where_states",
                "vsrmc_checker_deep_step_pairs", "vsrmc_checker_deep_witness"]

@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


@pytest.fixture()
def files(tmp_path):
    cfg = tmp_path / "VSR.cfg"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_cfg.py"), str(cfg), "3", "1", "v1, v2", "1"], check=True)
    pred = tmp_path / "p.txt"
    pred.write_text("Div == \\E r1, r2 \\in replicas : rep_op_number[r1] # rep_op_number[r2]\n")
    steps = tmp_path / "s.txt"
    steps.write_text("Mono == \\A r \\in replicas : rep_view_number'[r] >= rep_view_number[r]\n")
    return str(cfg), str(pred), str(steps)


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)


def test_cli_refuses_deep_predicates_without_a_predicate_flag(vt, files):
    cfg, pred, steps = files
    for extra in ([], ["-predicates", pred], ["-steps", steps]):      # (a file alone asks for nothing)
        r = _run(["-config", cfg, "-noTLA", "-deepPredicates"] + extra)
        assert r.returncode == 2, (r.returncode, r.stderr)
        assert "-deepPredicates needs -reach / -invariant / -whereReport" in r.stderr and "-stepReach / -stepInvariant / -stepReport" in r.stderr
        assert "lowered" not in r.stdout                              # refused before the model is printed, let alone a checker created


def test_cli_refuses_deep_predicates_on_several_gpus(vt, files):
    cfg, pred, _ = files
    r = _run(["-config", cfg, "-noTLA", "-predicates", pred, "-reach", "Div", "-deepPredicates", "-gpus", "2"])
    assert r.returncode == 2 and "-deepPredicates runs on one GPU" in r.stderr and r.stdout == "", (r.returncode, r.stderr, r.stdout)


def test_cli_refuses_deep_predicates_with_simulate(vt, files):
    cfg, pred, steps = files
    r = _run(["-config", cfg, "-noTLA", "-predicates", pred, "-reach", "Div", "-deepPredicates", "-simulate"])
    assert r.returncode == 2 and "-deepPredicates belongs to the exhaustive search" in r.stderr and "lowered" not in r.stdout, (r.returncode, r.stderr)


def test_cli_refuses_deep_predicates_with_the_fixed_probe_levels_and_with_two_state_programs(vt, files):
    cfg, pred, steps = files
    r = _run(["-config", cfg, "-noTLA", "-predicates", pred, "-reach", "Div", "-deepPredicates", "-probe2At", "5"])
    assert r.returncode == 2 and "-probe2At / -probe3At" in r.stderr
    r = _run(["-config", cfg, "-noTLA", "-predicates", pred, "-reach", "Div", "-whereReport", "-deepPredicates"])
    assert r.returncode == 2 and "one program of each kind" in r.stderr
    r = _run(["--help"])
    assert r.returncode == 0 and "-deepPredicates" in r.stdout


def test_header_declares_what_the_library_exports(vt):
    from vsr_tlaplus_amd import capi
    hdr = open(os.path.join(ROOT, "include", "vsrmc.h")).read()
    declared = set(re.findall(r"\b(vsrmc_[a-z_0-9]+)\s*\(", hdr))
    lib = C.CDLL(capi.LIB_PATH)
    for name in DEEP_SYMBOLS:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (vsrmc_[a-z_0-9]+)$", nm, re.M))
    hooks = set(capi.HOOK_SYMBOLS)
    assert exported - hooks == declared, (exported - hooks) ^ declared


def test_ctypes_structs_match_the_header(vt, tmp_path):
    from vsr_tlaplus_amd import build, capi
    pairs = [("vsrmc_deep_info", capi.DeepInfo), ("vsrmc_where_info", capi.WhereInfo), ("vsrmc_step_info", capi.StepInfo), ("vsrmc_level_info", capi.LevelInfo)]
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstdio>\n#include "%s"\nint main() { std::printf("%s\\n", %s); return 0; }\n' % (
        os.path.join(ROOT, "include", "vsrmc.h"), " ".join("%zu" for _ in pairs), ", ".join("sizeof(%s)" % n for n, _ in pairs)))
    exe = tmp_path / "sizes"
    subprocess.run([build.HIPCC, "-std=c++17", "-o", str(exe), str(src)], check=True, capture_output=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(t) for _, t in pairs], (sizes, [C.sizeof(t) for _, t in pairs])
    assert C.sizeof(capi.WhereInfo) == 8 + 8 + 3 * 64 + 8 and C.sizeof(capi.StepInfo) == 8 + 3 * 8 + 3 * 64 + 2 * 32 + 3 * 8 + 8   # the existing layouts are untouched
