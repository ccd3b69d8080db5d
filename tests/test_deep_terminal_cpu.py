"""The deadlock check beyond the record buffers, the part that needs no device (`-m "not gpu"`): the per-level figures the GPU tests compare against, from
the CPU oracle; the CLI refuses -deepTerminal where it cannot honour it, before any device call; the ValueError rules of run(deep=True); the header, the
library and the ctypes structure agree."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
SYMBOLS = ["vsrmc_checker_deep_terminal_attach", "vsrmc_checker_deep_terminal_levels", "vsrmc_checker_deep_terminal_result",
           "vsrmc_checker_deep_terminal_states", "vsrmc_checker_deep_terminal_witness"]

# states per level / terminal states per level, by the CPU oracle (terminal = `deadlocks` of the step that expands the level = successors == [])
STATES_3111 = [1, 3, 8, 24, 68, 163, 332, 595, 968, 1457, 2027, 2621, 3289, 4191, 5306, 6166]            # (3,1,{v1},1), levels 1-16
TERMINAL_3111 = [0] * 10 + [1, 8, 12, 18, 47, 141]
STATES_3121 = {11: 2533, 12: 3793, 13: 5664, 14: 8514, 15: 12640, 16: 17992, 17: 24159, 18: 30675}      # (3,1,{v1,v2},1), levels 11-18
TERMINAL_3121 = {11: 0, 12: 0, 13: 0, 14: 0, 15: 4, 16: 24, 17: 64, 18: 131}


@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


def _oracle_levels(orc, P, depth):
    """[(states, terminal states)] of levels 1 .. depth"""
    b = orc.Bfs(P)
    out, n = [], 1
    for _ in range(depth):
        nn = b.step()
        out.append((n, b.info["deadlocks"]))
        n = nn
    b.close()
    return out


def test_oracle_levels_of_the_three_replica_spaces(vt):
    from oracle import orc
    got = _oracle_levels(orc, orc.Params(3, 1, 1, 1), 16)
    assert [g[0] for g in got] == STATES_3111 and [g[1] for g in got] == TERMINAL_3111
    assert sum(TERMINAL_3111) == 227
    got = _oracle_levels(orc, orc.Params(3, 1, 2, 1), 18)
    assert {lvl: got[lvl - 1][0] for lvl in STATES_3121} == STATES_3121
    assert {lvl: got[lvl - 1][1] for lvl in TERMINAL_3121} == TERMINAL_3121
    assert all(t == 0 for _, t in got[:14])


@pytest.fixture()
def cfg(tmp_path):
    path = tmp_path / "VSR.cfg"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_cfg.py"), str(path), "3", "1", "v1, v2", "1"], check=True)
    return str(path)


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)


def test_cli_refuses_deep_terminal_alone(vt, cfg):
    r = _run(["-config", cfg, "-noTLA", "-deepTerminal"])
    assert r.returncode == 2 and "-deepTerminal needs -checkDeadlock" in r.stderr and "-terminalReport" in r.stderr, (r.returncode, r.stderr)
    assert "lowered" not in r.stdout and "Progress" not in r.stdout   # refused before the model is printed, let alone a checker created


@pytest.mark.parametrize("extra, text", [(["-gpus", "2"], "-deepTerminal runs on one GPU"), (["-simulate"], "-deepTerminal belongs to the exhaustive search"),
                                         (["-probe2At", "5"], "-probe2At / -probe3At"), (["-probe3At", "6"], "-probe2At / -probe3At")],
                         ids=["gpus", "simulate", "probe2", "probe3"])
@pytest.mark.parametrize("ask", [["-checkDeadlock"], ["-terminalReport"]], ids=["deadlock", "report"])
def test_cli_refuses_deep_terminal_where_it_cannot_run(vt, cfg, ask, extra, text):
    r = _run(["-config", cfg, "-noTLA", "-deepTerminal"] + ask + extra)
    assert r.returncode == 2 and text in r.stderr and "Progress" not in r.stdout, (r.returncode, r.stderr, r.stdout)


def test_cli_refuses_deep_terminal_with_a_constraint(vt, cfg, tmp_path):
    pred = tmp_path / "p.txt"
    pred.write_text("Always == TRUE\n")
    steps = tmp_path / "s.txt"
    steps.write_text("Mono == \\A r \\in replicas : rep_view_number'[r] >= rep_view_number[r]\n")
    for extra in (["-predicates", str(pred), "-constraint", "Always"], ["-steps", str(steps), "-actionConstraint", "Mono"]):
        r = _run(["-config", cfg, "-noTLA", "-checkDeadlock", "-deepTerminal"] + extra)
        assert r.returncode == 2 and "-deepTerminal cannot be combined with -constraint / -actionConstraint" in r.stderr and "Progress" not in r.stdout, (r.returncode, r.stderr)


def test_cli_help_names_the_switch(vt):
    r = _run(["--help"])
    assert r.returncode == 0 and "-deepTerminal" in r.stdout


def test_run_deep_value_errors(vt):
    mc = vt.ModelChecker.__new__(vt.ModelChecker)                   # run() raises before it touches the checker
    mc._constraint = None

    class W:
        names = ["P"]
        step = False
    with pytest.raises(ValueError, match="needs a predicate or check_deadlock"):
        mc.run(deep=True)
    with pytest.raises(ValueError, match="one state program"):
        mc.run(deep=True, check_deadlock=True, never=W(), reach=W())
    with pytest.raises(ValueError, match="one step program"):
        mc.run(deep=True, check_deadlock=True, step_never=W(), step_reach=W())
    with pytest.raises(ValueError, match="has not stopped at a terminal state beyond"):
        mc.deadlock = None
        mc.deep_terminal_trace()


def test_header_library_and_ctypes_agree(vt, tmp_path):
    from vsr_tlaplus_amd import build, capi
    hdr = open(os.path.join(ROOT, "include", "vsrmc.h")).read()
    declared = set(re.findall(r"\b(vsrmc_[a-z_0-9]+)\s*\(", hdr))
    lib = C.CDLL(capi.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "%s"\nint main() { std::printf("%%zu %%zu %%zu\\n", sizeof(vsrmc_deep_terminal_info), '
                   'offsetof(vsrmc_deep_terminal_info, min_fp), offsetof(vsrmc_deep_terminal_info, ms)); return 0; }\n' % os.path.join(ROOT, "include", "vsrmc.h"))
    exe = tmp_path / "sizes"
    subprocess.run([build.HIPCC, "-std=c++17", "-o", str(exe), str(src)], check=True, capture_output=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = capi.DeepTerminalInfo
    assert sizes == [C.sizeof(T), T.min_fp.offset, T.ms.offset], sizes
