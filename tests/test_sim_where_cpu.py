"""Simulation with state / step predicates, host side (`-m "not gpu"`): every refusal of vsrmc_simulate_where comes before a device is looked at, the
command line refuses the flags it used to drop silently, and the generator of the model helper (tests/sim_where_model.py) against draws worked out
by hand.  What the walks compute is checked on the GPU (test_sim_where_gpu.py)."""
import os
import subprocess

import pytest

import sim_where_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vsr_tlaplus_amd", "vsrmc")
E_ARG = -1


@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


@pytest.fixture(scope="module")
def m(vt):
    return vt.Model.from_constants(R=3, C_=1, n=2, L=2)


def _refused(vt, call, needle):
    with pytest.raises(vt.VsrmcError) as e:
        call()
    assert e.value.code == E_ARG and needle in e.value.message, (e.value.code, e.value.message)


def test_both_programs_absent_is_refused(vt, m):
    _refused(vt, lambda: m.simulate_where(), "neither a state program nor a step program")


def test_a_program_in_the_other_position_is_refused(vt, m):
    state, step = m.compile_predicates("TRUE"), m.compile_step_predicates("aux_svc' = aux_svc")
    _refused(vt, lambda: m.simulate_where(state=step), "step program")
    _refused(vt, lambda: m.simulate_where(step=state), "state program")
    _refused(vt, lambda: m.simulate_where(state=step, step=state), "step program")


@pytest.mark.parametrize("other", ["constants", "second", "third"])
def test_a_program_of_another_model_is_refused(vt, m, other):
    o = dict(constants=lambda: vt.Model.from_constants(R=2, C_=1, n=2, L=2), second=lambda: vt.Model.second_model(R=3, n=2, L=2),
             third=lambda: vt.Model.third_model(R=3, n=2, L=2))[other]()
    _refused(vt, lambda: o.simulate_where(state=m.compile_predicates("TRUE")), "compiled for another model")
    _refused(vt, lambda: o.simulate_where(step=m.compile_step_predicates("aux_svc' = aux_svc")), "compiled for another model")
    _refused(vt, lambda: m.simulate_where(state=o.compile_predicates("TRUE")), "compiled for another model")
    _refused(vt, lambda: m.simulate_where(state=m.compile_predicates("TRUE"), step=o.compile_step_predicates("aux_svc' = aux_svc")), "compiled for another model")


@pytest.mark.parametrize("depth", [0, -1, 513])
def test_max_depth_outside_its_range_is_refused(vt, m, depth):
    _refused(vt, lambda: m.simulate_where(state=m.compile_predicates("TRUE"), max_depth=depth), "max_depth outside 1..512")


def test_the_refusals_need_no_device(vt, m):
    """the same calls in a process that sees no device at all: still VSRMC_E_ARG with the same messages, not VSRMC_E_HIP"""
    code = ("import vsr_tlaplus_amd as vt\n"
            "m = vt.Model.from_constants(R=3, C_=1, n=2, L=2)\n"
            "for kw in (dict(), dict(state=m.compile_step_predicates(\"aux_svc' = aux_svc\")), dict(state=m.compile_predicates('TRUE'), max_depth=0)):\n"
            "    try:\n"
            "        m.simulate_where(**kw)\n"
            "    except vt.VsrmcError as e:\n"
            "        print(e.code, e.message)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run(["python3", "-c", code], capture_output=True, text=True, env=env, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and len(lines) == 3, (r.stdout, r.stderr)
    assert all(ln.startswith("-1 ") for ln in lines), lines
    assert "neither" in lines[0] and "step program" in lines[1] and "max_depth" in lines[2]


def test_the_result_struct_has_the_layout_of_the_header(vt):
    import ctypes as C
    from vsr_tlaplus_amd import capi
    r = capi.SimWhereResult
    assert (r.found.offset, r.viol_mask.offset, r.viol_steps.offset, r.steps.offset, r.walks.offset, r.rounds.offset) == (0, 4, 8, 16, 24, 32)
    assert (r.n_states.offset, r.n_pairs.offset, r.count_state.offset, r.count_step.offset, r.seconds.offset, r.ords.offset) == (40, 48, 56, 120, 184, 192)
    assert C.sizeof(r) == 192 + 4 * 512


# ---- the command line, as far as it gets without a device ----------------------------------------------------------------------------------------
def _cli(args):
    return subprocess.run([CLI] + args + ["-noTLA"], capture_output=True, text=True, timeout=120)


@pytest.fixture()
def cfg(vt, tmp_path):
    from test_host_cpu import _cfg
    return _cfg(tmp_path, R=3, vals="v1, v2", L=1)


@pytest.mark.parametrize("flags, needle", [
    (["-reach", "LogDivergence"], "-reach / -invariant / -whereReport need -predicates FILE"),
    (["-invariant", "LogDivergence"], "-reach / -invariant / -whereReport need -predicates FILE"),
    (["-whereReport"], "-reach / -invariant / -whereReport need -predicates FILE"),
    (["-stepReach", "CommitMonotonic"], "-stepReach / -stepInvariant / -stepReport need -steps FILE"),
    (["-stepInvariant", "CommitMonotonic"], "-stepReach / -stepInvariant / -stepReport need -steps FILE"),
    (["-stepReport"], "-stepReach / -stepInvariant / -stepReport need -steps FILE"),
])
def test_cli_refuses_a_question_without_its_file(cfg, flags, needle):
    r = _cli(["-config", cfg, "-simulate"] + flags)
    assert r.returncode == 2 and needle in r.stderr and "Simulation stopped" not in r.stdout, (r.stdout, r.stderr)


def test_cli_refuses_a_file_without_a_question(cfg):
    """-simulate used to drop -predicates / -steps without a word and report "without a violation" for a question never asked"""
    for flags in (["-predicates", os.path.join(ROOT, "tools", "predicates_example.txt")], ["-steps", os.path.join(ROOT, "tools", "steps_example.txt")],
                  ["-simRounds", "2"]):
        r = _cli(["-config", cfg, "-simulate"] + flags)
        assert r.returncode == 2 and "-simulate:" in r.stderr and "Simulation stopped" not in r.stdout, (flags, r.stdout, r.stderr)


def test_cli_refuses_a_name_the_file_does_not_export(cfg):
    r = _cli(["-config", cfg, "-simulate", "-predicates", os.path.join(ROOT, "tools", "predicates_example.txt"), "-reach", "NoSuchName"])
    assert r.returncode == 2 and "exports no predicate NoSuchName" in r.stderr
    r = _cli(["-config", cfg, "-simulate", "-steps", os.path.join(ROOT, "tools", "steps_example.txt"), "-stepInvariant", "NoSuchName"])
    assert r.returncode == 2 and "exports no predicate NoSuchName" in r.stderr


def test_cli_help_names_the_new_flags():
    r = subprocess.run([CLI, "-help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "-simRounds N" in r.stdout and "every\n" in r.stdout


# ---- the generator of the model helper ------------------------------------------------------------------------------------------------------------
def test_generator_against_hand_computed_draws():
    """seed 1, walker 0.  splitmix64: x = 1 + 0x9E3779B97F4A7C15 = 0x9E3779B97F4A7C16; z = (x ^ x >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) *
    0x94D049BB133111EB, z ^= z >> 31 -> 0x910A2DEC89025CC1 (the published first output of splitmix64 for seed 1).  Then three rounds of xorshift64*
    (x ^= x >> 12, x ^= x << 25, x ^= x >> 27; draw = x * 0x2545F4914F6CDD1D mod 2^64), worked out outside this repository's code."""
    s0, s1 = sm.splitmix64_stream(1, 2)
    assert (s0, s1) == (0x910A2DEC89025CC1, 0xBEEB8DA1658EEC67)
    draws = []
    x = s0
    for _ in range(3):
        x, d = sm.xorshift64star(x)
        draws.append(d)
    assert draws == [0x4B46A55DF3611B9B, 0xD7E1F1410E763EF4, 0x5F14EC66975F9B06]
    assert sm.splitmix64_stream(2 ** 64 - 1, 1)[0] != 0               # (a zero output would be replaced by 1: xorshift must not start at 0)
