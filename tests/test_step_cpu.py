"""Step predicates, host side (`-m "not gpu"`): what csrc/vsr_where_parse.hpp accepts and refuses through Model.compile_step — primes, UNCHANGED,
step_action, quantifiers over DOMAIN messages' — and that Model.compile_where is what it was.  No device is needed to compile.  What the compiled
programs compute is checked on the GPU (test_step_gpu.py) against tests/step_reference.py."""
import os
import re

import pytest

import step_reference as sr
from test_where_cpu import ACCEPTED as STATE_ACCEPTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


@pytest.fixture(scope="module")
def m(vt):
    return vt.Model.from_constants(R=3, C_=1, n=2, L=2)


# between them: every new construct
ACCEPTED = [t for _, t, _ in sr.SET_A + sr.SET_B + sr.SET_C] + [
    r"\A r \in replicas : rep_status'[r] = rep_status[r] \/ rep_op_number'[r] # rep_op_number[r] \/ rep_last_normal_view'[r] > 0",
    r"\E r \in replicas : rep_sent_dvc'[r] /\ ~rep_sent_dvc[r] /\ rep_sent_sv[r]' = rep_sent_sv[r]",
    r"\A r, p \in replicas : rep_peer_op_number'[r][p] >= rep_peer_op_number[r][p]",
    r"\A r \in replicas : \A c \in clients : rep_client_table'[r][c].executed \/ ~rep_client_table[r][c].executed",
    r"\E r \in replicas : rep_log'[r][1].operation # rep_log[r][1].operation /\ Len(rep_log'[r]) = 1",
    r"\A r \in replicas : Cardinality(rep_svc_recv'[r]) >= Cardinality(rep_svc_recv[r]) \/ Cardinality(rep_dvc_recv[r])' = 0",
    r"(\A r \in replicas : rep_view_number[r] = 1 /\ ReplicaCount = 3)'",
    r"(\E m \in DOMAIN messages : messages[m] = 2 /\ rep_view_number[m.dest] = m.view_number)'",
    r"\E r \in replicas : \E i \in DOMAIN rep_log'[r] : ~(i \in DOMAIN rep_log[r])",
    r"\A v \in Values : v \in DOMAIN aux_client_acked => v \in DOMAIN aux_client_acked'",
    r"\E m \in DOMAIN messages' : \E n \in DOMAIN messages' : m.dest = n.source /\ messages'[m] > messages'[n]",
    r"\E m \in DOMAIN messages' : m.type = PrepareMsg /\ m.message = rep_log'[m.dest][m.op_number]",
    r"UNCHANGED rep_status /\ UNCHANGED rep_view_number /\ UNCHANGED rep_op_number /\ UNCHANGED rep_commit_number /\ UNCHANGED rep_last_normal_view /\ UNCHANGED rep_log",
    r"\A r \in replicas : UNCHANGED rep_status[r] /\ UNCHANGED rep_sent_dvc[r] /\ UNCHANGED Len(rep_log[r]) /\ UNCHANGED rep_log[r][2] /\ UNCHANGED rep_log[r][1].operation",
    r"\A v \in Values : UNCHANGED aux_client_acked[v]",
    r"UNCHANGED (aux_svc + rep_view_number[1])",
    r"step_action = TimerSendSVC \/ step_action = ReceiveHigherSVC \/ step_action = ReceiveMatchingSVC \/ step_action = SendDVC \/ step_action = ReceiveHigherDVC "
    r"\/ step_action = ReceiveMatchingDVC \/ step_action = SendSV \/ step_action = ReceiveSV \/ step_action = ReceiveClientRequest \/ step_action = ReceivePrepareMsg "
    r"\/ step_action = ReceivePrepareOkMsg \/ step_action = ExecuteOp \/ step_action = SendGetState \/ step_action = ReceiveGetState \/ step_action /= ReceiveNewState",
    "LOCAL Grew == \\E r \\in replicas : Len(rep_log[r])' > Len(rep_log[r])\nA == Grew => step_action # TimerSendSVC\nB == (aux_svc = 1)' /\\ A\n",
]
PRIMED = [t for t in ACCEPTED if "'" in t or "UNCHANGED" in t or "step_action" in t]


@pytest.mark.parametrize("text", ACCEPTED)
def test_accepts(vt, m, text):
    w = m.compile_step(text)
    assert w.step is True and w.describe()["step"] is True


@pytest.mark.parametrize("text", PRIMED)
def test_the_state_compiler_still_refuses_every_one_of_them(vt, m, text):
    with pytest.raises(vt.VsrmcError) as e:
        m.compile_where(text)
    assert e.value.code == -1 and re.match(r"^\d+:\d+: ", e.value.message), e.value.message
    if "'" in text and "UNCHANGED" not in text and "step_action" not in text:
        assert "primed" in e.value.message


REFUSED = [
    ("double prime", r"\E r \in replicas : rep_view_number''[r] = 1", "double prime"),
    ("double prime", r"\E r \in replicas : rep_view_number'[r]' = 1", "double prime"),
    ("prime of a primed expression", r"(aux_svc' = 1)'", "double prime"),
    ("prime of a primed expression", r"(\E m \in DOMAIN messages' : messages'[m] = 1)'", "double prime"),
    ("prime of a definition that has one", "LOCAL A == aux_svc' = 1\nB == A'", "double prime"),
    ("UNCHANGED of a primed expression", r"UNCHANGED aux_svc'", "double prime"),
    ("cross-bag key", r"\E m \in DOMAIN messages : messages'[m] = 1", "other bag"),
    ("cross-bag key", r"\E m \in DOMAIN messages' : messages[m] = 1", "other bag"),
    ("cross-bag key", r"(\E m \in DOMAIN messages : TRUE) /\ (\E m \in DOMAIN messages' : messages[m]' = 1 /\ messages[m] = 1)", "other bag"),
    ("cross-bag membership", r"\E m \in DOMAIN messages : m \in DOMAIN messages'", "search the bag"),
    ("three message quantifiers across bags", r"\E a \in DOMAIN messages : \E b \in DOMAIN messages' : \E c \in DOMAIN messages : a.dest = c.dest", "at most two"),
    ("step_action is not an integer", r"step_action = 1", "type mismatch"),
    ("step_action is not ordered", r"step_action < ReceiveSV", "type mismatch"),
    ("UNCHANGED messages", r"UNCHANGED messages", "UNCHANGED messages"),
    ("UNCHANGED of another whole variable", r"UNCHANGED rep_client_table", "UNCHANGED rep_client_table"),
    ("a primed function", r"messages' = messages", "is a function"),
    ("temporal", r"[](\A r \in replicas : rep_view_number'[r] >= rep_view_number[r])", "temporal"),
    ("temporal", r"<>(aux_svc' = 1)", "temporal"),
    ("ENABLED", r"ENABLED (aux_svc' = 1)", "ENABLED"),
    ("type mismatch", r"\E r \in replicas : rep_status'[r] = 1", "type mismatch"),
    ("unknown identifier", r"rep_statu'[1] = Normal", "unknown identifier"),
]


@pytest.mark.parametrize("what,text,needle", REFUSED, ids=[r[0].replace(" ", "_") + str(i) for i, r in enumerate(REFUSED)])
def test_refuses_with_a_position(vt, m, what, text, needle):
    with pytest.raises(vt.VsrmcError) as e:
        m.compile_step(text)
    assert e.value.code == -1, e.value.message
    assert re.match(r"^\d+:\d+: ", e.value.message), e.value.message
    assert needle in e.value.message, e.value.message


def test_positions_point_at_the_token(vt, m):
    with pytest.raises(vt.VsrmcError) as e:
        m.compile_step("A == TRUE\nB == \\E r \\in replicas :\n     rep_view_number''[r] = 1\n")
    assert e.value.message.startswith("3:22: "), e.value.message               # the second '


@pytest.mark.parametrize("text", STATE_ACCEPTED)
def test_an_unprimed_text_compiles_to_the_same_program_through_both_entries(vt, m, text):
    a, b = m.compile_where(text).describe(), m.compile_step(text).describe()
    assert a["step"] is False and b["step"] is True
    assert {k: v for k, v in a.items() if k != "step"} == {k: v for k, v in b.items() if k != "step"}


def test_describe(vt, m):
    # the program of test_where_cpu.test_describe, with one side primed: the same shape, the same size
    d = m.compile_step(r"\E r1, r2 \in replicas : rep_view_number'[r1] # rep_view_number[r2]").describe()
    assert d["names"] == ["where"] and d["n_bodies"] == 9 and d["msg_loops"] == 0 and d["n_ops"] == 9 * 3 + 8 + 2 and d["depth"] == 4 and d["step"] is True
    # UNCHANGED of a whole per-replica variable: per replica two loads and a compare, an AND between replicas; the OUT and the END
    d = m.compile_step("UNCHANGED rep_commit_number").describe()
    assert d["n_ops"] == 3 * 3 + 2 + 2 and d["depth"] == 3
    d = m.compile_step(r"\E a \in DOMAIN messages : \A b \in DOMAIN messages' : a.dest = b.dest /\ step_action = SendSV").describe()
    assert d["msg_loops"] == 2 and d["n_bodies"] == 2


def test_symmetry_still_refuses_model_value_literals(vt):
    sym = vt.Model.from_constants(R=3, C_=1, n=2, L=2, symmetry=True)
    with pytest.raises(vt.VsrmcError) as e:
        sym.compile_step(r"\E r \in replicas : rep_log'[r][1].operation = v1")
    assert e.value.code == -1 and "SYMMETRY" in e.value.message
    sym.compile_step(r"\E v \in Values : \E r \in replicas : rep_log'[r][1].operation = v /\ rep_log[r][1].operation # v")


def test_analysis_models_are_refused(vt):
    for other in (vt.Model.second_model(R=2, n=2, L=2), vt.Model.third_model(R=2, n=2, L=2)):
        with pytest.raises(vt.VsrmcError) as e:
            other.compile_step("TRUE")
        assert e.value.code == -1 and e.value.message == "step predicates: VSR.tla only"


def test_example_file_compiles(vt, m):
    w = m.compile_step(open(os.path.join(ROOT, "tools", "steps_example.txt")).read())
    assert w.names == ["ViewMonotonic", "CommitMonotonic", "LogNeverShrinks", "LogPrefixStable", "CommittedPrefixStable", "ReceiveSVShrinksLog",
                       "OtherActionShrinksLog", "TimerKeepsLogs"]
    assert w.step and w.describe()["msg_loops"] == 0


def test_program_past_the_caps_is_a_representation_error(vt):
    m5 = vt.Model.from_constants(R=5, C_=1, n=2, L=2)
    big = r"\E a, b, c, d \in replicas : rep_view_number'[a] + rep_view_number[b] < rep_view_number'[c] + rep_view_number[d]"   # 625 bodies of 9 ops
    with pytest.raises(vt.VsrmcError) as e:
        m5.compile_step(big)
    assert e.value.code == -5 and "4096" in e.value.message
    deep = "rep_view_number'[1]" + "".join(" + (rep_view_number'[1]" for _ in range(40)) + ")" * 40 + " = 1"
    with pytest.raises(vt.VsrmcError) as e:
        m5.compile_step(deep)
    assert e.value.code == -5 and "depth" in e.value.message
    with pytest.raises(vt.VsrmcError) as e:
        m5.compile_step("\n".join("P%d == aux_svc' = %d" % (k, k) for k in range(9)))
    assert e.value.code == -1 and "more than 8" in e.value.message


def test_programs_are_refused_by_the_other_kind_of_entry_point(vt, m):
    """the argument checks come before any device work: both directions fail with VSRMC_E_ARG, with or without a device"""
    import numpy as np
    rec = m.init_state()
    off = np.array([0, len(rec)], dtype=np.uint64)
    with pytest.raises(vt.VsrmcError) as e:
        m.where_flags(m.compile_step("aux_svc' = aux_svc"), rec, off)
    assert e.value.code == -1 and "step program" in e.value.message
    with pytest.raises(vt.VsrmcError) as e:
        m.step_flags(m.compile_where("TRUE"), rec, off)
    assert e.value.code == -1 and "vsrmc_step_compile" in e.value.message
    other = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
    with pytest.raises(vt.VsrmcError) as e:
        other.step_flags(m.compile_step("aux_svc' = aux_svc"), other.init_state(), np.array([0, len(other.init_state())], dtype=np.uint64))
    assert e.value.code == -1 and "another model" in e.value.message
