"""Step predicates on the two analysis models, host side (`-m "not gpu"`): what csrc/vsr_where_parse.hpp accepts and refuses for VR_STATE_TRANSFER.tla and
VR_APP_STATE.tla through Model.compile_step_predicates — primes over the models' own variable table, UNCHANGED, step_action — that the entry is
Model.compile_step on a VSR.tla model, and that the older entries refuse what they refused.  No device is needed to compile.  What the compiled programs
compute is checked on the GPU (test_step_models_gpu.py) against tests/step_models_reference.py."""
import os
import re

import numpy as np
import pytest

import step_models_reference as sm
from test_step_cpu import ACCEPTED as VSR_STEP_ACCEPTED
from test_where_models_cpu import ACCEPTED as STATE_ACCEPTED, ACCEPTED_THIRD as STATE_ACCEPTED_THIRD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


@pytest.fixture(scope="module")
def models(vt):
    return {"second": vt.Model.second_model(R=3, n=2, L=2), "third": vt.Model.third_model(R=3, n=2, L=2)}


# between them: every primed construct both analysis models accept
ACCEPTED = [t for _, t, _ in sm.SIX + sm.SET_B + sm.SET_C + sm.NEIGHBOUR] + [
    sm.COMMIT_MONOTONIC, sm.COUNT_GOES_DOWN,
    r"\A r \in replicas : rep_status'[r] = rep_status[r] \/ no_progress'[r] \/ no_progress_ctr' > no_progress_ctr \/ rep_last_normal_view[r]' > 0",
    r"\E r \in replicas : rep_sent_dvc'[r] /\ ~rep_sent_dvc[r] /\ rep_sent_sv[r]' = rep_sent_sv[r]",
    r"\A r, p \in replicas : rep_peer_op_number'[r][p] >= rep_peer_op_number[r][p]",
    r"aux_svc' >= aux_svc /\ (\A v \in Values : aux_client_acked'[v] \/ ~aux_client_acked[v])",
    r"\E r \in replicas : rep_log'[r][1].operation # rep_log[r][1].operation /\ Len(rep_log'[r]) = 1 /\ Len(rep_log[r])' = 1 /\ 2 \in DOMAIN rep_log'[r]",
    r"\E r \in replicas : \E i \in DOMAIN rep_log'[r] : ~(i \in DOMAIN rep_log[r]) /\ rep_log'[r][i] = rep_log[r][1]",
    r"(\A r \in replicas : rep_view_number[r] = 1 /\ ReplicaCount = 3 /\ rep_status[r] # StateTransfer)'",
    r"(\E m \in DOMAIN messages : messages[m] = 2 /\ rep_view_number[m.dest] = m.view_number /\ Len(m.log) = 1)'",
    r"\E m \in DOMAIN messages' : \E n \in DOMAIN messages' : m.dest = n.source /\ messages'[m] > messages'[n] /\ m.log[1] = n.log[1]",
    r"\E m \in DOMAIN messages' : m.type = PrepareMsg /\ m.message = rep_log'[m.dest][m.op_number] /\ m.dest # AnyDest",
    r"\E m \in DOMAIN messages' : m.type = NewStateMsg /\ (\A i \in DOMAIN m.log : m.log[i].operation = rep_log[m.source][i].operation) /\ Len(m.log) >= 1",
    r"UNCHANGED rep_status /\ UNCHANGED rep_view_number /\ UNCHANGED rep_op_number /\ UNCHANGED rep_commit_number /\ UNCHANGED rep_last_normal_view /\ UNCHANGED rep_log "
    r"/\ UNCHANGED no_progress",
    r"\A r \in replicas : UNCHANGED rep_status[r] /\ UNCHANGED rep_sent_dvc[r] /\ UNCHANGED Len(rep_log[r]) /\ UNCHANGED rep_log[r][2] /\ UNCHANGED rep_log[r][1].operation "
    r"/\ UNCHANGED rep_log[r] /\ UNCHANGED no_progress[r] /\ UNCHANGED rep_peer_op_number[r][1]",
    r"\A v \in Values : UNCHANGED aux_client_acked[v]",
    r"UNCHANGED (aux_svc + rep_view_number[1]) /\ UNCHANGED no_progress_ctr",
    r"\A m \in DOMAIN messages : UNCHANGED rep_log[m.source]",
    r"step_action = TimerSendSVC \/ step_action = ReceiveHigherSVC \/ step_action = ReceiveMatchingSVC \/ step_action = SendDVC \/ step_action = ReceiveHigherDVC "
    r"\/ step_action = ReceiveMatchingDVC \/ step_action = SendSV \/ step_action = ReceiveSV \/ step_action = ReceiveClientRequest \/ step_action = ReceivePrepareMsg "
    r"\/ step_action = ReceivePrepareOkMsg \/ step_action = ExecuteOp \/ step_action = SendGetState \/ step_action = ReceiveGetState \/ step_action /= ReceiveNewState",
    "LOCAL Grew == \\E r \\in replicas : Len(rep_log[r])' > Len(rep_log[r])\nA == Grew => step_action # TimerSendSVC\nB == (aux_svc = 1)' /\\ A\n",
]
# VR_APP_STATE.tla only
ACCEPTED_THIRD = [t for _, t, _ in sm.SET_3 + sm.NEIGHBOUR_3] + [
    sm.HELD_DROPPED, sm.HELD_UNCHANGED,
    r"\E r \in replicas : Len(rep_app_state'[r]) > Len(rep_app_state[r]) /\ Len(rep_app_state[r])' = 1 /\ rep_app_state'[r][1].operation # Nil /\ 1 \in DOMAIN rep_app_state'[r]",
    r"\A r \in replicas : \A i \in DOMAIN rep_app_state'[r] : rep_app_state[r][i]' = rep_log'[r][i]",
    r"\E r \in replicas : Cardinality(rep_recv_dvc[r])' > Cardinality(rep_recv_dvc'[r]) - 1",
    r"\E r \in replicas : \E d \in rep_recv_dvc'[r] : d.type = DoViewChangeMsg /\ d.view_number = rep_view_number'[r] /\ d.source # r /\ d.dest = r"
    r" /\ d.last_normal_vn <= d.view_number /\ d.op_number >= d.commit_number /\ Len(d.log) <= 3 /\ (\A i \in DOMAIN d.log : d.log[i] = rep_log[d.source][i])",
    r"\A r \in replicas : \A d \in rep_recv_dvc'[r] : \E e \in rep_recv_dvc[r] : e.source = d.source /\ e.log[1] = d.log[1]",
    r"\E m \in DOMAIN messages : \E d \in rep_recv_dvc'[m.dest] : d.source = m.source /\ d.log[1].operation = m.log[1].operation",
    r"UNCHANGED rep_app_state /\ (\A r \in replicas : UNCHANGED rep_app_state[r] /\ UNCHANGED rep_app_state[r][1] /\ UNCHANGED Cardinality(rep_recv_dvc[r]))",
]
PRIMED = [t for t in ACCEPTED if "'" in t or "UNCHANGED" in t or "step_action" in t]


@pytest.mark.parametrize("which", sm.MODELS)
@pytest.mark.parametrize("text", ACCEPTED)
def test_accepts(models, which, text):
    w = models[which].compile_step_predicates(text)
    assert w.step is True and w.describe()["step"] is True


@pytest.mark.parametrize("text", ACCEPTED_THIRD)
def test_third_model_accepts(vt, models, text):
    assert models["third"].compile_step_predicates(text).step is True
    with pytest.raises(vt.VsrmcError) as e:                          # rep_app_state and rep_recv_dvc are unknown identifiers on VR_STATE_TRANSFER.tla
        models["second"].compile_step_predicates(text)
    assert e.value.code == -1 and "unknown identifier rep_" in e.value.message


@pytest.mark.parametrize("which", sm.MODELS)
def test_every_set_of_the_gpu_tests_compiles(models, which):
    for tag, preds in sm.sets(which) + [("N", sm.neighbour(which))]:
        w = models[which].compile_step_predicates(sm.text_of(preds))
        assert w.names == [p[0] for p in preds] and w.step, tag
    d = models[which].compile_step_predicates(sm.NEW_STATE_APPEARS).describe()
    assert d["msg_loops"] == 2 and d["n_bodies"] == 5                # two loops, one over each bag, and \A i \in 1..3 unfolded inside the inner one


@pytest.mark.parametrize("which", sm.MODELS)
@pytest.mark.parametrize("text", STATE_ACCEPTED)
def test_an_unprimed_text_compiles_to_the_same_program_through_both_entries(models, which, text):
    a, b = models[which].compile_predicates(text).describe(), models[which].compile_step_predicates(text).describe()
    assert a["step"] is False and b["step"] is True
    assert {k: v for k, v in a.items() if k != "step"} == {k: v for k, v in b.items() if k != "step"}


@pytest.mark.parametrize("text", STATE_ACCEPTED_THIRD)
def test_an_unprimed_text_of_the_third_model_too(models, text):
    a, b = models["third"].compile_predicates(text).describe(), models["third"].compile_step_predicates(text).describe()
    assert {k: v for k, v in a.items() if k != "step"} == {k: v for k, v in b.items() if k != "step"} and b["step"] is True


@pytest.mark.parametrize("text", VSR_STEP_ACCEPTED)
def test_on_a_vsr_tla_model_the_entry_is_compile_step(vt, text):
    m = vt.Model.from_constants(R=3, C_=1, n=2, L=2)
    assert m.compile_step_predicates(text).describe() == m.compile_step(text).describe()


def test_describe(models):
    # UNCHANGED of a whole per-replica variable: per replica two loads and a compare, an AND between replicas; the OUT and the END
    for which in sm.MODELS:
        d = models[which].compile_step_predicates("UNCHANGED rep_commit_number").describe()
        assert d["n_ops"] == 3 * 3 + 2 + 2 and d["depth"] == 3 and d["step"] is True
        assert models[which].compile_step_predicates("UNCHANGED no_progress").describe()["n_ops"] == 3 * 3 + 2 + 2
        # a log of one replica: the length and the three positions, each side a load and a normalising op
        d = models[which].compile_step_predicates("UNCHANGED rep_log[2]").describe()
        assert d["n_ops"] == 4 * 5 + 3 + 2
        assert models[which].compile_step_predicates("UNCHANGED rep_log").describe()["n_ops"] == 3 * (4 * 5 + 3) + 2 + 2
    # the application state: the length is the commit number (one load a side), an entry is one op a side
    d = models["third"].compile_step_predicates("UNCHANGED rep_app_state[2]").describe()
    assert d["n_ops"] == 4 * 3 + 3 + 2


@pytest.mark.parametrize("which", sm.MODELS)
@pytest.mark.parametrize("text", PRIMED)
def test_the_state_entry_still_refuses_every_one_of_them(vt, models, which, text):
    with pytest.raises(vt.VsrmcError) as e:
        models[which].compile_predicates(text)
    assert e.value.code == -1 and re.match(r"^\d+:\d+: ", e.value.message), e.value.message
    if "'" in text and "UNCHANGED" not in text and "step_action" not in text:
        assert "primed" in e.value.message


# (what, text, needle, models it is refused so on)
BOTH = ("second", "third")
REFUSED = [
    ("double prime", r"\E r \in replicas : rep_view_number''[r] = 1", "double prime", BOTH),
    ("double prime", r"\E r \in replicas : rep_log'[r]'[1] = rep_log[r][1]", "double prime", BOTH),
    ("double prime", r"\E r \in replicas : Len(rep_log'[r])' = 1", "double prime", BOTH),
    ("prime of a primed expression", r"(no_progress_ctr' = 1)'", "double prime", BOTH),
    ("prime of a primed expression", r"(\E m \in DOMAIN messages' : messages'[m] = 1)'", "double prime", BOTH),
    ("prime of a definition that has one", "LOCAL A == \\E r \\in replicas : no_progress'[r]\nB == A'", "double prime", BOTH),
    ("UNCHANGED of a primed expression", r"UNCHANGED no_progress_ctr'", "double prime", BOTH),
    ("UNCHANGED of a primed log", r"UNCHANGED rep_log'[1]", "double prime", BOTH),
    ("prime of a held set inside a primed expression", r"(\E d \in rep_recv_dvc'[1] : d.source = 2)'", "double prime", ("third",)),
    ("a bound variable cannot be primed", r"\E d \in rep_recv_dvc[1] : d'.source = 2", "bound variable", ("third",)),
    ("a bound variable cannot be primed", r"\E m \in DOMAIN messages : m'.log[1] = rep_log[1][1]", "bound variable", BOTH),
    ("cross-bag key", r"\E m \in DOMAIN messages : messages'[m] = 1", "other bag", BOTH),
    ("cross-bag key", r"\E m \in DOMAIN messages' : messages[m] = 1", "other bag", BOTH),
    ("cross-bag membership", r"\E m \in DOMAIN messages : m \in DOMAIN messages'", "search the bag", BOTH),
    ("three message quantifiers across bags", r"\E a \in DOMAIN messages : \E b \in DOMAIN messages' : \E c \in DOMAIN messages : a.dest = c.dest", "at most two", BOTH),
    ("step_action is not an integer", r"step_action = 1", "type mismatch", BOTH),
    ("step_action is not ordered", r"step_action < ReceiveSV", "type mismatch", BOTH),
    ("UNCHANGED messages", r"UNCHANGED messages", "UNCHANGED messages: a whole bag", BOTH),
    ("UNCHANGED rep_recv_dvc", r"UNCHANGED rep_recv_dvc", "UNCHANGED rep_recv_dvc: the sets of held DoViewChanges of VR_APP_STATE.tla", ("third",)),
    ("UNCHANGED of another whole variable", r"UNCHANGED rep_peer_op_number", "UNCHANGED rep_peer_op_number: a whole variable of VR_", BOTH),
    ("UNCHANGED of a variable the model lacks", r"UNCHANGED rep_client_table", "has no clients", BOTH),
    ("a whole log is not a value", r"\E r \in replicas : rep_log'[r] = rep_log[r]", "rep_log[r][i]", BOTH),
    ("a whole log is not a value", r"\E m \in DOMAIN messages' : UNCHANGED m.log", "whole log", BOTH),
    ("a primed function", r"messages' = messages", "is a function", BOTH),
    ("a primed function", r"no_progress' = no_progress", "is a function", BOTH),
    ("a primed function", r"rep_app_state' = rep_app_state", "is a function", ("third",)),
    ("an entry has one field", r"\E r \in replicas : rep_log'[r][1].view_number = 1", "VR_", BOTH),
    ("a name of VSR.tla", r"\E r \in replicas : rep_status'[r] = Recovering", "not a status of VR_", BOTH),
    ("a name of VSR.tla", r"\A r \in replicas : Cardinality(rep_dvc_recv'[r]) = 0", "is not a variable of VR_", BOTH),
    ("temporal", r"[](\A r \in replicas : rep_view_number'[r] >= rep_view_number[r])", "temporal", BOTH),
    ("ENABLED", r"ENABLED (aux_svc' = 1)", "ENABLED", BOTH),
    ("type mismatch", r"\E r \in replicas : rep_status'[r] = 1", "type mismatch", BOTH),
    ("unknown identifier", r"rep_statu'[1] = Normal", "unknown identifier", BOTH),
    ("unknown action", r"step_action = ReceiveRecovery", "unknown identifier ReceiveRecovery", BOTH),
]


@pytest.mark.parametrize("what,text,needle,where", REFUSED, ids=[r[0].replace(" ", "_") + str(i) for i, r in enumerate(REFUSED)])
def test_refuses_with_a_position(vt, models, what, text, needle, where):
    for which in where:
        with pytest.raises(vt.VsrmcError) as e:
            models[which].compile_step_predicates(text)
        assert e.value.code == -1, e.value.message
        assert re.match(r"^\d+:\d+: ", e.value.message), e.value.message
        assert needle in e.value.message, e.value.message


def test_positions_point_at_the_token(vt, models):
    with pytest.raises(vt.VsrmcError) as e:
        models["second"].compile_step_predicates("A == TRUE\nB == \\E r \\in replicas :\n     no_progress''[r]\n")
    assert e.value.message.startswith("3:18: "), e.value.message               # the second '
    with pytest.raises(vt.VsrmcError) as e:
        models["third"].compile_step_predicates("A == TRUE\nB == A /\\\n  UNCHANGED rep_recv_dvc\n")
    assert e.value.message.startswith("3:13: "), e.value.message               # the variable


def test_the_older_entries_keep_refusing(vt, models):
    for which in sm.MODELS:
        for entry in (models[which].compile_step, models[which].compile_where):
            with pytest.raises(vt.VsrmcError) as e:
                entry("TRUE")
            assert e.value.code == -1 and e.value.message.endswith("VSR.tla only")
        with pytest.raises(vt.VsrmcError) as e:
            models[which].compile_predicates("step_action = SendSV")
        assert "step_action belongs to step predicates" in e.value.message


def test_example_files_compile(models):
    w = models["second"].compile_step_predicates(open(os.path.join(ROOT, "tools", "steps_model2_example.txt")).read())
    assert w.names == ["CommitMonotonic", "LogNeverShrinks", "CommittedPrefixStable", "EntersStateTransfer", "NewStateAppears"] and w.step
    w = models["third"].compile_step_predicates(open(os.path.join(ROOT, "tools", "steps_model3_example.txt")).read())
    assert w.names == ["CommitMonotonic", "LogNeverShrinks", "CommittedPrefixStable", "EntersStateTransfer", "NewStateAppears", "AppPrefixStable", "HeldDvcsDropped"]
    assert w.step and w.describe()["msg_loops"] == 2
    assert set(w.names) <= set(sm.EXAMPLE)


def test_a_program_is_refused_by_another_model_and_by_the_state_entry_points(vt, models):
    """the argument checks come before any device work: they fail with VSRMC_E_ARG, with or without a device"""
    second, third = models["second"], models["third"]
    w2 = second.compile_step_predicates("aux_svc' = aux_svc")
    rec2, rec3 = second.init_state(), third.init_state()
    off2, off3 = (np.array([0, len(r)], dtype=np.uint64) for r in (rec2, rec3))
    with pytest.raises(vt.VsrmcError) as e:
        second.where_flags(w2, rec2, off2)
    assert e.value.code == -1 and "step program" in e.value.message
    with pytest.raises(vt.VsrmcError) as e:
        second.step_flags(second.compile_predicates("TRUE"), rec2, off2)
    assert e.value.code == -1 and "vsrmc_step_compile" in e.value.message
    with pytest.raises(vt.VsrmcError) as e:                          # equal constants, another model
        third.step_flags(w2, rec3, off3)
    assert e.value.code == -1 and "another model" in e.value.message
    vsr = vt.Model.from_constants(R=3, C_=1, n=2, L=2, symmetry=False)
    with pytest.raises(vt.VsrmcError) as e:
        vsr.step_flags(w2, vsr.init_state(), np.array([0, len(vsr.init_state())], dtype=np.uint64))
    assert e.value.code == -1 and "another model" in e.value.message
    with pytest.raises(vt.VsrmcError) as e:
        second.step_flags(vsr.compile_step_predicates("aux_svc' = aux_svc"), rec2, off2)
    assert e.value.code == -1 and "another model" in e.value.message
    with pytest.raises(vt.VsrmcError) as e:                          # other constants
        vt.Model.second_model(R=2, n=2, L=2).step_flags(w2, rec2, off2)
    assert e.value.code == -1 and "another model" in e.value.message
