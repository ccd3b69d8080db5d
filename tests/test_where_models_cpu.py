"""State predicates on the two analysis models, host side (`-m "not gpu"`): the language csrc/vsr_where_parse.hpp accepts and refuses for
VR_STATE_TRANSFER.tla and VR_APP_STATE.tla, through Model.compile_predicates — no device is needed to compile.  What the compiled programs compute is
checked on the GPU (test_where_models_gpu.py) against tests/where_models_reference.py."""
import os
import re

import pytest

import where_models_reference as wm
from test_where_cpu import ACCEPTED as VSR_ACCEPTED

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


# between them: every construct both analysis models accept
ACCEPTED = [
    r"TRUE",
    r"(TRUE => FALSE) <=> (FALSE /\ ~TRUE) \/ FALSE",
    r"1 + 2 - 3 = 0 /\ 7 \div 2 = 3 /\ 1 \div 0 = 0",
    r"ReplicaCount = 3 /\ StartViewOnTimerLimit =< 2 /\ NoProgressChangeLimit = 0 /\ Cardinality(Values) # 0",
    r"\A r \in replicas : rep_status[r] = Normal \/ rep_status[r] = ViewChange \/ rep_status[r] # StateTransfer",
    r"\E r1, r2 \in replicas : rep_view_number[r1] < rep_view_number[r2] /\ rep_op_number[r1] >= rep_commit_number[r2] /\ rep_last_normal_view[r1] <= 3",
    r"\E r \in replicas : rep_sent_dvc[r] /\ ~rep_sent_sv[r] /\ no_progress[r] = FALSE",
    r"\A r, p \in replicas : rep_peer_op_number[r][p] <= 3",
    r"\E r \in replicas : Len(rep_log[r]) = 2 /\ rep_log[r][1].operation # Nil /\ rep_log[r][1] = rep_log[r][2]",
    r"\E r1, r2 \in replicas : \E i \in DOMAIN rep_log[r1] : i \in DOMAIN rep_log[r2] /\ rep_log[r1][i] # rep_log[r2][i]",
    r"\E v \in Values : \E r \in replicas : \E i \in 1..3 : rep_log[r][i].operation = v",
    r"no_progress_ctr = 0 /\ aux_svc <= StartViewOnTimerLimit /\ (\A v \in Values : v \in DOMAIN aux_client_acked => (aux_client_acked[v] \/ ~aux_client_acked[v]))",
    r"\E m \in DOMAIN messages : m.type = GetStateMsg /\ m.dest = AnyDest /\ messages[m] >= 1 /\ rep_view_number[m.dest] = 0 - 1",
    r"\A m \in DOMAIN messages : m.source # m.dest /\ m.op_number >= m.commit_number /\ m.last_normal_vn <= m.view_number /\ m.first_op <= 3",
    r"\E m \in DOMAIN messages : m.type = PrepareMsg /\ m.message = rep_log[m.source][m.op_number] /\ aux_client_acked[m.message.operation]",
    r"\E m1, m2 \in DOMAIN messages : m1.type = DoViewChangeMsg /\ m2.type = StartViewChangeMsg /\ m1.dest = m2.dest",
    r"\A m \in DOMAIN messages : m.type = PrepareOkMsg \/ m.type = StartViewMsg \/ m.type = NewStateMsg \/ m.type # PrepareMsg",
    r"\E m \in DOMAIN messages : Len(m.log) >= 1 /\ 2 \in DOMAIN m.log /\ m.log[2].operation # Nil /\ m.log[1] = rep_log[m.dest][1]",
    r"\E m \in DOMAIN messages : (\A i \in DOMAIN m.log : m.log[i] = rep_log[m.source][i]) /\ (\E j \in DOMAIN m.log : m.log[j].operation = m.message.operation)",
    "\\* a comment line\nTRUE (* a (* nested *) comment *) /\\ TRUE",
    "LOCAL Two == 2\nA == \\E r \\in replicas : rep_view_number[r] > Two\nB == ~A \\/ A\n",
]
# VR_APP_STATE.tla only
ACCEPTED_THIRD = [
    r"\E r1, r2 \in replicas : Len(rep_app_state[r1]) > Len(rep_log[r2])",
    r"\A r \in replicas : \A i \in DOMAIN rep_app_state[r] : rep_app_state[r][i] = rep_log[r][i] /\ rep_app_state[r][i].operation # Nil /\ i \in DOMAIN rep_app_state[r]",
    r"\E r \in replicas : Cardinality(rep_recv_dvc[r]) >= 2",
    r"\E r \in replicas : \E d \in rep_recv_dvc[r] : d.type = DoViewChangeMsg /\ d.view_number = rep_view_number[r] /\ d.source # r /\ d.dest = r"
    r" /\ d.last_normal_vn <= d.view_number /\ d.op_number >= d.commit_number",
    r"\E r \in replicas : \A d1, d2 \in rep_recv_dvc[r] : Len(d1.log) = Len(d2.log) /\ (\A i \in DOMAIN d1.log : i \in DOMAIN d2.log /\ d1.log[i] = d2.log[i])",
    r"\E m \in DOMAIN messages : \E d \in rep_recv_dvc[m.dest] : d.source = m.source /\ d.log[1].operation = m.log[1].operation",
]


@pytest.mark.parametrize("which", wm.MODELS)
@pytest.mark.parametrize("text", ACCEPTED)
def test_accepts(models, which, text):
    models[which].compile_predicates(text)


@pytest.mark.parametrize("text", ACCEPTED_THIRD)
def test_third_model_accepts(models, text):
    models["third"].compile_predicates(text)


# one per bullet of the refusal list; the needle of a name the model does not have is the model's own name
REFUSED = [
    ("clients", r"\E c \in clients : TRUE", "{spec} has no clients"),
    ("ClientCount", r"ClientCount = 1", "{spec} has no clients"),
    ("rep_client_table", r"rep_client_table[1][1].executed", "{spec} has no clients"),
    ("rep_svc_recv", r"Cardinality(rep_svc_recv[1]) = 0", "not a variable of {spec}"),
    ("rep_dvc_recv", r"Cardinality(rep_dvc_recv[1]) = 0", "not a variable of {spec}"),
    ("Recovering", r"\E r \in replicas : rep_status[r] = Recovering", "not a status of {spec}"),
    ("aux_restart", r"aux_restart = 0", "cfg of {spec}"),
    ("rep_rec_number", r"rep_rec_number[1] = 0", "cfg of {spec}"),
    ("rep_rec_recv", r"Cardinality(rep_rec_recv[1]) = 0", "cfg of {spec}"),
    ("prime", r"\E r \in replicas : rep_view_number'[r] = 1", "primed"),
    ("UNCHANGED", r"UNCHANGED rep_status", "UNCHANGED"),
    ("step_action", r"step_action = SendSV", "not built for {spec}"),
    ("temporal", r"[](\A r \in replicas : rep_status[r] = Normal)", "temporal"),
    ("entry field", r"\E r \in replicas : rep_log[r][1].view_number = 1", "[operation |-> v]"),
    ("entry field of a message", r"\E m \in DOMAIN messages : m.message.request_number = 1", "[operation |-> v]"),
    ("whole log", r"\E m \in DOMAIN messages : m.log = rep_log[1]", "whole log"),
    ("three message quantifiers", r"\E a \in DOMAIN messages : \E b \in DOMAIN messages : \E c \in DOMAIN messages : a.dest = c.dest", "at most two"),
    ("unknown identifier", r"rep_statu[1] = Normal", "unknown identifier"),
    ("type mismatch", r"\E r \in replicas : rep_status[r] = 1", "type mismatch"),
    ("entry against a value", r"\E r \in replicas : rep_log[r][1] = Nil", "type mismatch"),
    ("CHOOSE", r"(CHOOSE r \in replicas : TRUE) = 1", "CHOOSE"),
    ("set constructor", r"\E r \in {1, 2} : rep_status[r] = Normal", "constructors"),
    ("other set", r"\E x \in DOMAIN aux_client_acked : TRUE", "a quantifier ranges over"),
    ("mixed junctions", r"TRUE /\ FALSE \/ TRUE", "mixed"),
    ("more than 8 exports", "\n".join("P%d == TRUE" % k for k in range(9)), "more than 8"),
]
SPEC = {"second": "VR_STATE_TRANSFER.tla", "third": "VR_APP_STATE.tla"}


@pytest.mark.parametrize("which", wm.MODELS)
@pytest.mark.parametrize("what,text,needle", REFUSED, ids=[r[0].replace(" ", "_") + str(i) for i, r in enumerate(REFUSED)])
def test_refuses_with_a_position(vt, models, which, what, text, needle):
    with pytest.raises(vt.VsrmcError) as e:
        models[which].compile_predicates(text)
    assert e.value.code == -1, e.value.message
    assert re.match(r"^\d+:\d+: ", e.value.message), e.value.message
    assert needle.format(spec=SPEC[which]) in e.value.message, e.value.message


def test_app_state_and_held_dvcs_exist_on_the_third_model_only(vt, models):
    for text in (r"\E r \in replicas : Len(rep_app_state[r]) = 1", r"\E r \in replicas : rep_app_state[r][1].operation # Nil",
                 r"\E r \in replicas : Cardinality(rep_recv_dvc[r]) = 1", r"\E r \in replicas : \E d \in rep_recv_dvc[r] : d.source = 1",
                 r"\E r \in replicas : \E i \in DOMAIN rep_app_state[r] : i = 1"):
        models["third"].compile_predicates(text)
        with pytest.raises(vt.VsrmcError) as e:
            models["second"].compile_predicates(text)
        assert e.value.code == -1 and re.match(r"^1:\d+: unknown identifier rep_(app_state|recv_dvc)", e.value.message), e.value.message


def test_positions_point_at_the_token(vt, models):
    with pytest.raises(vt.VsrmcError) as e:
        models["second"].compile_predicates("A == TRUE\nB == \\E r \\in replicas :\n     rep_status[r] = Recovering\n")
    assert e.value.message.startswith("3:22: "), e.value.message


def test_caps_carry_over(vt):
    m5 = vt.Model.second_model(R=5, n=2, L=2)
    big = r"\E a, b, c, d \in replicas : rep_view_number[a] + rep_view_number[b] < rep_view_number[c] + rep_view_number[d]"
    with pytest.raises(vt.VsrmcError) as e:
        m5.compile_predicates(big)
    assert e.value.code == -5 and "4096" in e.value.message
    deep = "rep_view_number[1]" + "".join(" + (rep_view_number[1]" for _ in range(40)) + ")" * 40 + " = 1"
    with pytest.raises(vt.VsrmcError) as e:
        m5.compile_predicates(deep)
    assert e.value.code == -5 and "depth" in e.value.message


def test_model_value_literals_and_symmetry(vt, models):
    """The analysis models are never loaded with SYMMETRY (their constructors refuse it), so a value may be named there; the rule itself is the
    generic entry's as it is the old one's"""
    models["second"].compile_predicates(r"\E r \in replicas : rep_log[r][1].operation = v1")
    models["third"].compile_predicates(r"\E r \in replicas : rep_log[r][1].operation = a")
    with pytest.raises(vt.VsrmcError) as e:
        models["third"].compile_predicates(r"\E r \in replicas : rep_log[r][1].operation = v1")      # (this model's values are a, b)
    assert "unknown identifier v1" in e.value.message
    text = r"\E r \in replicas : rep_log[r][1].operation = v1"
    sym = vt.Model.from_constants(R=3, C_=1, n=2, L=2, symmetry=True)
    with pytest.raises(vt.VsrmcError) as e:
        sym.compile_predicates(text)
    assert e.value.code == -1 and "SYMMETRY" in e.value.message and re.match(r"^1:\d+: ", e.value.message)
    vt.Model.from_constants(R=3, C_=1, n=2, L=2, symmetry=False).compile_predicates(text)
    with pytest.raises(vt.VsrmcError):
        vt.Model.second_model(R=3, n=2, L=2, symmetry=True)


@pytest.mark.parametrize("text", VSR_ACCEPTED)
def test_generic_entry_on_vsr_tla_is_the_old_entry(vt, text):
    m = vt.Model.from_constants(R=3, C_=1, n=2, L=2)
    a, b = m.compile_where(text).describe(), m.compile_predicates(text).describe()
    assert a == b and not b["step"]
    with pytest.raises(vt.VsrmcError) as e:                         # and its refusals are the old entry's: nothing of the analysis models leaks in
        m.compile_predicates(r"\E m \in DOMAIN messages : m.log = 1")
    assert "m.log is not supported" in e.value.message
    for name in ("StateTransfer", "AnyDest", "no_progress_ctr"):
        with pytest.raises(vt.VsrmcError) as e:
            m.compile_predicates("%s = %s" % (name, name))
        assert "unknown identifier " + name in e.value.message


def test_describe(models):
    w = models["second"].compile_predicates(r"\E r1, r2 \in replicas : rep_view_number[r1] # rep_view_number[r2]")
    d = w.describe()
    assert d["names"] == ["where"] and d["n_bodies"] == 9 and d["msg_loops"] == 0 and d["n_ops"] == 9 * 3 + 8 + 2 and d["depth"] == 4 and not d["step"]
    # a held DoViewChange unfolds over the three source slots: no loop remains (9 bodies of the inner quantifier, 3 of the outer)
    d = models["third"].compile_predicates(r"\E r \in replicas : \E d \in rep_recv_dvc[r] : d.op_number = 1").describe()
    assert d["n_bodies"] == 9 + 3 and d["msg_loops"] == 0


def test_example_files_compile(models):
    w = models["second"].compile_predicates(open(os.path.join(ROOT, "tools", "predicates_model2_example.txt")).read())
    assert w.names == ["InStateTransfer", "GetStateToAny", "DvcLogBelowCommit", "SvLogDropsEntry", "LogDivergence", "CountedDvc", "NewStateCarriesV2"]
    w = models["third"].compile_predicates(open(os.path.join(ROOT, "tools", "predicates_model3_example.txt")).read())
    assert w.names == ["InStateTransfer", "GetStateToAny", "DvcLogBelowCommit", "SvLogDropsEntry", "LogDivergence", "AppAheadOfSomeLog", "TwoDvcsHeld",
                       "HeldDvcShorterLog"]


def test_reference_sets_compile(models):
    """the texts the GPU tests evaluate (tests/where_models_reference.py) are in the language"""
    for which, values in (("second", ("v1", "v2")), ("third", ("a", "b"))):
        assert models[which].compile_predicates(wm.text_of(wm.set_a(values))).names == [p[0] for p in wm.set_a(values)]
        assert models[which].compile_predicates(wm.text_of(wm.SET_B)).names == [p[0] for p in wm.SET_B]
    assert models["third"].compile_predicates(wm.text_of(wm.SET_A3)).names == [p[0] for p in wm.SET_A3]
    assert models["third"].compile_predicates(wm.text_of(wm.SET_B3)).names == [p[0] for p in wm.SET_B3]
    for which in wm.MODELS:
        preds = wm.random_predicates(20261018, 3, 1, 104, third=which == "third")
        m = (models[which].__class__.second_model if which == "second" else models[which].__class__.third_model)(R=3, n=2, L=1)
        for j in range(0, len(preds), 8):
            m.compile_predicates("\n".join("P%d == %s" % (k, t) for k, (t, _) in enumerate(preds[j: j + 8])))


def test_a_program_is_its_models_own(vt, models):
    """the two analysis models with equal constants are different models; so is VSR.tla.  The batch entry looks at the program before it looks for a
    device, so the refusal shows without one; the matching pair computes where a device is visible and fails with VSRMC_E_HIP where none is"""
    import numpy as np
    vsr = vt.Model.from_constants(R=3, C_=1, n=2, L=2, symmetry=False)
    progs = {"second": models["second"].compile_predicates("TRUE"), "third": models["third"].compile_predicates("TRUE"), "vsr": vsr.compile_predicates("TRUE")}
    ms = dict(models, vsr=vsr)
    have_device = vt.load().vsrmc_device_count() > 0
    for a in progs:
        for b in ms:
            rec = ms[b].init_state()
            off = np.array([0, len(rec)], dtype=np.uint64)
            if a == b and have_device:
                assert [int(x) for x in ms[b].where_flags(progs[a], rec, off)] == [1]
                continue
            with pytest.raises(vt.VsrmcError) as e:
                ms[b].where_flags(progs[a], rec, off)
            if a == b:
                assert e.value.code == -3
            else:
                assert e.value.code == -1 and "compiled for another model" in e.value.message, (a, b)
