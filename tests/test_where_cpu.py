"""State predicates, host side (`-m "not gpu"`): the language csrc/vsr_where_parse.hpp accepts and refuses, through Model.compile_where — no device
is needed to compile.  What the compiled programs compute is checked on the GPU (test_where_gpu.py) against tests/where_reference.py."""
import re

import pytest


@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


@pytest.fixture(scope="module")
def m(vt):
    return vt.Model.from_constants(R=3, C_=1, n=2, L=2)


# between them: every construct of the language
ACCEPTED = [
    r"TRUE",
    r"FALSE \/ ~TRUE",
    r"(TRUE => FALSE) <=> (FALSE /\ TRUE)",
    r"\lnot (TRUE \land FALSE) \lor FALSE",
    r"1 + 2 - 3 = 0 /\ 7 \div 2 = 3",
    r"ReplicaCount = 3 /\ ClientCount >= 1 /\ StartViewOnTimerLimit =< 2 /\ Cardinality(Values) # 0",
    r"1 < 2 /\ 2 <= 2 /\ 2 =< 3 /\ 3 > 2 /\ 3 >= 3 /\ 1 /= 2 /\ 1 # 2",
    r"\A r \in replicas : rep_status[r] = Normal \/ rep_status[r] = ViewChange \/ rep_status[r] # Recovering",
    r"\E r1, r2 \in replicas : rep_view_number[r1] < rep_view_number[r2]",
    r"\A r \in replicas : rep_op_number[r] >= rep_commit_number[r] /\ rep_last_normal_view[r] <= rep_view_number[r]",
    r"\E r \in replicas : rep_sent_dvc[r] /\ ~rep_sent_sv[r] /\ rep_sent_sv[r] = FALSE",
    r"\A r, p \in replicas : rep_peer_op_number[r][p] <= 3",
    r"\A r \in replicas : \A c \in clients : rep_client_table[r][c].executed \/ rep_client_table[r][c].request_number > rep_client_table[r][c].op_number",
    r"\E r \in replicas : Len(rep_log[r]) = 2 /\ rep_log[r][1].view_number = 1 /\ rep_log[r][2].client_id = 1 /\ rep_log[r][1].request_number = 1",
    r"\E r1, r2 \in replicas : \E i \in DOMAIN rep_log[r1] : i \in DOMAIN rep_log[r2] /\ rep_log[r1][i] # rep_log[r2][i]",
    r"\E v \in Values : \E r \in replicas : \E i \in 1..3 : rep_log[r][i].operation = v /\ rep_log[r][i].operation # Nil",
    r"\A r \in replicas : Cardinality(rep_svc_recv[r]) + Cardinality(rep_dvc_recv[r]) <= 6",
    r"aux_svc <= StartViewOnTimerLimit /\ (\A v \in Values : v \in DOMAIN aux_client_acked => (aux_client_acked[v] \/ ~aux_client_acked[v]))",
    r"\E m \in DOMAIN messages : m.type = StartViewMsg /\ messages[m] >= 1 /\ rep_view_number[m.dest] > m.view_number",
    r"\A m \in DOMAIN messages : m.source # m.dest /\ m.op_number >= m.commit_number /\ m.last_normal_vn <= m.view_number /\ m.first_op <= 3",
    r"\E m \in DOMAIN messages : m.type = PrepareMsg /\ m.message.view_number = m.view_number /\ aux_client_acked[m.message.operation]",
    r"\E m \in DOMAIN messages : m.type = PrepareMsg /\ m.message = rep_log[m.dest][m.op_number]",
    r"\E m1, m2 \in DOMAIN messages : m1.type = DoViewChangeMsg /\ m2.type = StartViewChangeMsg /\ m1.dest = m2.dest",
    r"\A m \in DOMAIN messages : m.type = PrepareOkMsg \/ m.type = GetStateMsg \/ m.type = NewStateMsg \/ m.type # PrepareMsg",
    r"\E i \in 1..ReplicaCount - 1 : i \in replicas /\ i \in 2..3 /\ rep_status[i + 1] = Normal",
    "\\* a comment line\nTRUE (* a (* nested *) comment *) /\\ TRUE",
    "LOCAL Two == 2\nA == \\E r \\in replicas : rep_view_number[r] > Two\nB == ~A \\/ A\n",
]


@pytest.mark.parametrize("text", ACCEPTED)
def test_accepts(vt, m, text):
    m.compile_where(text)


# one per bullet of the refusal list
REFUSED = [
    ("unknown identifier", r"rep_statu[1] = Normal", "unknown identifier"),
    ("unbound variable", r"\E r \in replicas : rep_status[q] = Normal", "unknown identifier q"),
    ("forward reference", "A == B\nB == TRUE", "unknown identifier B"),
    ("recursive reference", "A == ~A", "refers to itself"),
    ("type mismatch", r"\E r \in replicas : rep_status[r] = 1", "type mismatch"),
    ("type mismatch in an index", r"rep_status[TRUE] = Normal", "type mismatch"),
    ("prime", r"\E r \in replicas : rep_view_number'[r] = 1", "primed"),
    ("temporal", r"[](\A r \in replicas : rep_status[r] = Normal)", "temporal"),
    ("temporal", r"<>(aux_svc = 1)", "temporal"),
    ("CHOOSE", r"(CHOOSE r \in replicas : TRUE) = 1", "CHOOSE"),
    ("LAMBDA", r"LAMBDA x : x", "LAMBDA"),
    ("set constructor", r"\E r \in {1, 2} : rep_status[r] = Normal", "constructors"),
    ("other set", r"\E m \in rep_svc_recv[1] : TRUE", "a quantifier ranges over"),
    ("other set", r"\E x \in DOMAIN aux_client_acked : TRUE", "a quantifier ranges over"),
    ("mixed junctions", r"TRUE /\ FALSE \/ TRUE", "mixed"),
    ("three message quantifiers", r"\E a \in DOMAIN messages : \E b \in DOMAIN messages : \E c \in DOMAIN messages : a.dest = c.dest", "at most two"),
    ("more than 8 exports", "\n".join("P%d == TRUE" % k for k in range(9)), "more than 8"),
    ("not a boolean", r"1 + 1", "type mismatch"),
    ("m.log", r"\E m \in DOMAIN messages : m.log = 1", "m.log"),
]


@pytest.mark.parametrize("what,text,needle", REFUSED, ids=[r[0].replace(" ", "_") + str(i) for i, r in enumerate(REFUSED)])
def test_refuses_with_a_position(vt, m, what, text, needle):
    with pytest.raises(vt.VsrmcError) as e:
        m.compile_where(text)
    assert e.value.code == -1, e.value.message
    assert re.match(r"^\d+:\d+: ", e.value.message), e.value.message
    assert needle in e.value.message, e.value.message


def test_positions_point_at_the_token(vt, m):
    with pytest.raises(vt.VsrmcError) as e:
        m.compile_where("A == TRUE\nB == \\E r \\in replicas :\n     rep_status[r] = 1\n")
    assert e.value.message.startswith("3:20: "), e.value.message             # the `=` that compares a status with an integer


def test_program_past_the_caps_is_a_representation_error(vt):
    m5 = vt.Model.from_constants(R=5, C_=1, n=2, L=2)
    big = r"\E a, b, c, d \in replicas : rep_view_number[a] + rep_view_number[b] < rep_view_number[c] + rep_view_number[d]"   # 625 bodies of 9 ops
    with pytest.raises(vt.VsrmcError) as e:
        m5.compile_where(big)
    assert e.value.code == -5 and "4096" in e.value.message
    deep = "1" + "".join(" + (1" for _ in range(40)) + ")" * 40 + " = rep_view_number[1]"      # constants fold: still shallow
    m5.compile_where(deep)
    deep = "rep_view_number[1]" + "".join(" + (rep_view_number[1]" for _ in range(40)) + ")" * 40 + " = 1"
    with pytest.raises(vt.VsrmcError) as e:
        m5.compile_where(deep)
    assert e.value.code == -5 and "depth" in e.value.message


def test_describe(vt, m):
    w = m.compile_where(r"\E r1, r2 \in replicas : rep_view_number[r1] # rep_view_number[r2]")
    d = w.describe()
    assert d["names"] == ["where"] == w.names and d["n_bodies"] == 9 and d["msg_loops"] == 0
    # per body: two loads and a compare, an OR between bodies; the OUT and the END.  Deepest: r1's accumulator, r2's accumulator, the two operands
    assert d["n_ops"] == 9 * 3 + 8 + 2 and d["depth"] == 4
    w = m.compile_where("LOCAL H == 1\nA == \\E m \\in DOMAIN messages : \\A n \\in DOMAIN messages : m.dest = n.dest\nB == \\E m \\in DOMAIN messages : rep_view_number[m.dest] = H")
    d = w.describe()
    assert d["names"] == ["A", "B"] and d["msg_loops"] == 2 and d["n_bodies"] == 3
    m2 = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
    assert m2.compile_where(r"\E r1, r2 \in replicas : rep_view_number[r1] # rep_view_number[r2]").describe()["n_bodies"] == 4
    # a dynamic index is a select chain over the R candidates: longer at R = 3 than at R = 2
    dyn = r"\E m \in DOMAIN messages : rep_view_number[m.dest] = 1"
    assert m.compile_where(dyn).describe()["n_ops"] > m2.compile_where(dyn).describe()["n_ops"]


def test_symmetry_refuses_model_value_literals(vt):
    text = r"\E r \in replicas : rep_log[r][1].operation = v1"
    sym = vt.Model.from_constants(R=3, C_=1, n=2, L=2, symmetry=True)
    with pytest.raises(vt.VsrmcError) as e:
        sym.compile_where(text)
    assert e.value.code == -1 and "SYMMETRY" in e.value.message and re.match(r"^1:\d+: ", e.value.message)
    vt.Model.from_constants(R=3, C_=1, n=2, L=2, symmetry=False).compile_where(text)
    sym.compile_where(r"\E v \in Values : \E r \in replicas : rep_log[r][1].operation = v")      # through a bound variable: symmetric


def test_analysis_models_are_refused(vt):
    for other in (vt.Model.second_model(R=2, n=2, L=2), vt.Model.third_model(R=2, n=2, L=2)):
        with pytest.raises(vt.VsrmcError) as e:
            other.compile_where("TRUE")
        assert e.value.code == -1 and e.value.message == "state predicates: VSR.tla only"


def test_example_file_compiles(vt, m):
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "predicates_example.txt")
    w = m.compile_where(open(path).read())
    assert w.names == ["LogDivergence", "CommittedLogDivergence", "AckedWriteSurvives", "AckedWriteOnMajority"]


def test_without_a_device_the_compute_call_fails_loudly(vt, m):
    """no CPU evaluation: where a device is visible the call answers, where none is it fails with VSRMC_E_HIP"""
    import numpy as np
    w = m.compile_where(r"\A r \in replicas : rep_status[r] = Normal")
    rec = m.init_state()
    off = np.array([0, len(rec)], dtype=np.uint64)
    if vt.load().vsrmc_device_count() > 0:
        assert [int(x) for x in m.where_flags(w, rec, off)] == [1]
        return
    with pytest.raises(vt.VsrmcError) as e:
        m.where_flags(w, rec, off)
    assert e.value.code == -3
