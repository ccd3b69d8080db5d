"""The invariant evaluators of the two analysis models on VIOLATING states, host side (no GPU).

Every state the suite's walks visit satisfies the invariants of VR_STATE_TRANSFER / VR_APP_STATE, so the two CPU readings — the C++
oracle's check_invariants (oracle/vrst_oracle.cpp, oracle/vras_oracle.cpp) and the Python restatements (oracle/pyoracle2.py,
oracle/pyoracle3.py) — were only ever compared on "all clear".  Here they meet on the mutants of tests/invariant_mutants.py and on
every child of the C++ oracle's successors of a mutant (taken with mask 0): each invariant alone gives the same answer from both,
the C++ OracleError and the Python IndexError coincide, and AcknowledgedWriteNotLost (bit 1, absent from the restatements' masks)
is checked against a restatement written here.  Where the two disagreed, VR_STATE_TRANSFER.tla:806-847 / VR_APP_STATE.tla:840-894
decide.

Also here: the cfg loader gives every invariant name its bit, and the three name tables list the same names in the same order."""
import collections
import os
import re

import numpy as np
import pytest

import invariant_mutants as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(model, space) for model in (2, 3) for space in im.SPACES]


def _ack_not_lost(po, M, s):
    """AcknowledgedWriteNotLost (VRST.tla:830-835, VRAS.tla:877-882): every acknowledged value is in some replica's log"""
    for v, acked in s["aux_client_acked"].items():
        if acked is True and not any(po.get(e, "operation") == v for log in s["rep_log"] for e in log):
            return False
    return True


def _py_verdicts(po, M, s, model):
    out = {}
    for b in im.BITS[model]:
        try:
            out[b] = 0 if (_ack_not_lost(po, M, s) if b == 1 else getattr(po, im.NAMES[b])(M, s)) else b
        except IndexError:
            out[b] = im.RAISES
    return out


@pytest.mark.parametrize("model,space", CASES)
def test_mutants_are_well_formed_and_distinct(model, space):
    orc, po = im.MODELS[model]
    R, values, L, _depth = im.SPACES[space]
    M, P = po.Model(R, values, L), im.oracle_params(model, space, 0)
    muts = im.mutants(model, space)
    base = set(im.base_records(model, space))
    assert len(set(tuple(int(x) for x in m.words) for m in muts)) == len(muts) and not any(tuple(int(x) for x in m.words) in base for m in muts)
    for m in muts:                                                    # both codecs take the record and give it back
        w = [int(x) for x in m.words]
        assert po.pack(M, po.unpack(M, w)) == w
        assert po.normalise(M, [int(x) for x in orc.normalise(P, m.words)]) == w          # (the two codecs order the bag differently)
    want = set("ABDEFN") | ({"C"} if model == 3 else set())
    if len(values) + 1 > 3:
        want.discard("D")                                             # commit > Len(log) = n does not fit the commit field at n = 3
    assert set(m.cls for m in muts) == want


def test_generator_is_deterministic():
    again = im.mutants.__wrapped__(3, "r3v3")
    first = im.mutants(3, "r3v3")
    assert [(m.cls, m.tag, m.expect) for m in again] == [(m.cls, m.tag, m.expect) for m in first]
    assert all(np.array_equal(a.words, b.words) for a, b in zip(again, first))


@pytest.mark.parametrize("model,space", CASES)
def test_the_two_cpu_readings_agree_on_violating_states(model, space):
    orc, po = im.MODELS[model]
    R, values, L, _depth = im.SPACES[space]
    M = po.Model(R, values, L)
    fams, refused = im.families(model, space)
    n = collections.Counter()
    for f in fams:
        s = po.unpack(M, [int(x) for x in f.mutant.words])
        assert f.verdicts == _py_verdicts(po, M, s, model), (f.mutant.cls, f.mutant.tag)
        for b, want in f.mutant.expect.items():                       # what the construction promises, near misses included
            assert f.verdicts[b] == want, (f.mutant.cls, f.mutant.tag, b)
        for c in f.children:
            t = po.unpack(M, [int(x) for x in c["words"]])
            assert c["verdicts"] == _py_verdicts(po, M, t, model), (f.mutant.cls, f.mutant.tag, orc.ACTIONS[c["action"]])
            for b, v in c["verdicts"].items():
                n[(b, "raises" if v == im.RAISES else "set" if v else "clear")] += 1
    print("model %d %s: %d parents (%d refused), verdicts of the children %s" % (model, space, len(fams), refused, sorted(n.items())))
    assert refused * 100 <= len(fams) + refused
    for b in im.BITS[model]:
        assert n[(b, "set")] > 0 and n[(b, "clear")] > 0
    assert n[(4, "raises")] > 0 and (model == 2 or n[(16, "raises")] > 0)


@pytest.mark.parametrize("model", [2, 3])
def test_floors_on_the_oracles_side(model):
    im.check_floors(model)


# ---- the cfg loader and the name tables ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vt():
    import __graft_entry__
    __graft_entry__.build()
    import vsr_tlaplus_amd as vt
    return vt


def _cfg(tmp_path, invariants):
    from test_model3_host_cpu import CFG
    text = CFG % dict(R=3, vals="a, b", L=2, npl=0, spec="Spec", extra="")
    p = tmp_path / ("inv_%s.cfg" % "_".join(invariants))
    p.write_text(text[: text.index("INVARIANT\n")] + "INVARIANT\n" + "".join(i + "\n" for i in invariants))
    return str(p)


def test_every_invariant_name_loads_to_its_bit(vt, tmp_path):
    """a cfg naming one invariant: exactly its bit.  Without a .tla the constants select the analysis models and NoAppStateDivergence
    the third one, so the third model's bits 1-8 are read from a cfg that names NoAppStateDivergence too."""
    from vsr_tlaplus_amd import sharded_cli
    names = sharded_cli.INVARIANTS
    assert names == [im.NAMES[1 << k] for k in range(5)]
    for k, name in enumerate(names[:4]):
        lay = vt.Model.load(_cfg(tmp_path, [name])).layout
        assert (lay.invariant_mask, lay.words_per_replica) == (1 << k, 1), name
        lay = vt.Model.load(_cfg(tmp_path, [name, names[4]])).layout
        assert (lay.invariant_mask, lay.words_per_replica) == ((1 << k) | 16, 2), name
    lay = vt.Model.load(_cfg(tmp_path, [names[4]])).layout
    assert (lay.invariant_mask, lay.words_per_replica) == (16, 2)
    with pytest.raises(vt.VsrmcError):
        vt.Model.load(_cfg(tmp_path, ["NoLogDivergance"]))
    ref = "/root/reference/vsr-revisited/paper/analysis"
    if os.path.exists(ref):                                           # the shipped modules name the model: each bit alone, 16 refused for the second
        for k, name in enumerate(names):
            lay = vt.Model.load(_cfg(tmp_path, [name]), ref + "/04-application-state/VR_APP_STATE.tla").layout
            assert (lay.invariant_mask, lay.words_per_replica) == (1 << k, 2), name
            if k < 4:
                lay = vt.Model.load(_cfg(tmp_path, [name]), ref + "/03-state-transfer/VR_STATE_TRANSFER.tla").layout
                assert (lay.invariant_mask, lay.words_per_replica) == (1 << k, 1), name
        with pytest.raises(vt.VsrmcError):
            vt.Model.load(_cfg(tmp_path, [names[4]]), ref + "/03-state-transfer/VR_STATE_TRANSFER.tla")
    # the constructors' masks are the layout's
    for mask in (1, 2, 4, 8, 14, 15):
        assert vt.Model.second_model(invariant_mask=mask).layout.invariant_mask == mask
    for mask in (1, 2, 4, 8, 16, 30, 31):
        assert vt.Model.third_model(invariant_mask=mask).layout.invariant_mask == mask


def test_the_name_tables_agree():
    """vsrmc_cli.cpp INVARIANT_NAMES, sharded_cli.INVARIANTS and the loader's chain (host_model.hpp) in one bit order"""
    from vsr_tlaplus_amd import sharded_cli
    csrc = os.path.join(ROOT, "vsr_tlaplus_amd", "csrc")
    with open(os.path.join(csrc, "vsrmc_cli.cpp")) as f:
        cli = re.search(r"INVARIANT_NAMES\[5\]\s*=\s*\{(.*?)\};", f.read(), re.S)
    assert re.findall(r'"(\w+)"', cli.group(1)) == sharded_cli.INVARIANTS
    with open(os.path.join(csrc, "host_model.hpp")) as f:
        text = f.read()
    chain = re.findall(r'iv == "(\w+)"(?: && module == 2)?\) mask2 \|= (\d+);', text[text.index("int mask2 = 0;"):])
    assert [(n, int(b)) for n, b in chain if int(b)] == [(n, 1 << k) for k, n in enumerate(sharded_cli.INVARIANTS)]
