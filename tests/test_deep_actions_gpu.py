"""The action bodies deep in the view-change and state-transfer protocol at FIVE and FOUR replicas, GPU legs (`-m gpu`).

Level totals at R = 5 / R = 4 (tests/test_gpu_parity.py, the 14 levels of oracle_levels_config5.json) never execute ReceiveSV, SendGetState,
ReceiveGetState or ReceiveNewState and compare no record of SendSV's.  The states come from tests/deep_harvest.py (a deterministic guided walk on the
C++ oracle; pinned by tests/test_deep_actions_cpu.py), all of them reachable, all within the layout's bag capacity: no state is skipped, no successor
may carry an error, everything is integer and must be equal.

  leg A  k_successors (Model.get_next_states, one lane per parent): for EVERY harvested state the multiset of (action, fingerprint, auxkey,
         invariant mask, normalised record) equals the C++ oracle's, on a sample (60 states per counted action and space) also the Python
         restatement's; Model.fingerprints equals the oracle's, Model.terminal_flags bit 0 equals "the oracle lists no successor".
  leg B  k_expand itself (tests/deep_seeded_worker.py in a child process under libvsrmc_hooks.so): the harvested states are seeded as level 1 of a
         checker and one step / probe / deepen / terminal scan / select runs over them; every expected figure comes from the oracle alone.
         (5,1,2,1) runs the whole family of instantiations (SPEC 512), (4,1,2,1) a fused one (SPEC 412), (5,1,1,2) and (4,1,1,2) the generic ones.

Floors, asserted here: directly compared instances per action >= 1000 at R = 5 and >= 200 at R = 4 for SendSV, ReceiveSV, ReceiveHigherDVC,
ReceivePrepareOkMsg, ExecuteOp, SendGetState, ReceiveGetState, ReceiveNewState — in leg A and, as act_generated, in leg B.
"""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import deep_harvest as dh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACES = sorted(dh.SPACES)
IDS = ["%d-%d-%d-%d" % k for k in SPACES]
BATCH = 2048


@pytest.fixture(scope="module")
def vt():
    import vsr_tlaplus_amd as vt
    assert vt.load().vsrmc_device_count() >= 1, "no HIP device visible"
    return vt


@pytest.fixture(scope="module")
def orc():
    from oracle import orc
    return orc


def _norm(orc, P, words):
    return tuple(int(x) for x in orc.normalise(P, words))


_leg_a = {}


def _three_ways(vt, orc, key, py_sample=None):
    """leg A over one space of deep_harvest.SPACES or SPACES_C2 (under the policy of that space) -> instances per action (memoised: the floor test needs
    every space).  py_sample: the indices of the states on which the Python restatement is compared; None: the first 60 states that enable each expected
    action"""
    if key in _leg_a:
        return _leg_a[key]
    from oracle import pycodec, pyoracle as po
    h = dh.space(orc, key)
    P = h.P
    PM = dh.py_model(key)
    m = dh.product_model(vt, key)
    expected = dh.expected(key)
    py_set = None if py_sample is None else set(py_sample)
    n_py = 0
    inst = collections.Counter()
    py_checked = collections.Counter()
    n_states = 0
    for lo in range(0, len(h), BATCH):
        hi = min(len(h), lo + BATCH)
        words, off = h.batch(lo, hi)
        osucc = [h.successors(i) for i in range(lo, hi)]
        n_succ = sum(len(s) for s in osucc)
        gpu = collections.defaultdict(list)
        for s in m.get_next_states(words, off, cap_succ=n_succ + 64, cap_words=sum(len(x["words"]) for ss in osucc for x in ss) + 4096):
            assert s["err"] == 0, (key, lo + s["parent"], s["err"])
            gpu[s["parent"]].append((s["action"], s["fp"], s["auxkey"], s["inv"], _norm(orc, P, s["words"])))
        assert sum(len(v) for v in gpu.values()) == n_succ
        fps, aks = m.fingerprints(words, off)
        flags = m.terminal_flags(words, off)
        for k, i in enumerate(range(lo, hi)):
            theirs = sorted((x["action"], x["fp"], x["auxkey"], x["inv"], _norm(orc, P, x["words"])) for x in osucc[k])
            assert sorted(gpu.get(k, [])) == theirs, (key, i)
            assert (int(fps[k]), int(aks[k])) == orc.fingerprint(P, h.records[i]), (key, i)
            assert (int(flags[k]) & 1) == (0 if osucc[k] else 1), (key, i)
            n_states += 1
            enabled = set()
            for x in osucc[k]:
                inst[x["action"]] += 1
                enabled.add(x["action"])
            want_py = [a for a in expected if a in enabled and py_checked[a] < 60] if py_set is None else i in py_set
            if want_py:                                             # the independent Python restatement on a sample
                n_py += 1
                st = pycodec.unpack(PM, [int(x) for x in h.records[i]])
                ps = sorted((nm, tuple(pycodec.normalise(PM, pycodec.pack(PM, t)))) for nm, t in po.successors(PM, st))
                cs = sorted((vt.ACTION_NAMES[x["action"]], tuple(pycodec.normalise(PM, [int(v) for v in x["words"]]))) for x in osucc[k])
                assert ps == cs, (key, i)
                for a in enabled:
                    py_checked[a] += 1
    m.close()
    assert n_states == len(h)                                       # the share of harvested states left out of the comparison is zero
    if py_set is None:
        for a in expected:
            assert py_checked[a] >= 60, (key, vt.ACTION_NAMES[a], py_checked[a])
    else:
        assert n_py == len(py_set)                                  # ... and so is the share of the sample
    print(key, "states", n_states, "of them through the Python restatement", n_py, {vt.ACTION_NAMES[a]: inst[a] for a in sorted(inst)})
    _leg_a[key] = inst
    return inst


@pytest.mark.parametrize("key", SPACES, ids=IDS)
def test_k_successors_three_ways_on_every_harvested_state(vt, orc, key):
    inst = _three_ways(vt, orc, key)
    for a in dh.EXPECTED[key]:
        assert inst[a] >= 60, (vt.ACTION_NAMES[a], inst[a])


def test_k_successors_instances_reach_the_floors(vt, orc):
    for R in (5, 4):
        total = collections.Counter()
        for key in SPACES:
            if key[0] == R:
                total.update(_three_ways(vt, orc, key))
        for a in dh.COUNTED:
            assert total[a] >= dh.FLOOR[R], (R, vt.ACTION_NAMES[a], total[a])


# ---------------------------------------------------------------------------------------------------------------------
# leg B: k_expand on the seeded level
# ---------------------------------------------------------------------------------------------------------------------
_leg_b = {}


def _seeded(orc, key, tmp, mode=None, env=None, tag=""):
    """the harvest of one space seeded as level 1 of a checker in a child process (tests/deep_seeded_worker.py) -> what the worker reports.  mode: the
    worker's mode and policy arguments; env: more environment of the child; tag: what tells two runs of one space apart"""
    if (key, tag) in _leg_b:
        return _leg_b[(key, tag)]
    h = dh.space(orc, key)
    words, off = h.batch(0, len(h))
    seeds = os.path.join(str(tmp), "seeds_%d%d%d%d.npz" % key)
    out = os.path.join(str(tmp), "seeded_%d%d%d%d%s.json" % (key + (tag,)))
    np.savez(seeds, words=words, off=off)
    hooks = os.path.join(ROOT, "vsr_tlaplus_amd", "libvsrmc_hooks.so")
    assert os.path.exists(hooks), "build it: python vsr_tlaplus_amd/build.py"
    if mode is None:
        mode = {(5, 1, 2, 1): ["full"], (4, 1, 2, 1): ["viol"]}.get(key, [])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "deep_seeded_worker.py")] + [str(x) for x in key] + [seeds, out] + mode,
                       capture_output=True, text=True, timeout=1500, env=dict(os.environ, VSRMC_LIB=hooks, **(env or {})))
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    with open(out) as f:
        _leg_b[(key, tag)] = json.load(f)
    return _leg_b[(key, tag)]


def _act(res, exact):
    """act_generated of the single-pass runs (their parts added up) / of the exact_ties run"""
    tot = [0] * 16
    for run in res["runs"]:
        if run["label"].startswith("exact_ties=%d" % exact) and "mask" not in run["label"]:
            tot = [a + b for a, b in zip(tot, run["act_generated"])]
    return tot


@pytest.mark.parametrize("key", SPACES, ids=IDS)
def test_k_expand_on_the_seeded_level(orc, key, tmp_path_factory):
    res = _seeded(orc, key, tmp_path_factory.mktemp("deep_seeded"))
    assert res["seeds"] == len(dh.space(orc, key)) >= 4096
    assert res["left_out"] * 100 <= res["seeds"]
    labels = [r["label"] for r in res["runs"]]
    assert "exact_ties=0 part 0" in labels and "exact_ties=1" in labels
    if key in ((5, 1, 2, 1), (4, 1, 2, 1)):                          # a stored step whose image violates (invariant mask 3)
        assert [r for r in res["runs"] if r["label"] == "exact_ties=0 mask 3"][0]["violators"] > 0
    if key == (5, 1, 2, 1):
        assert res["probe_violators"] > 0 and res["deepen"]["level2_words"] > res["deepen"]["frontier_words"]
    for exact in (0, 1):
        act = _act(res, exact)
        for a in dh.EXPECTED[key]:
            assert act[a] >= 60, (exact, a, act[a])


def test_k_expand_instances_reach_the_floors(vt, orc, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("deep_seeded_floors")
    for R in (5, 4):
        for exact in (0, 1):
            total = [0] * 16
            for key in SPACES:
                if key[0] == R:
                    total = [a + b for a, b in zip(total, _act(_seeded(orc, key, tmp), exact))]
            for a in dh.COUNTED:
                # (a single-pass run leaves out at most 1 % of the seeds: the floors must hold without them)
                assert total[a] >= dh.FLOOR[R], (R, exact, vt.ACTION_NAMES[a], total[a])


# ---------------------------------------------------------------------------------------------------------------------
# hand-built records: HighestLog at f + 1 = 3 (VSR.tla:716-722), HighestCommitNumber (:729-733), state transfer with two lagging replicas
# ---------------------------------------------------------------------------------------------------------------------
def _three_way_states(vt, orc, key, states):
    """successor multisets of python states: HIP == C++ oracle == Python restatement -> (wire records, the oracle's successors as python states)"""
    from oracle import pycodec, pyoracle as po
    R, C_, n, L = key
    PM = po.Model(R, C_, tuple("v%d" % (i + 1) for i in range(n)), L)
    P = orc.Params(*key)
    m = vt.Model.from_constants(R=R, C_=C_, n=n, L=L)
    recs = [np.array(pycodec.pack(PM, s), dtype=np.uint64) for s in states]
    words = np.concatenate(recs)
    off = np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64)
    gpu = collections.defaultdict(list)
    for s in m.get_next_states(words, off):
        assert s["err"] == 0
        gpu[s["parent"]].append((s["action"], s["fp"], s["auxkey"], s["inv"], _norm(orc, P, s["words"])))
    m.close()
    out = []
    for i, (s, rec) in enumerate(zip(states, recs)):
        osucc = orc.successors(P, rec)
        theirs = sorted((x["action"], x["fp"], x["auxkey"], x["inv"], _norm(orc, P, x["words"])) for x in osucc)
        assert sorted(gpu.get(i, [])) == theirs, i
        ps = sorted((nm, tuple(pycodec.normalise(PM, pycodec.pack(PM, t)))) for nm, t in po.successors(PM, s))
        cs = sorted((vt.ACTION_NAMES[x["action"]], tuple(pycodec.normalise(PM, [int(v) for v in x["words"]]))) for x in osucc)
        assert ps == cs, i
        out.append([(vt.ACTION_NAMES[x["action"]], pycodec.unpack(PM, [int(v) for v in x["words"]])) for x in osucc])
    return recs, out


@pytest.mark.parametrize("R", [5, 4])
def test_hand_built_view_change_and_state_transfer_records(vt, orc, R, tmp_path):
    key = (R, 1, 2, 1)
    states, checks = dh.hand_built(R)
    recs, succ = _three_way_states(vt, orc, key, states)
    for k, chk in checks:
        chk(succ[k])
    # ... and through k_expand: the hand-built records among harvested ones (full tiles), one seeded step each way
    h = dh.space(orc, key)
    mine = set(orc.fingerprint(h.P, r)[0] for r in recs)
    assert len(mine) == len(recs) and not mine & set(h.fps)
    recs = recs + h.records[:1024]
    seeds = os.path.join(str(tmp_path), "hand.npz")
    out = os.path.join(str(tmp_path), "hand.json")
    np.savez(seeds, words=np.concatenate(recs), off=np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64))
    hooks = os.path.join(ROOT, "vsr_tlaplus_amd", "libvsrmc_hooks.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "deep_seeded_worker.py")] + [str(x) for x in key] + [seeds, out, "small"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, VSRMC_LIB=hooks))
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    with open(out) as f:
        res = json.load(f)
    assert res["seeds"] == len(recs) and res["left_out"] == 0
    n_sv = sum(1 for ss in succ for a, _t in ss if a == "SendSV")
    n_sgs = sum(1 for ss in succ for a, _t in ss if a == "SendGetState")
    assert n_sv >= 9 and n_sgs >= 11
    assert all(run["act_generated"][dh.A_SendSV] >= n_sv and run["act_generated"][dh.A_SendGetState] >= n_sgs for run in res["runs"])
