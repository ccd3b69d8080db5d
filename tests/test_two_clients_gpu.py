"""The action bodies at TWO CLIENTS, state by state, GPU legs (`-m gpu`).

BASELINE configs[3] — 3 replicas, 2 clients, {v1,v2,v3}, limit 3, policy assume_commit_number — was compared through level totals alone.  The states come from
the three two-client harvests of tests/deep_harvest.py (SPACES_C2; pinned, with their floors, by tests/test_two_clients_cpu.py): (3,2,3,1) and (3,2,3,2) are
SPEC 323, k_expand's instantiation of that configuration, (3,2,2,1) a generic one.  Everything is integer and must be equal; no state is left out.

  leg A  k_successors, fingerprints, terminal flags: the body of test_deep_actions_gpu._three_ways over EVERY state of the three harvests (63 648 states; the
         Python restatement on the sample of deep_harvest.c2_py_sample).  The strict model on (3,2,2,1): every ReceivePrepareMsg instance carries
         ERR_EVAL_421, every other row is the policy model's.
  leg B  k_expand and friends on the harvest seeded as level 1 (tests/deep_seeded_worker.py, mode c2): a fused step (at SPEC 323 the ordinary level's
         k_expand<true,323,EXPAND_PLAIN>), an exact_ties step (k_expand<false,0> + k_materialize<0>), the probe (k_expand<true,323> / <true,0> in MODE_PROBE: k_probe_scan /
         k_probe_apply have no instantiation with ClientCount = 2 and stay unpinned there), the terminal scan, select, two passes beyond
         the record buffers (k_expand<true,323> in its insert and regenerate roles), a stored step and a probe under invariant mask 3; the two stored steps
         once more under VSRMC_CCAP=256.  Whole spaces level by level: (2,2,2,1) and (3,2,1,1), fused and exact_ties,
         and (3,2,1,1) through the automatic scheme with record buffers too small for its widest level.

Floors, asserted on what was compared: leg A >= 500 instances of each of the nine counted actions over the three spaces and >= 800 ReceivePrepareMsg
instances per client on (3,2,3,1) that flip the executed bit of a row they did not write; leg B act_generated on (3,2,3,1) >= 1000 (SendSV >= 150)."""
import collections

import numpy as np
import pytest

import deep_harvest as dh
from test_deep_actions_gpu import _act, _seeded, _three_ways
from test_deep_search import _oracle_levels
from test_gpu_parity import _compare_levels

pytestmark = pytest.mark.gpu

SPACES = sorted(dh.SPACES_C2)
IDS = ["%d-%d-%d-%d" % k for k in SPACES]
C2_MODE = ["c2", "assume_commit_number"]


@pytest.fixture(scope="module")
def vt():
    import vsr_tlaplus_amd as vt
    assert vt.load().vsrmc_device_count() >= 1, "no HIP device visible"
    return vt


@pytest.fixture(scope="module")
def orc():
    from oracle import orc
    return orc


# ---------------------------------------------------------------------------------------------------------------------
# leg A
# ---------------------------------------------------------------------------------------------------------------------
def _leg_a(vt, orc, key):
    return _three_ways(vt, orc, key, py_sample=dh.c2_py_sample(orc, key)[0])


@pytest.mark.parametrize("key", SPACES, ids=IDS)
def test_k_successors_three_ways_on_the_two_client_harvests(vt, orc, key):
    inst = _leg_a(vt, orc, key)
    e = dh.space(orc, key).enabled()
    for a in range(1, 16):
        assert inst[a] == e[a], (vt.ACTION_NAMES[a], inst[a], e[a])          # every instance of the harvest was compared


def test_k_successors_instances_reach_the_two_client_floors(vt, orc):
    total = collections.Counter()
    for key in SPACES:
        total.update(_leg_a(vt, orc, key))
    print("leg A, instances compared over the three spaces:", {vt.ACTION_NAMES[a]: total[a] for a in dh.COUNTED_C2})
    for a in dh.COUNTED_C2:
        assert total[a] >= dh.FLOOR_C2, (vt.ACTION_NAMES[a], total[a])
    flips = dh.c2_facts(orc, (3, 2, 3, 1))["flips"]                  # (every state was compared: these are instances leg A compared)
    print("leg A, (3,2,3,1): ReceivePrepareMsg flips a row it did not write:", flips)
    assert min(flips.values()) >= dh.FLOOR_C2_FLIPS


def test_the_strict_model_errs_on_every_receive_prepare_and_nowhere_else(vt, orc):
    """(3,2,2,1), the same states: at ClientCount = 2 the loop of VSR.tla:414-421 always meets the other client, whose row reads `m.commit`"""
    key = (3, 2, 2, 1)
    h = dh.space(orc, key)
    policy, strict = dh.product_model(vt, key), vt.Model.from_constants(R=3, C_=2, n=2, L=1)
    n_err = n_rows = 0
    for lo in range(0, len(h), 2048):
        hi = min(len(h), lo + 2048)
        words, off = h.batch(lo, hi)
        cap = sum(len(h.actions(i)) for i in range(lo, hi)) + 64
        a, b = policy.get_next_states(words, off, cap_succ=cap), strict.get_next_states(words, off, cap_succ=cap)
        assert len(a) == len(b) == cap - 64
        for x, y in zip(a, b):
            assert (x["parent"], x["ordinal"], x["action"], x["err"]) == (y["parent"], y["ordinal"], y["action"], 0), (lo + x["parent"], x["ordinal"])
            if x["action"] == dh.A_ReceivePrepareMsg:
                assert y["err"] == 1, (lo + x["parent"], x["ordinal"], y["err"])                      # ERR_EVAL_421
                n_err += 1
            else:
                assert y["err"] == 0 and (x["fp"], x["auxkey"], x["inv"]) == (y["fp"], y["auxkey"], y["inv"]) and np.array_equal(x["words"], y["words"])
            n_rows += 1
    policy.close()
    strict.close()
    print("strict model on (3,2,2,1): %d rows, %d of them ReceivePrepareMsg with ERR_EVAL_421" % (n_rows, n_err))
    assert n_err == h.enabled()[dh.A_ReceivePrepareMsg] >= 2000


# ---------------------------------------------------------------------------------------------------------------------
# leg B: k_expand and friends on the seeded level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(3, 2, 3, 1), (3, 2, 2, 1)], ids=["3-2-3-1", "3-2-2-1"])
def test_k_expand_on_the_seeded_two_client_level(orc, key, tmp_path_factory):
    res = _seeded(orc, key, tmp_path_factory.mktemp("c2_seeded"), mode=C2_MODE, tag="c2")
    h = dh.space(orc, key)
    assert res["seeds"] == len(h) >= 4096 and res["left_out"] == 0 and res["parts"] == [len(h)]
    labels = [r["label"] for r in res["runs"]]
    assert labels == ["exact_ties=0 part 0", "exact_ties=1", "exact_ties=0 mask 3"]
    assert res["runs"][2]["violators"] > 0 and res["probe_violators"] > 0
    assert all(r["traces"] >= 48 and r["n_new"] == res["deepen"]["n_new"][0] for r in res["runs"])
    d = res["deepen"]
    assert max(d["level2_words"], d["level3_words"]) > d["frontier_words"] and d["n_new"][1] > d["n_new"][0] > len(h)
    e = h.enabled()
    assert res["select"] == {orc.ACTIONS[a]: sum(1 for i in range(len(h)) if a in h.actions(i)) for a in dh.COUNTED_C2}
    for exact in (0, 1):
        act = _act(res, exact)
        assert act == [e[a] for a in range(16)]                      # (checked in the child against the level's own figures; here against the harvest)
        if key == (3, 2, 3, 1):
            print("leg B, act_generated, exact_ties=%d:" % exact, {orc.ACTIONS[a]: act[a] for a in sorted(dh.FLOOR_C2_EXPAND)})
            for a, floor in dh.FLOOR_C2_EXPAND.items():
                assert act[a] >= floor, (exact, orc.ACTIONS[a], act[a])


def test_tiles_are_taken_again_in_pieces_at_two_clients(orc, tmp_path_factory):
    """VSRMC_CCAP=256 shortens k_expand's work list to 4 instances per record (the harvest of (3,2,3,1) has 4.07 per state on average): tiles overflow it and
    must be taken again in pieces; the buffers are those of test_a_tile_that_overflows_the_work_list_is_taken_again_in_pieces.

    This test found that SPEC 323 could not do that: only the EXPAND_PLAIN / EXPAND_PROBE instantiations write an overflowed tile down for the host to launch
    again in halves (k_expand: REDO_OK), 323 had k_expand<true,323> alone, and the step ended in `device error 21` (ERR_FRONTIER_FULL, raised for the tile -
    loudly, nothing committed; on a run of BASELINE configs[3] one tile with more than 24 enabled instances per record would have ended the search the same
    way).  kernels_for() now gives 323 k_expand<true,323,EXPAND_PLAIN> for its ordinary unsharded level, as the other BASELINE configurations have.
    That tiles DID overflow is asserted, not assumed: the worker reports how many lists of overflowed tiles the fused step launched again (the hooks
    library's vsrmc_test_checker_extra_launches) - at least one under VSRMC_CCAP=256, none with the full work list."""
    key = (3, 2, 3, 1)
    res = _seeded(orc, key, tmp_path_factory.mktemp("c2_ccap"), mode=["assume_commit_number", "generous"], env=dict(VSRMC_CCAP="256"), tag="ccap")
    e = dh.space(orc, key).enabled()
    assert [r["label"] for r in res["runs"]] == ["exact_ties=0 part 0", "exact_ties=1"] and res["left_out"] == 0
    print("lists of overflowed tiles launched again:", [r["redo_launches"] for r in res["runs"]])
    assert res["runs"][0]["redo_launches"] >= 1                      # tiles DID overflow the short list and were taken again (the hooks library's counter)
    plain = _seeded(orc, key, tmp_path_factory.mktemp("c2_seeded"), mode=C2_MODE, tag="c2")
    assert plain["runs"][0]["redo_launches"] == 0                    # ... and with the full work list none does
    for exact in (0, 1):
        assert _act(res, exact) == [e[a] for a in range(16)]


@pytest.mark.parametrize("exact", [False, True], ids=["fused", "exact_ties"])
@pytest.mark.parametrize("params, want", [((2, 2, 2, 1), (973, 18)), ((3, 2, 1, 1), (86516, 24))], ids=["2-2-2-1", "3-2-1-1"])
def test_whole_two_client_spaces_level_by_level(vt, orc, params, want, exact):
    assert _compare_levels(vt, orc, params, 100, exact_ties=exact, assume_commit_number=True) == want


def test_whole_two_client_space_beyond_the_record_buffers(vt, orc):
    """(3,2,1,1): 86 516 states in 24 levels, the widest of 12 331 states.  Record buffers of 8 192 states / 131 072 words do not hold it: the automatic scheme
    stores the levels that fit and passes the others through the seen-set alone; every level has the oracle's figures, to exhaustion"""
    P = orc.Params(3, 2, 1, 1, assume_commit_number=True)
    want, ob = _oracle_levels(orc, P, 100)
    ob.close()
    assert max(w["n_new"] for w in want) == 12331 and 1 + sum(w["n_new"] for w in want) == 86516
    m = vt.Model.from_constants(R=3, C_=2, n=1, L=1, assume_commit_number=True)
    mc = vt.ModelChecker(m, table_log2=20, frontier_words=1 << 17, frontier_states=1 << 13, pending_entries=1 << 16)
    kinds = []
    for w in want:
        kind, a, b = mc.advance()
        kinds.append(kind)
        if w["n_new"] == 0:
            assert a["n_new"] == 0
            break
        assert (a["level"], a["n_new"], a["generated"], a["deadlocks"], a["viol_mask"]) == (w["level"], w["n_new"], w["generated"], w["deadlocks"], 0), w["level"]
        got = mc.level_checksum()[:2] if kind == "level" else (a["fp_xor"], a["fp_sum"])
        assert got == (w["fp_xor"], w["fp_sum"]), (kind, w["level"])
    print("kinds of progress:", kinds, "re-based:", [r["level"] for r in mc.rebased])
    assert kinds.count("deep") >= 3 and mc.distinct == 86516
    mc.close()
    m.close()
