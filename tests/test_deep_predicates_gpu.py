"""The predicate kernels at FIVE and FOUR replicas (`-m gpu`): k_where and k_step_list / k_step_apply on records whose replica blocks have a fourth word.

test_where_gpu.py and test_step_gpu.py walk spaces of two and three replicas.  What exists only from four replicas on — the fourth block word in the pair
view (StepPair::word), the DoViewChange slots of sources 4 and 5 in Cardinality(rep_dvc_recv[r]), broadcasts that append R - 1 bag entries
(StepPair::msg), select chains over five candidates, bags above 32 messages in the two-deep message loops — runs here, on a deterministic sample of the
harvest of tests/deep_harvest.py (deep_predicates_reference.py: 1500 states and 150 parents with all their successors per space; what the sample holds is
pinned by test_deep_predicates_cpu.py) and on the hand-built records of deep_harvest.hand_built.  Every comparison is exact, against hand-written Python
functions over pycodec's unpack of the CPU oracle's records (where_reference.py, step_reference.py, deep_predicates_reference.py — never the parser).

The level scans run in a child process under libvsrmc_hooks.so (tests/deep_predicates_worker.py): the sample is seeded as level 1 of a checker.

TWO CLIENTS: the same tests run on (3,2,3,1) and (3,2,2,1) of deep_harvest.SPACES_C2 under the policy assume_commit_number, with the two-client sets of
deep_predicates_reference.py (tag C2) in the place of the R >= 4 sets: the second row of a client table, "exists c in clients", a client index that is an expression,
client_id = 2 in logs and in the entry a PrepareMsg carries, ClientCount, and the row ReceivePrepareMsg rewrites for the client whose entry it did NOT append.  Half of
the 150 parents there are states in which that happens (deep_predicates_reference.c2_parent_indices).  Every two-client predicate takes each verdict at least 20
times on what is compared (pinned on the CPU by test_two_clients_cpu.py).  On these spaces the seeded child also runs two passes beyond the record buffers
with the C2 sets attached: the inserted and regenerated levels (k_where / k_step_list on scratch slices) and the probed level (k_probe_where) against the
oracle's levels through the Python predicates."""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import deep_harvest as dh
import deep_predicates_reference as dp
import step_reference as sr
import where_reference as wr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2_SPACES = [(3, 2, 3, 1), (3, 2, 2, 1)]
SPACES = sorted(dh.SPACES) + C2_SPACES
IDS = ["%d-%d-%d-%d" % k for k in SPACES]
N_DEEP = 40                                                         # parents seeded for the passes beyond the record buffers (two-client spaces)
Sample = collections.namedtuple("Sample", "key P PM fixed recs fps states words off precs pfps pstates pwords poff succ")


@pytest.fixture(scope="module")
def vt():
    import vsr_tlaplus_amd as vt
    assert vt.load().vsrmc_device_count() >= 1, "no HIP device visible"
    return vt


@pytest.fixture(scope="module")
def orc():
    from oracle import orc
    return orc


def _norm(fixed, r):
    return tuple(int(x) for x in r[:fixed]) + tuple(sorted(int(x) for x in r[fixed:]))


def _batch(recs):
    return np.concatenate(recs), np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64)


_pm = dh.py_model
_state_sets = dp.state_sets
_samples = {}
_views = {}                                                         # (key, normalised record) -> Python view
_step_bits = {}                                                     # (key, tag, parent, child, action name) -> bits by the reference


def _view(key, norm):
    from oracle import pycodec
    k = (key, norm)
    if k not in _views:
        _views[k] = pycodec.unpack(_pm(key), list(norm))
    return _views[k]


def _bits_of_pair(key, tag, preds, pn, cn, a):
    k = (key, tag, pn, cn, a)
    if k not in _step_bits:
        _step_bits[k] = sr.bits_of(preds, _view(key, pn), _view(key, cn), a)
    return _step_bits[k]


def _sample(vt, orc, key):
    """the sample of one space: records, fingerprints and Python views of the 1500 states; of the 150 parents also the oracle's successors as
    (action name, normalised child record); computed once per process, never changed"""
    if key not in _samples:
        h = dh.space(orc, key)
        fixed = h.P.fixed_words()
        si = dp.state_indices(len(h))
        if key[1] == 2:
            flips = dh.c2_facts(orc, key)["flip_states"]
            pi = dp.c2_parent_indices(len(h), flips[1] + flips[2])
            assert len(set(si)) == dp.N_STATES and len(set(pi)) == dp.N_PARENTS
        else:
            pi = dp.parent_indices(len(h))
            assert len(set(si)) == dp.N_STATES and si[::10] == pi
        recs = [h.records[i] for i in si]
        states = [_view(key, _norm(fixed, r)) for r in recs]
        precs = [h.records[i] for i in pi]
        succ = [[(vt.ACTION_NAMES[s["action"]], _norm(fixed, s["words"])) for s in h.successors(i)] for i in pi]
        words, off = _batch(recs)
        pwords, poff = _batch(precs)
        _samples[key] = Sample(key, h.P, _pm(key), fixed, recs, [h.fps[i] for i in si], states, words, off, precs, [h.fps[i] for i in pi],
                               [_view(key, _norm(fixed, r)) for r in precs], pwords, poff, succ)
    return _samples[key]


def _model(vt, key):
    return dh.product_model(vt, key)


def _both_verdicts(hits, n, label):
    """every two-client predicate: true on at least 20 and false on at least 20 of the n items compared"""
    for name, k in hits.items():
        assert dp.BOTH_VERDICTS <= k <= n - dp.BOTH_VERDICTS, (label, name, k, n)


# ---------------------------------------------------------------------------------------------------------------------
# 1. states
# ---------------------------------------------------------------------------------------------------------------------
def _flags_equal_the_reference(m, key, sets, words, off, states, label):
    hits = {}
    for tag, preds in sets:
        w = m.compile_where(wr.text_of(preds))
        assert w.names == [p[0] for p in preds]
        flags = m.where_flags(w, words, off)
        assert len(flags) == len(states)
        n = [0] * len(preds)
        for i, s in enumerate(states):
            want = wr.bits_of(preds, s)
            assert int(flags[i]) == want, (label, tag, i, bin(int(flags[i])), bin(want))
            for k in range(len(preds)):
                n[k] += (want >> k) & 1
        hits[tag] = dict(zip((p[0] for p in preds), n))
    return hits


@pytest.mark.parametrize("key", SPACES, ids=IDS)
def test_where_flags_on_the_sampled_states(vt, orc, key):
    S = _sample(vt, orc, key)
    m = _model(vt, key)
    hits = _flags_equal_the_reference(m, key, _state_sets(key), S.words, S.off, S.states, key)
    m.close()
    print("where_flags %s, hits of %d states: %s" % (key, len(S.states), hits))
    if key[1] == 2:
        _both_verdicts(hits["C2"], len(S.states), key)
        return
    for name in ("DvcHeld", "DvcQuorum", "DvcAllButOne", "SvcFour", "TailView"):      # (both verdicts per replica count: test_deep_predicates_cpu.py)
        assert 0 < hits["R4"][name] < len(S.states), name


@pytest.mark.parametrize("key", SPACES, ids=IDS)
def test_random_expressions_on_a_sub_stride(vt, orc, key):
    S = _sample(vt, orc, key)
    m = _model(vt, key)
    assert dp.N_STATES % dp.N_RANDOM == 0
    stride = dp.N_STATES // dp.N_RANDOM
    assert [dp.state_indices(len(dh.space(orc, key)))[i] for i in range(0, dp.N_STATES, stride)] == dp.random_indices(len(dh.space(orc, key)))
    recs, states = S.recs[::stride], S.states[::stride]
    words, off = _batch(recs)
    preds = wr.random_predicates(20261017, key[0], 100)
    n_true = collections.Counter()
    for j in range(0, 100, 8):
        chunk = preds[j: j + 8]
        w = m.compile_where("\n".join("P%d == %s" % (k, t) for k, (t, _) in enumerate(chunk)))
        flags = m.where_flags(w, words, off)
        for i, s in enumerate(states):
            got = int(flags[i])
            for k, (text, f) in enumerate(chunk):
                want = f(s)
                n_true[j + k] += want
                assert bool((got >> k) & 1) == want, "space %s, sampled state %d: %s is %s in the reference" % (key, i * stride, text, want)
    m.close()
    used = sum(1 for k in range(100) if 0 < n_true[k] < len(states))
    print("random expressions: %d of 100 have both verdicts on %d states of %s" % (used, len(states), key))
    assert used >= 30                                                # (the floor of test_where_gpu.py; by the reference alone 37, 61, 38 and 54 of them do here, 68 and 64 at the two two-client spaces)


# ---------------------------------------------------------------------------------------------------------------------
# 2. pairs
# ---------------------------------------------------------------------------------------------------------------------
def _step_flags_equal_the_reference(vt, m, key, fixed, words, off, parents, succ, label):
    """the shape of test_step_gpu._pair_by_pair: rows equal get_next_states in (parent, ordinal, action, err); per parent the multiset (normalised child,
    action name, bits) equals the one built from the oracle's successors and the reference -> hits per set and predicate"""
    nx = m.get_next_states(words, off, cap_succ=max(64, 64 * len(parents)))
    assert len(nx) == sum(len(x) for x in succ), label
    hits = {}
    for tag, preds in dp.step_sets(key):
        w = m.compile_step(sr.text_of(preds))
        assert w.names == [p[0] for p in preds] and w.step
        rows = m.step_flags(w, words, off)
        assert rows.shape == (len(nx), 5), (label, tag)
        got = [collections.Counter() for _ in parents]
        for row, s in zip(rows, nx):
            assert (int(row[0]), int(row[1]), int(row[2]), int(row[4])) == (s["parent"], s["ordinal"], s["action"], s["err"]) and s["err"] == 0, (label, tag)
            got[s["parent"]][(_norm(fixed, s["words"]), vt.ACTION_NAMES[s["action"]], int(row[3]))] += 1
        n = [0] * len(preds)
        for i, pn in enumerate(parents):
            want = collections.Counter()
            for a, cn in succ[i]:
                bits = _bits_of_pair(key, tag, preds, pn, cn, a)
                want[(cn, a, bits)] += 1
                for k in range(len(preds)):
                    n[k] += (bits >> k) & 1
            assert got[i] == want, (label, tag, i)
        hits[tag] = dict(zip((p[0] for p in preds), n))
    return hits


@pytest.mark.parametrize("key", SPACES, ids=IDS)
def test_step_flags_on_the_sampled_parents(vt, orc, key):
    S = _sample(vt, orc, key)
    m = _model(vt, key)
    parents = [_norm(S.fixed, r) for r in S.precs]
    hits = _step_flags_equal_the_reference(vt, m, key, S.fixed, S.pwords, S.poff, parents, S.succ, key)
    m.close()
    n_pairs = sum(len(x) for x in S.succ)
    by_action = collections.Counter(a for row in S.succ for a, _cn in row)
    word3 = sum(1 for pn, row in zip(parents, S.succ) for _a, cn in row if dp.fourth_word_changes(_view(key, pn), _view(key, cn)))
    growth = collections.Counter(len(cn) - len(pn) for pn, row in zip(parents, S.succ) for _a, cn in row)
    print("step_flags %s: %d pairs of %d parents, by action %s" % (key, n_pairs, len(parents), dict(by_action)))
    print("step_flags %s: pairs whose fourth block word changes %d, bag entries appended %s" % (key, word3, sorted(growth.items())))
    print("step_flags %s, hits: %s" % (key, hits))
    if key[1] == 2:
        _both_verdicts(hits["C2"], n_pairs, key)
        assert by_action["ReceivePrepareMsg"] >= dp.N_C2_FLIP_PARENTS
        return
    fl = dp.floors(key)
    assert word3 >= fl["word3"] and growth[key[0] - 1] >= fl["bcast"]
    assert hits["R4"]["DvcGrew"] > 0 and hits["R4"]["NewKeyForLast"] > 0 and hits["R4"]["DvcQuorumReached"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. hand-built records: HighestLog ties at a quorum of three, state transfer with lagging replicas (deep_harvest.hand_built)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [5, 4])
def test_hand_built_records_through_both(vt, orc, R):
    from oracle import pycodec
    key = (R, 1, 2, 1)
    PM = _pm(key)
    P = orc.Params(*key)
    fixed = P.fixed_words()
    states, _checks = dh.hand_built(R)
    recs = [np.array(pycodec.pack(PM, s), dtype=np.uint64) for s in states]
    words, off = _batch(recs)
    m = _model(vt, key)
    views = [_view(key, _norm(fixed, r)) for r in recs]
    hits = _flags_equal_the_reference(m, key, _state_sets(key), words, off, views, ("hand-built", R))
    assert hits["R4"]["DvcQuorum"] >= 9 and hits["R4"]["DvcHeld"] > hits["R4"]["DvcQuorum"]      # (the record one short of the quorum)
    succ = [[(vt.ACTION_NAMES[s["action"]], _norm(fixed, s["words"])) for s in orc.successors(P, r)] for r in recs]
    phits = _step_flags_equal_the_reference(vt, m, key, fixed, words, off, [_norm(fixed, r) for r in recs], succ, ("hand-built", R))
    m.close()
    print("hand-built R = %d: %d states, %d pairs; state hits %s; step hits %s" % (R, len(recs), sum(len(x) for x in succ), hits["R4"], phits["R4"]))
    assert phits["R4"]["NewKeyForLast"] >= 9 and phits["R4"]["TailUnchanged"] >= 9                # every SendSV broadcasts a StartView, ReplicaCount among the destinations


# ---------------------------------------------------------------------------------------------------------------------
# 4. the scans of a seeded level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SPACES, ids=IDS)
def test_scans_on_the_seeded_level(vt, orc, key, tmp_path):
    S = _sample(vt, orc, key)
    seeds, out, frontier = (os.path.join(str(tmp_path), x) for x in ("seeds.npz", "out.json", "frontier.npz"))
    dwords, doff = _batch(S.precs[:N_DEEP])
    np.savez(seeds, words=S.words, off=S.off, pwords=S.pwords, poff=S.poff, dwords=dwords, doff=doff)
    hooks = os.path.join(ROOT, "vsr_tlaplus_amd", "libvsrmc_hooks.so")
    assert os.path.exists(hooks), "build it: python vsr_tlaplus_amd/build.py"
    more = ["assume_commit_number", "deep"] if key[1] == 2 else []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "deep_predicates_worker.py")] + [str(x) for x in key] + [seeds, out, frontier] + more,
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, VSRMC_LIB=hooks))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    with open(out) as f:
        res = json.load(f)
    # ---- states: where_scan / where_states over the 1500 seeded states
    for tag, preds in _state_sets(key):
        t = res["where"][tag]
        want = sorted((int(fp), wr.bits_of(preds, s)) for fp, s in zip(S.fps, S.states))
        assert (t["level"], t["n_states"]) == (1, len(S.states)), tag
        assert [tuple(x) for x in t["states"]] == [x for x in want if x[1]], tag
        for k in range(len(preds)):
            mine = [fp for fp, b in want if (b >> k) & 1]
            assert t["count"][k] == len(mine), (tag, preds[k][0])
            if mine:
                assert t["min_fp"][k] == mine[0] and t["min_index"][k] == t["found_at"][k] is not None, (tag, preds[k][0])
            else:
                assert t["min_fp"][k] is None and t["min_index"][k] is None, (tag, preds[k][0])
        print("where_scan %s %s: %s" % (key, tag, dict(zip((p[0] for p in preds), t["count"]))))
    # ---- pairs: step_scan / step_pairs over the 150 seeded parents.  Which pair is which ordinal: the level's own records (the bag order of a stored
    # record names the ordinals) through get_next_states, whose rows test_step_flags_on_the_sampled_parents holds against the oracle
    z = np.load(frontier)
    fwords, foff = z["words"], z["off"]
    frecs = [fwords[int(foff[i]): int(foff[i + 1])] for i in range(len(foff) - 1)]
    ffps = [int(orc.fingerprint(S.P, rec)[0]) for rec in frecs]
    assert sorted(ffps) == sorted(int(x) for x in S.pfps)
    fnorm = [_norm(S.fixed, rec) for rec in frecs]
    n_succ = sum(len(x) for x in S.succ)
    m = _model(vt, key)
    nx = m.get_next_states(fwords, foff, cap_succ=max(64, 64 * len(frecs)))
    m.close()
    assert len(nx) == n_succ
    for tag, preds in dp.step_sets(key):
        t = res["step"][tag]
        assert (t["level"], t["n_states"], t["n_err"]) == (1, len(frecs), 0), tag
        assert t["n_pairs"] + t["n_err"] == n_succ, tag              # the oracle's successor count
        want = []
        action_of = {}
        for s in nx:
            a = vt.ACTION_NAMES[s["action"]]
            bits = _bits_of_pair(key, tag, preds, fnorm[s["parent"]], _norm(S.fixed, s["words"]), a)
            action_of[(ffps[s["parent"]], int(s["ordinal"]))] = int(s["action"])
            if bits:
                want.append((ffps[s["parent"]], int(s["ordinal"]), int(bits)))
        want.sort()
        assert [tuple(x) for x in t["pairs"]] == want, tag
        for k in range(len(preds)):
            hit = [(fp, o) for fp, o, b in want if (b >> k) & 1]
            assert t["count"][k] == len(hit), (tag, preds[k][0])
            if hit:
                assert (t["min_fp"][k], t["min_ordinal"][k], t["min_action"][k]) == hit[0] + (action_of[hit[0]],), (tag, preds[k][0])
                assert t["min_index"][k] == t["found_at"][k] is not None
            else:
                assert t["min_fp"][k] is None and t["min_ordinal"][k] is None and t["min_action"][k] is None, (tag, preds[k][0])
        print("step_scan %s %s: %d pairs, %s" % (key, tag, t["n_pairs"], dict(zip((p[0] for p in preds), t["count"]))))
    if key[1] == 2:
        _check_the_passes_beyond_the_buffers(orc, S, res["deep"])


def _check_the_passes_beyond_the_buffers(orc, S, deep):
    """the first N_DEEP parents seeded as level 1, the C2 sets attached, two deepen() passes: levels 2 and 3 are scanned as regenerated / inserted levels (state
    and step program), level 4 as the probed level (k_probe_where, the state program).  The levels are the oracle's: level k + 1 = the successors of level k
    that no earlier level holds.  No C2 predicate reads an aux variable or names a value: every copy of a state has the same bits."""
    key = S.key
    state_preds, step_preds = dp.state_sets(key)[-1][1], dp.step_sets(key)[-1][1]
    levels = {1: {int(orc.fingerprint(S.P, r)[0]): r for r in S.precs[:N_DEEP]}}
    succ_of = {}
    known = set(levels[1])
    for lvl in (2, 3, 4):
        nxt = {}
        for fp, rec in levels[lvl - 1].items():
            succ_of[fp] = orc.successors(S.P, rec)
            for s in succ_of[fp]:
                if s["fp"] not in known and s["fp"] not in nxt:
                    nxt[s["fp"]] = s["words"]
        known.update(nxt)
        levels[lvl] = nxt
    assert [(p["inserted"]["level"], p["inserted"]["n_new"], p["inserted"]["viol_mask"]) for p in deep["passes"]] == [(2, len(levels[2]), 0), (3, len(levels[3]), 0)]
    assert deep["passes"][1]["inserted"]["generated"] == sum(len(succ_of[fp]) for fp in levels[2])
    seen = {}
    for r in deep["results"]:
        probed = r["kind"] == "probed"
        assert (r["level"], probed) not in seen and r["exact"] is True
        seen[(r["level"], probed)] = r
        lv = levels[r["level"]]
        want = sorted((fp, wr.bits_of(state_preds, _view(key, _norm(S.fixed, rec)))) for fp, rec in lv.items())
        hit = [x for x in want if x[1]]
        assert [tuple(x) for x in r["states"]] == hit and r["n_hit_states"] == len(hit), (r["level"], r["kind"])
        for k in range(len(state_preds)):
            mine = [fp for fp, b in want if (b >> k) & 1]
            assert (r["state"]["count"][k], r["state"]["min_fp"][k]) == (len(mine), mine[0] if mine else None), (r["level"], r["kind"], state_preds[k][0])
        print("beyond the buffers %s: level %d %s, %d states, state hits %s" % (key, r["level"], r["kind"], len(lv), dict(zip((p[0] for p in state_preds), r["state"]["count"]))))
        if probed:
            assert r["step"] is None
            continue
        assert r["state"]["n_states"] == len(lv)
        pairs = []
        for fp, rec in lv.items():
            pn = _norm(S.fixed, rec)
            for s in succ_of[fp]:
                bits = sr.bits_of(step_preds, _view(key, pn), _view(key, _norm(S.fixed, s["words"])), orc.ACTIONS[s["action"]])
                pairs.append((fp, bits))
        assert (r["step"]["n_states"], r["step"]["n_pairs"], r["step"]["n_err"]) == (len(lv), len(pairs), 0), r["level"]
        hitp = sorted(x for x in pairs if x[1])
        assert sorted(tuple(x) for x in r["pairs"]) == hitp and r["n_hit_pairs"] == len(hitp), r["level"]
        for k in range(len(step_preds)):
            mine = [fp for fp, b in hitp if (b >> k) & 1]
            assert (r["step"]["count"][k], r["step"]["min_fp"][k]) == (len(mine), mine[0] if mine else None), (r["level"], step_preds[k][0])
        print("beyond the buffers %s: level %d, %d pairs, step hits %s" % (key, r["level"], len(pairs), dict(zip((p[0] for p in step_preds), r["step"]["count"]))))
    assert sorted(seen) == [(2, False), (3, False), (4, True)], sorted(seen)
    assert sum(seen[(4, True)]["state"]["count"]) > 0 and sum(seen[(3, False)]["step"]["count"]) > 0
