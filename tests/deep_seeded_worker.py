"""Child process of tests/test_deep_actions_gpu.py: k_expand itself on harvested states (TEST INFRASTRUCTURE).

Runs with VSRMC_LIB = libvsrmc_hooks.so: a checker is seeded with the harvested records (ModelChecker.seed_records, csrc/host_test_seed.hpp) and
the ordinary level machinery runs over that level.  Every expected value comes from the C++ CPU oracle alone: with S the seeds,

    generated        = number of successors of S                      act_generated[a] = of action a
    deadlocks        = seeds without successor                        n_new            = |fp(succ(S)) \\ fp(S)|
    level_fps()      = that set, level_checksum() its xor and sum     frontier()       = per fingerprint, the oracle's record (normalised)
    viol_fp / _mask  = the smallest violating new fingerprint / the or of the new states' verdicts
    trace(2, i)      = [seed, state]: the seed with the smallest (canonical auxkey of the successor, low 45 bits of its own fingerprint) among the
                       seeds that produce the state (csrc/vsr_model.hpp: the meta word), the action one by which that seed produces it

A seed set is not a BFS level: its image can hold one fingerprint under two canonical auxkeys, which a single-pass level (exact_ties = 0) refuses by
design (VSRMC_E_STATE).  The oracle decides: a set whose image has such fingerprints is split by the header's aux_svc (the timer count, the aux variable
that differs) and every part is stepped on its own; seeds that still produce one are left out of that run (at most 1 %, printed).  exact_ties = 1 takes
the whole set and must resolve every such fingerprint to the smallest auxkey.

usage: deep_seeded_worker.py R C n L seeds.npz out.json [full | viol | small | c2] [assume_commit_number] [generous]
    full, viol, small, c2   what runs besides the two stored steps (main)
    assume_commit_number    the policy of the two-client spaces, for the oracle's Params and for Model.from_constants alike
    generous                the buffers of test_a_tile_that_overflows_the_work_list_is_taken_again_in_pieces (for a run under VSRMC_CCAP)
"""
import collections
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

M64 = (1 << 64) - 1
PFP_MASK = (1 << 45) - 1
E_ARG, E_REP = -1, -5


def _pow2_at_least(x):
    k = 1
    while k < x:
        k *= 2
    return k


class Case:
    """the oracle's side of one seed set under one invariant mask.  `orc` is the oracle module of the model: oracle/orc.py with key = (R, C, n, L),
    or oracle/orc2.py / orc3.py with key = (R, n, L) — then `make_model(vt, inv_mask)` builds the product's model of the same constants (no SYMMETRY: one
    view hash per record) and `verdict(words, inv_mask)` gives the oracle's verdict on a record where orc.invariants alone does not (an evaluation error
    that the kernels report as a violation)."""

    def __init__(self, orc, key, recs, succ, inv_mask=1, make_model=None, verdict=None, policy=None):
        self.orc, self.key, self.recs, self.succ = orc, key, recs, succ
        self.inv_mask, self.make_model, self.verdict = inv_mask, make_model, verdict
        self.policy = dict(policy or {})                            # e.g. assume_commit_number=True: the oracle's Params and the product's model alike
        self.P = orc.Params(*key, invariant_mask=inv_mask, **self.policy)
        self.fps = [orc.fingerprint(self.P, r)[0] for r in recs]
        assert len(set(self.fps)) == len(recs), "the seeds are distinct states"
        seed_fp = set(self.fps)
        self.generated = 0
        self.act = [0] * 16
        self.deadlocks = []
        self.by_fp = collections.defaultdict(list)                  # new fingerprint -> [(auxkey, seed number, successor)]
        self.enabled = collections.Counter()                        # action -> seeds in which it is enabled
        self.viol = {}                                              # new violating fingerprint -> verdict
        for i, ss in enumerate(succ):
            if not ss:
                self.deadlocks.append(self.fps[i])
            for a in set(s["action"] for s in ss):
                self.enabled[a] += 1
            for s in ss:
                self.generated += 1
                self.act[s["action"]] += 1
                if s["fp"] in seed_fp:
                    continue
                self.by_fp[s["fp"]].append((s["auxkey"], i, s))
                inv = self.verdict_of(s["words"]) if (verdict or inv_mask != 1) else s["inv"]
                if inv:
                    self.viol[s["fp"]] = self.viol.get(s["fp"], 0) | inv
        self.new = sorted(self.by_fp)
        self.ties = [f for f, v in self.by_fp.items() if len(set(ak for ak, _i, _s in v)) > 1]
        self.new_words_dev = 0                                      # words of the new level in device layout (wire + one view hash per permutation)
        perms = 1
        for k in range(2, (1 if make_model else key[2]) + 1):
            perms *= k
        for f in self.new:
            self.new_words_dev += len(self.by_fp[f][0][2]["words"]) + perms
        self.seed_words_dev = sum(len(r) + perms for r in recs)

    def verdict_of(self, words):
        return self.verdict(words, self.inv_mask) if self.verdict else self.orc.invariants(self.P, words)

    def tie_producers(self):
        return sorted(set(i for f in self.ties for _ak, i, _s in self.by_fp[f]))

    def batch(self):
        return np.concatenate(self.recs), np.cumsum([0] + [len(r) for r in self.recs]).astype(np.uint64)

    def norm(self, words):
        return tuple(int(x) for x in self.orc.normalise(self.P, words))


def make_checker(vt, case, exact, frontier_words=None, generous=False):
    """generous: the buffers of test_a_tile_that_overflows_the_work_list_is_taken_again_in_pieces (every re-launch leaves partly used chunks behind)"""
    if case.make_model:
        m = case.make_model(vt, int(case.P.arr[7]))
    else:
        R, C_, n, L = case.key
        m = vt.Model.from_constants(R=R, C_=C_, n=n, L=L, invariant_mask=int(case.P.arr[7]), **case.policy)
    fw = frontier_words or _pow2_at_least(max(1 << 24, 2 * max(case.new_words_dev, case.seed_words_dev)))
    fs = _pow2_at_least(max(1 << 16, 4 * max(len(case.new), len(case.recs))))
    if generous:
        mc = vt.ModelChecker(m, table_log2=22, frontier_words=1 << 26, frontier_states=1 << 22, pending_entries=1 << 21, exact_ties=bool(exact))
    else:
        mc = vt.ModelChecker(m, table_log2=23, frontier_words=fw, frontier_states=fs, pending_entries=1 << 22 if exact else 1 << 16,
                             exact_ties=bool(exact))
    return m, mc


def check_records(case, mc, by_fp, label):
    """every record of the newest level (mc.frontier()): the oracle's record of that fingerprint (under the winning auxkey), bag order aside.  by_fp: fingerprint
    -> [(auxkey, producer number, successor, ..)] of exactly the states the level must hold; case: what gives orc, P and norm().  Shared with
    tests/constrained_seeded_worker.py, where by_fp holds the PERMITTED producers of the states the state constraint keeps."""
    words, off = mc.frontier()
    assert len(off) - 1 == len(by_fp), (label, len(off) - 1, len(by_fp))
    seen = set()
    for k in range(len(off) - 1):
        rec = words[int(off[k]): int(off[k + 1])]
        fp, ak = case.orc.fingerprint(case.P, rec)
        cands = by_fp.get(fp)
        assert cands, (label, "a record of the level is no successor of a seed", k)
        best = min(c[0] for c in cands)
        assert ak == best, (label, "the smallest canonical auxkey wins", k, ak, best)
        assert case.norm(rec) in set(case.norm(c[2]["words"]) for c in cands if c[0] == best), (label, "record", k, fp)
        seen.add(fp)
    assert len(seen) == len(by_fp), label


def check_level(vt, case, mc, d, label, n_traces=48):
    """everything a stored step over the seeds must have left, against the oracle"""
    assert d["level"] == 2 and d["error_code"] == 0, (label, d)
    assert d["generated"] == case.generated, (label, d["generated"], case.generated)
    assert list(d["act_generated"]) == case.act, (label, d["act_generated"], case.act)
    assert d["deadlocks"] == len(case.deadlocks), (label, d["deadlocks"], len(case.deadlocks))
    assert d["n_new"] == len(case.new), (label, d["n_new"], len(case.new))
    assert d["distinct"] == len(case.recs) + len(case.new)
    want = np.array(case.new, dtype=np.uint64)
    assert np.array_equal(mc.level_fps(), want), label
    x = s_ = 0
    for f in case.new:
        x ^= f
        s_ = (s_ + f) & M64
    assert mc.level_checksum() == (x, s_, len(case.new)), label
    # every record of the level: the oracle's record of that fingerprint (under the winning auxkey), bag order aside
    assert len(case.by_fp) == len(case.new)
    check_records(case, mc, case.by_fp, label)
    # violations
    if case.viol:
        vfp = min(case.viol)
        vmask = 0
        for v in case.viol.values():
            vmask |= v
        assert (d["viol_fp"], d["viol_mask"]) == (vfp, vmask), (label, d["viol_fp"], d["viol_mask"], vfp, vmask)
        idx = d["viol_index"]
        t = mc.trace(2, idx)
        assert case.orc.fingerprint(case.P, t[-1][1])[0] == vfp and case.verdict_of(t[-1][1]) != 0
    else:
        assert d["viol_mask"] == 0 and d["viol_fp"] == M64, (label, d["viol_fp"], d["viol_mask"])
    # traces: [the seed the meta word names, the state]
    step = max(1, len(case.new) // n_traces)
    sample = case.new[::step] + [f for f in case.ties if f in case.by_fp][:16] + (sorted(case.viol)[:4])
    for fp in sample:
        cands = case.by_fp[fp]
        _key, pi = min(((a, case.fps[i] & PFP_MASK), i) for a, i, _s in cands)
        idx = mc.find_fp(fp)
        assert idx is not None, (label, fp)
        t = mc.trace(2, idx)
        assert len(t) == 2 and t[0][0] == "Initial predicate", (label, t)
        assert case.norm(t[0][1]) == case.norm(case.recs[pi]), (label, "trace: the parent is the seed of the smallest key", fp)
        via = set((vt.ACTION_NAMES[s["action"]], case.norm(s["words"])) for s in case.succ[pi] if s["fp"] == fp)
        assert (t[1][0], case.norm(t[1][1])) in via, (label, fp, t[1][0])
    return len(sample)


def run_step(vt, orc, key, recs, succ, exact, inv_mask=1, label="", generous=False, **model_kw):
    case = Case(orc, key, recs, succ, inv_mask, **model_kw)
    m, mc = make_checker(vt, case, exact, generous=generous)
    try:
        mc.seed_records(*case.batch())
        assert np.array_equal(mc.level_fps(), np.array(sorted(case.fps), dtype=np.uint64)), label
        before = mc.extra_launches()
        t0 = time.time()
        d = mc.step()
        dt = time.time() - t0
        redo = mc.extra_launches() - before                           # lists of overflowed tiles launched again (k_expand: s_over, redo_overflowed_tiles)
        n_tr = check_level(vt, case, mc, d, label)
    finally:
        mc.close()
        m.close()
    return dict(label=label, seeds=len(recs), generated=case.generated, n_new=len(case.new), ties=len(case.ties), violators=len(case.viol),
                act_generated=case.act, traces=n_tr, step_seconds=dt, expand_ms=d["expand_ms"], redo_launches=redo)


def parts_without_ties(orc, key, recs, succ, **model_kw):
    """the seed set as parts a single-pass level can take -> ([part: list of seed numbers], seeds left out)"""
    whole = Case(orc, key, recs, succ, **model_kw)
    if not whole.ties:
        return [list(range(len(recs)))], 0
    groups = collections.defaultdict(list)
    for i, r in enumerate(recs):
        groups[(int(r[0]) >> 8) & 7].append(i)                      # aux_svc of the header
    parts, left = [], 0
    for g in sorted(groups):
        idx = groups[g]
        c = Case(orc, key, [recs[i] for i in idx], [succ[i] for i in idx], **model_kw)
        drop = set(c.tie_producers())
        left += len(drop)
        parts.append([i for k, i in enumerate(idx) if k not in drop])
    return parts, left


def extras_512(vt, orc, key, recs, succ, out):
    """the rest of the family at SPEC 512: probe, terminal scan, select, a level beyond the record buffers, the refusals of the hook"""
    from deep_harvest import COUNTED
    case = Case(orc, key, recs, succ)
    m, mc = make_checker(vt, case, 0)
    try:
        # refusals first: nothing is launched, the checker stays where it was (at Init)
        init_fps = mc.level_fps()
        words, off = case.batch()
        lay = m.layout
        filler = recs[0][int(lay.fixed_words):][:1] if len(recs[0]) > int(lay.fixed_words) else np.array([1], dtype=np.uint64)
        long_rec = np.concatenate([recs[0][: int(lay.fixed_words)]] + [filler] * (int(lay.max_bag) + 1))
        long_rec[0] = (int(long_rec[0]) & ~0xFF) | (int(lay.max_bag) + 1)
        for bad_w, bad_o, code in ((long_rec, np.array([0, len(long_rec)], dtype=np.uint64), E_REP),                   # a bag beyond the layout
                                   (np.concatenate([recs[0], recs[0]]), np.array([0, len(recs[0]), 2 * len(recs[0])], dtype=np.uint64), E_ARG),   # duplicates
                                   (recs[0], np.array([0, len(recs[0]) - 1], dtype=np.uint64), E_ARG),                 # length against the header
                                   (words, off[: 1], E_ARG)):                                                           # no record
            try:
                mc.seed_records(bad_w, bad_o)
            except vt.VsrmcError as e:
                assert e.code == code, (e.code, code, str(e))
            else:
                raise AssertionError("seed_records accepted a bad batch")
            assert np.array_equal(mc.level_fps(), init_fps)
        # more records than the index arrays (2048) / than half of the seen-set's 2048 slots / more words than the record buffer (4096) holds
        for kw, hi in ((dict(table_log2=16, frontier_words=1 << 20, frontier_states=2048), 2049),
                       (dict(table_log2=11, frontier_words=1 << 20, frontier_states=2048), 2048),
                       (dict(table_log2=16, frontier_words=4096, frontier_states=2048), 256)):
            small = vt.ModelChecker(m, pending_entries=1 << 16, **kw)
            try:
                small.seed_records(np.concatenate(recs[:hi]), np.cumsum([0] + [len(r) for r in recs[:hi]]).astype(np.uint64))
            except vt.VsrmcError as e:
                assert e.code == E_ARG, str(e)
            else:
                raise AssertionError("seed_records accepted more records than the buffers hold")
            finally:
                small.close()
        # probe straight after seeding
        mc.seed_records(words, off)
        p = mc.probe()
        assert p["generated"] == case.generated and p["viol_mask"] == 0, (p["generated"], case.generated)
        assert mc.probe_violators() == []
        # terminal scan and select on the seeded level
        mc.seed_records(words, off)
        t = mc.terminal_scan()
        assert (t["level"], t["n_states"], t["n_terminal"]) == (1, len(recs), len(case.deadlocks)), t
        assert t["min_fp"] == (min(case.deadlocks) if case.deadlocks else None)
        for a in COUNTED:
            _w, _o, n_match = mc.select(1 << a, 16)
            assert n_match == case.enabled[a], (vt.ACTION_NAMES[a], n_match, case.enabled[a])
        out["terminal"] = len(case.deadlocks)
        out["select"] = {vt.ACTION_NAMES[a]: case.enabled[a] for a in COUNTED}
    finally:
        mc.close()
        m.close()
    # a probe and a stored step whose image violates: the same seeds under invariant mask 3 (AcknowledgedWritesExistOnMajority, VSR.tla:937-943)
    case3 = Case(orc, key, recs, succ, inv_mask=3)
    assert case3.viol, "no violating successor under mask 3: the violation checks would be vacuous"
    m, mc = make_checker(vt, case3, 0)
    try:
        mc.seed_records(*case3.batch())
        p = mc.probe()
        vmask = 0
        for v in case3.viol.values():
            vmask |= v
        assert (p["generated"], p["viol_fp"], p["viol_mask"]) == (case3.generated, min(case3.viol), vmask), p
        assert mc.probe_violators() == sorted(case3.viol)
        out["probe_violators"] = len(case3.viol)
    finally:
        mc.close()
        m.close()
    # one level beyond the record buffers: the buffers hold the seeds, not their image
    fw = _pow2_at_least(case.seed_words_dev + (1 << 20))
    assert case.new_words_dev > fw, "the record buffers of this run must be too small for level 2"
    m, mc = make_checker(vt, case, 0, frontier_words=fw)
    try:
        mc.seed_records(*case.batch())
        a, _b = mc.deepen()
        x = s_ = 0
        for f in case.new:
            x ^= f
            s_ = (s_ + f) & M64
        got = (a["level"], a["n_new"], a["generated"], list(a["act_generated"]), a["fp_xor"], a["fp_sum"], a["viol_mask"])
        assert got == (2, len(case.new), case.generated, case.act, x, s_, 0), (got[:3], len(case.new), case.generated)
        out["deepen"] = dict(frontier_words=fw, level2_words=case.new_words_dev, n_new=a["n_new"])
    finally:
        mc.close()
        m.close()


def _xor_sum(fps):
    x = s_ = 0
    for f in fps:
        x ^= f
        s_ = (s_ + f) & M64
    return x, s_


def extras_c2(vt, orc, key, recs, succ, out, policy):
    """the rest of the family at two clients (SPEC 323 at (3,2,3,L), generic at (3,2,2,1)): probe, terminal scan, select, two passes beyond the record
    buffers — the first inserts level 2 into the seen-set only, the second regenerates it from the seeds and inserts level 3"""
    from deep_harvest import COUNTED_C2
    case = Case(orc, key, recs, succ, policy=policy)
    assert not case.ties
    words, off = case.batch()
    m, mc = make_checker(vt, case, 0)
    try:
        mc.seed_records(words, off)
        p = mc.probe()
        assert p["generated"] == case.generated and p["viol_mask"] == 0, (p["generated"], case.generated)
        assert mc.probe_violators() == []
        mc.seed_records(words, off)
        t = mc.terminal_scan()
        assert (t["level"], t["n_states"], t["n_terminal"]) == (1, len(recs), len(case.deadlocks)), t
        assert t["min_fp"] == (min(case.deadlocks) if case.deadlocks else None)
        for a in COUNTED_C2:
            _w, _o, n_match = mc.select(1 << a, 16)
            assert n_match == case.enabled[a], (vt.ACTION_NAMES[a], n_match, case.enabled[a])
        out["terminal"] = len(case.deadlocks)
        out["select"] = {vt.ACTION_NAMES[a]: case.enabled[a] for a in COUNTED_C2}
    finally:
        mc.close()
        m.close()
    # the probe of an image that violates: the same seeds under invariant mask 3 (AcknowledgedWritesExistOnMajority, VSR.tla:937-943)
    case3 = Case(orc, key, recs, succ, inv_mask=3, policy=policy)
    assert case3.viol, "no violating successor under mask 3: the violation checks would be vacuous"
    m, mc = make_checker(vt, case3, 0)
    try:
        mc.seed_records(*case3.batch())
        p = mc.probe()
        vmask = 0
        for v in case3.viol.values():
            vmask |= v
        assert (p["generated"], p["viol_fp"], p["viol_mask"]) == (case3.generated, min(case3.viol), vmask), p
        assert mc.probe_violators() == sorted(case3.viol)
        out["probe_violators"] = len(case3.viol)
    finally:
        mc.close()
        m.close()
    # level 3 by the oracle: the successors of level 2 that are neither seeds nor of level 2
    known = set(case.fps) | set(case.new)
    gen3, act3, new3, viol3 = 0, [0] * 16, {}, 0
    perms = 1
    for k in range(2, key[2] + 1):
        perms *= k
    for f in case.new:
        for s in orc.successors(case.P, case.by_fp[f][0][2]["words"]):
            gen3 += 1
            act3[s["action"]] += 1
            if s["fp"] not in known:
                new3.setdefault(s["fp"], (set(), len(s["words"]) + perms))[0].add(s["auxkey"])
                viol3 |= s["inv"]
    assert all(len(aks) == 1 for aks, _n in new3.values()), "level 3 holds one fingerprint under two auxkeys"
    words3 = sum(n for _aks, n in new3.values())
    fw = _pow2_at_least(case.seed_words_dev)
    assert max(case.new_words_dev, words3) > fw, "the record buffers of this run must be too small for a level it passes"
    m, mc = make_checker(vt, case, 0, frontier_words=fw)
    try:
        mc.seed_records(words, off)
        a, b = mc.deepen()
        got = (a["level"], a["n_new"], a["generated"], list(a["act_generated"]), a["fp_xor"], a["fp_sum"], a["viol_mask"])
        assert got == (2, len(case.new), case.generated, case.act) + _xor_sum(case.new) + (0,), (got[:3], len(case.new), case.generated)
        assert b is None or (b["level"], b["generated"], b["viol_mask"]) == (3, gen3, viol3), b      # (a probed level generates what it generates when it is inserted)
        a, b = mc.deepen()
        got = (a["level"], a["n_new"], a["generated"], list(a["act_generated"]), a["fp_xor"], a["fp_sum"], a["viol_mask"])
        assert got == (3, len(new3), gen3, act3) + _xor_sum(new3) + (viol3,), (got[:3], len(new3), gen3)
        assert a["distinct"] == len(recs) + len(case.new) + len(new3)
        out["deepen"] = dict(frontier_words=fw, level2_words=case.new_words_dev, level3_words=words3, n_new=[len(case.new), len(new3)], generated=[case.generated, gen3],
                             act_generated3=act3)
    finally:
        mc.close()
        m.close()


def main():
    flags = set(sys.argv[7:])
    generous = "generous" in flags
    policy = dict(assume_commit_number=True) if "assume_commit_number" in flags else {}
    key = tuple(int(x) for x in sys.argv[1:5])
    z = np.load(sys.argv[5])
    out_path = sys.argv[6]
    full = "full" in flags                                            # SPEC 512: the whole family
    viol = full or "viol" in flags or "c2" in flags                   # a stored step whose image violates (invariant mask 3)
    import vsr_tlaplus_amd as vt
    from oracle import orc
    assert getattr(vt.load(), "vsrmc_test_checker_seed_records", None) is not None, "run me with VSRMC_LIB = libvsrmc_hooks.so"
    words, off = z["words"], z["off"]
    recs = [words[int(off[i]): int(off[i + 1])].copy() for i in range(len(off) - 1)]
    P = orc.Params(*key, **policy)
    succ = [orc.successors(P, r) for r in recs]
    out = dict(key=list(key), seeds=len(recs), runs=[])
    parts, left = parts_without_ties(orc, key, recs, succ, policy=policy)
    assert left * 100 <= len(recs), ("more than 1 % of the seeds left out of the single-pass run", left, len(recs))
    print("seeds %d, parts %s, left out of the single-pass run %d" % (len(recs), [len(p) for p in parts], left), flush=True)
    out["left_out"], out["parts"] = left, [len(p) for p in parts]
    small = "small" in flags                                        # hand-built records among a few harvested ones
    assert small or max(len(p) for p in parts) >= 4096
    for k, part in enumerate(parts):
        out["runs"].append(run_step(vt, orc, key, [recs[i] for i in part], [succ[i] for i in part], 0, label="exact_ties=0 part %d" % k, policy=policy, generous=generous))
        print(json.dumps(out["runs"][-1]), flush=True)
    out["runs"].append(run_step(vt, orc, key, recs, succ, 1, label="exact_ties=1", policy=policy, generous=generous))
    print(json.dumps(out["runs"][-1]), flush=True)
    if viol:
        out["runs"].append(run_step(vt, orc, key, recs, succ, 0, inv_mask=3, label="exact_ties=0 mask 3", policy=policy))
        assert out["runs"][-1]["violators"] > 0
        print(json.dumps(out["runs"][-1]), flush=True)
    if full:
        extras_512(vt, orc, key, recs, succ, out)
    if "c2" in flags:
        extras_c2(vt, orc, key, recs, succ, out, policy)
    with open(out_path, "w") as f:
        json.dump(out, f)
    print("ok", flush=True)


if __name__ == "__main__":
    main()
