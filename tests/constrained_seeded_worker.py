"""Child process of tests/test_constrained_seeded_gpu.py: the constrained level step — k_step_list / k_step_apply / k_step_expand, k_constrain, k_step_keep, the
gated trace — on harvested states of five replicas, four replicas and two clients (TEST INFRASTRUCTURE).

Runs with VSRMC_LIB = libvsrmc_hooks.so.  Per case one checker: the constraints are attached FIRST (both attach calls end in checker_seed, which puts Init back),
then the 1500 sampled states are seeded as level 1 (ModelChecker.seed_records keeps the attachments and restarts their results; the seeds are subject to neither
constraint).  Every expected value comes from tests/constrained_seeded_reference.py: the C++ CPU oracle and hand-written Python predicates.

  (a) the action constraint alone, under invariant mask 3           (b) the state constraint alone
  (c) both, two steps                                                (d) the second action constraint alone, under invariant mask 3
  (e) two clients only: the action constraint with ~RowsDiffer as state constraint under invariant mask 3 (violators among the pruned states)
  scan: step_scan of the space's whole step set on a checker with the action constraint attached (k_step_keep)
  regimes, five replicas only: case (c) again under VSRMC_ACTION_SLICE=64, VSRMC_ACTION_LIST_CAP=64 and VSRMC_CONSTRAIN_GRID=1 — identical figures

Per step: the level figures, action_constraint_results, constraint_results / constraint_pruned, EVERY RECORD of frontier() against the oracle's record of that
fingerprint (deep_seeded_worker.check_records), the violation fields, and traces into a sample of the new states and into every rescued one.

usage: constrained_seeded_worker.py R C n L out.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import constrained_seeded_reference as cs          # noqa: E402
import where_reference as wr                       # noqa: E402
from deep_seeded_worker import check_records       # noqa: E402

M64 = cs.M64
SIZES = dict(table_log2=20, frontier_words=1 << 23, frontier_states=1 << 17, pending_entries=1 << 16)
REGIME_KNOBS = ("VSRMC_ACTION_SLICE", "VSRMC_ACTION_LIST_CAP", "VSRMC_CONSTRAIN_GRID")
N_TRACES, N_TRACES_L3 = 48, 16


def _stride(items, k):
    k = min(k, len(items))
    return [items[(j * len(items)) // k] for j in range(k)]


def _checker(vt, sp, action, state, inv_mask):
    """a checker of the space's model with the programs attached, the state constraint first, then seeded -> (model, checker)"""
    R, C_, n, L = sp.key
    m = vt.Model.from_constants(R=R, C_=C_, n=n, L=L, invariant_mask=inv_mask, **sp.policy)
    mc = vt.ModelChecker(m, device=0, **SIZES)
    if state is not None:
        mc.constrain(m.compile_predicates(wr.text_of(state["preds"])), state["name"])
    if action is not None:
        mc.action_constrain(m.compile_step_predicates(wr.text_of(action["preds"])), action["name"])
    mc.seed_records(*sp.batch())
    assert np.array_equal(mc.level_fps(), np.array(sorted(sp.fps), dtype=np.uint64))
    # the attachments stayed, their results started over: nothing of Init is left (Init fails Client2Committed, and is no state of this search)
    if state is not None:
        assert mc._constraint[1] == state["k"] and mc.constraint_results() == [], "a level-1 figure of Init survived seed_records"
    if action is not None:
        assert mc._action_constraint[1] == action["k"] and mc.action_constraint_results() == []
    assert mc.seen_set_load()[0] == len(sp.recs) and mc.room() == 0
    return m, mc


def check_step(vt, sp, mc, d, st, parents, level, held, distinct, action, state, label, full, kept_before=None):
    """one step against the reference's Step `st`; held: seen-set slots before it; distinct: distinct states before it -> the figures two regimes must agree on"""
    names = vt.ACTION_NAMES
    all_words = sum(st.words_dev(sp, f) for f in st.new)
    # 1. the level figures
    assert d["level"] == level and d["error_code"] == 0, (label, d)
    got = (d["n_new"], d["generated"], list(d["act_generated"]), d["deadlocks"], d["distinct"], d["max_bag"], d["record_words"])
    want = (len(st.kept), st.generated, st.act, st.deadlocks, distinct + len(st.kept), st.max_bag, st.kept_words if state else all_words)
    print("%s level %d: new %d generated %d blocked %d kept %d pruned %d rescued %d" % (label, level, len(st.new), st.generated, st.blocked, len(st.kept),
                                                                                       len(st.pruned), len(st.rescued)), flush=True)
    assert got == want, (label, level, got, want)
    assert np.array_equal(mc.level_fps(), np.array(st.kept, dtype=np.uint64)), (label, level)
    assert mc.level_checksum() == (st.kept_xor, st.kept_sum, len(st.kept)), (label, level)
    occupied = mc.seen_set_load()[0]
    assert occupied == held + len(st.new), (label, level, "a blocked successor holds no slot, a pruned one does", occupied, held, len(st.new))
    fig = dict(level=level, step=got, checksum=[st.kept_xor, st.kept_sum], occupied=occupied)
    # 2. the gate's figures
    if action is not None:
        ai = mc.action_constraint_results(level)
        assert ai == mc.action_constraint_results(0) and (ai["level"], ai["k"]) == (level, action["k"])
        got = {k: ai[k] for k in ("parents", "pairs", "permitted", "blocked", "blocked_act", "blocked_min_fp", "blocked_violating", "blocked_viol_mask",
                                  "blocked_viol_min_fp", "n_new")}
        want = dict(parents=st.parents, pairs=st.generated, permitted=st.permitted, blocked=st.blocked, blocked_act={names[a]: n for a, n in st.blocked_act.items()},
                    blocked_min_fp=st.blocked_min_fp, blocked_violating=st.blocked_violating, blocked_viol_mask=st.blocked_viol_mask,
                    blocked_viol_min_fp=st.blocked_viol_min_fp, n_new=len(st.new))
        assert got == want, (label, level, got, want)
        fig["action"] = got
        fig["relisted"], fig["slices"] = ai["relisted"], ai["slices"]
    # 3. the filter's figures
    if state is not None:
        ci = mc.constraint_results(level)
        assert ci == mc.constraint_results(0) and (ci["level"], ci["k"]) == (level, state["k"])
        got = {k: ci[k] for k in ("n_states", "kept", "pruned", "kept_xor", "kept_sum", "kept_max_bag", "kept_words", "pruned_min_fp", "pruned_count", "pruned_min_fp_k")}
        want = dict(n_states=len(st.new), kept=len(st.kept), pruned=len(st.pruned), kept_xor=st.kept_xor, kept_sum=st.kept_sum, kept_max_bag=st.kept_max_bag,
                    kept_words=st.kept_words, pruned_min_fp=st.pruned_min_fp, pruned_count=st.pruned_count, pruned_min_fp_k=st.pruned_min_fp_k)
        assert got == want, (label, level, got, want)
        assert np.array_equal(mc.constraint_pruned(), np.array(st.pruned, dtype=np.uint64)), (label, level)
        fig["state"] = got
    # 5. violations: over the permitted-new states only, kept or pruned; a blocked violator is counted (above) and never reported
    if st.viol:
        vfp, vmask = min(st.viol), 0
        for v in st.viol.values():
            vmask |= v
        assert (d["viol_fp"], d["viol_mask"]) == (vfp, vmask), (label, level, d["viol_fp"], d["viol_mask"], vfp, vmask)
        if vfp in set(st.pruned):                                    # as test_constraint_gpu.py::test_built_in_violation_on_a_pruned_state pins it at three replicas
            assert d["viol_index"] == M64 and mc.find_fp(vfp) is None and vfp in set(int(f) for f in mc.constraint_pruned())
        else:
            assert d["viol_index"] == mc.find_fp(vfp) is not None
        assert mc.violation is not None and mc.violation["fp"] == vfp
        if level == 2:
            t = mc.trace_fp(2, vfp)                                  # the behaviour into it, out of model or not: [a seed with a permitted step into it, the state]
            pi = cs.trace_parent(st, parents, vfp)
            assert len(t) == 2 and sp.norm(t[0][1]) == sp.norm(parents[pi][1][0]) and sp.orc.fingerprint(sp.P, t[1][1])[0] == vfp, (label, vfp)
            assert sp.orc.invariants(sp.params(st.inv_mask), t[1][1]) == st.viol[vfp]
    else:
        assert d["viol_mask"] == 0 and d["viol_fp"] == M64, (label, level, d["viol_fp"], d["viol_mask"])
    fig["viol"] = [d["viol_fp"], d["viol_mask"]]
    if not full:
        return fig
    # 4. EVERY record of the level: the oracle's record of that fingerprint under the smallest auxkey among its permitted producers, bag order aside; exactly
    #    the kept states, no record of a pruned one, every rescued state the constraint keeps among them
    check_records(sp, mc, {f: st.producers[f] for f in st.kept}, "%s level %d" % (label, level))
    for f in st.rescued_kept:
        assert mc.find_fp(f) is not None, (label, level, "a rescued state is missing", f)
    for f in _stride(st.pruned, 16) + [f for f in st.rescued if f not in set(st.rescued_kept)]:
        assert mc.find_fp(f) is None, (label, level, "a pruned state is still in the level", f)
    # 6. traces
    act_f = action["preds"][action["k"]][2] if action is not None else (lambda p, c, a: True)
    if level == 2:
        sample = _stride(st.kept, N_TRACES) + st.rescued_kept
        for fp in sample:
            pi = cs.trace_parent(st, parents, fp)
            idx = mc.find_fp(fp)
            assert idx is not None, (label, fp)
            t = mc.trace(2, idx)
            assert len(t) == 2 and t[0][0] == "Initial predicate", (label, t)
            assert sp.norm(t[0][1]) == sp.norm(parents[pi][1][0]), (label, "trace: the parent is the seed of the smallest key among the PERMITTED producers", fp)
            via = set((names[a], sp.norm(s["words"])) for _ak, i, s, a in st.producers[fp] if i == pi)
            assert (t[1][0], sp.norm(t[1][1])) in via, (label, "trace: the step is a permitted edge of that seed", fp, t[1][0])
            permitted_from = set(i for _ak, i, _s, _a in st.producers[fp])
            for b in st.blocked_from.get(fp, ()):                    # a rescued state: its blocked producer is not the printed parent
                if b not in permitted_from:
                    assert sp.norm(t[0][1]) != sp.norm(parents[b][1][0]), (label, "trace: through a blocked edge", fp)
        fig["traces"] = len(sample)
    else:
        sample = _stride(st.kept, N_TRACES_L3)
        seeds, middle = set(sp.fps), set(kept_before)
        for fp in sample:
            t = mc.trace(level, mc.find_fp(fp))
            assert len(t) == 3 and t[0][0] == "Initial predicate", (label, fp, len(t))
            fps = [sp.orc.fingerprint(sp.P, rec)[0] for _a, rec in t]
            assert fps[0] in seeds and fps[1] in middle and fps[2] == fp, (label, "trace: seed, a KEPT level-2 state, the state", fp)
            assert fps[1] == parents[cs.trace_parent(st, parents, fp)][0], (label, "trace: the parent of the smallest key among the permitted producers", fp)
            for k in (1, 2):                                         # every step exists, with that action, and is a permitted one
                succ = [(names[s["action"]], s["fp"]) for s in sp.orc.successors(sp.P, t[k - 1][1])]
                assert (t[k][0], fps[k]) in succ, (label, fp, k)
                assert act_f(sp.view(t[k - 1][1]), sp.view(t[k][1]), t[k][0]), (label, "trace: a blocked step", fp, k)
        fig["traces"] = len(sample)
    return fig


def run_case(vt, sp, label, action, state, inv_mask, steps, parents, env=None, full=True):
    """attach, seed, step once per Step of `steps` (parents[k]: the parents of steps[k]) -> [figures per step]"""
    for k in REGIME_KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env or {})
    t0 = time.time()
    m, mc = _checker(vt, sp, action, state, inv_mask)
    out = []
    try:
        held = distinct = len(sp.recs)
        kept_before = None
        for k, st in enumerate(steps):
            assert mc.room() == 0
            d = mc.step()
            out.append(check_step(vt, sp, mc, d, st, parents[k], 2 + k, held, distinct, action, state, label, full, kept_before))
            held += len(st.new)
            distinct += len(st.kept)
            kept_before = st.kept
    finally:
        mc.close()
        m.close()
        for k in REGIME_KNOBS:
            os.environ.pop(k, None)
    print("%s: %.1f s on the device side" % (label, time.time() - t0), flush=True)
    return out


def run_scan(vt, sp, action, ref):
    """7. step_scan of the space's whole step set on a checker with the action constraint attached: the permitted pairs only (k_step_keep).  Which pair is which
    ordinal: the level's own records through get_next_states, whose rows are held against the oracle's successors here"""
    preds = cs.PROGRAMS[sp.key]["step_set"]
    act_f = action["preds"][action["k"]][2]
    m, mc = _checker(vt, sp, action, None, 1)
    try:
        w = m.compile_step_predicates(wr.text_of(preds))
        t = mc.step_scan(w)
        fw, fo = mc.frontier()
        nx = m.get_next_states(fw, fo, cap_succ=ref.generated + 64, cap_words=(ref.generated + 64) * int(m.layout.max_record_words))
        assert len(nx) == ref.generated
        seed_of = {f: i for i, f in enumerate(sp.fps)}
        exp = sp.expansion(sp.seeds(), cached=True)
        by_parent = {}
        for s in nx:
            assert s["err"] == 0
            by_parent.setdefault(s["parent"], []).append(s)
        hits, n_permitted = [[] for _ in preds], 0
        for k in range(len(fo) - 1):
            frec = fw[int(fo[k]): int(fo[k + 1])]
            pfp = sp.orc.fingerprint(sp.P, frec)[0]
            _rec, pv, succ, views = exp[seed_of[pfp]][0]
            assert sp.norm(frec) == sp.norm(_rec)
            view_of = {(s["action"], sp.norm(s["words"])): v for s, v in zip(succ, views)}
            mine = by_parent.get(k, [])
            assert sorted((s["action"], sp.norm(s["words"])) for s in mine) == sorted((s["action"], sp.norm(s["words"])) for s in succ), ("get_next_states", k)
            for s in mine:
                cv, a = view_of[(s["action"], sp.norm(s["words"]))], vt.ACTION_NAMES[s["action"]]
                if not act_f(pv, cv, a):
                    continue
                n_permitted += 1
                for j, (_nm, _t, f) in enumerate(preds):
                    if f(pv, cv, a):
                        hits[j].append((pfp, int(s["ordinal"]), int(s["action"])))
        assert (t["level"], t["n_states"], t["n_pairs"], t["n_err"]) == (1, len(sp.recs), n_permitted, 0), (t["n_pairs"], n_permitted)
        assert n_permitted == ref.permitted < ref.generated
        for j, (nm, _t, _f) in enumerate(preds):
            assert t["count"][j] == len(hits[j]), (nm, t["count"][j], len(hits[j]))
            if hits[j]:
                assert (t["min_fp"][j], t["min_ordinal"][j], t["min_action"][j]) == min(hits[j]), (nm, t["min_fp"][j], t["min_ordinal"][j], min(hits[j]))
                assert t["min_index"][j] == mc.find_fp(t["min_fp"][j]) is not None
            else:
                assert t["min_fp"][j] is None and t["min_ordinal"][j] is None and t["min_action"][j] is None, nm
        print("step_scan: %d permitted pairs of %d, %s" % (n_permitted, ref.generated, dict(zip((p[0] for p in preds), t["count"]))), flush=True)
        return dict(n_pairs=t["n_pairs"], count=t["count"])
    finally:
        mc.close()
        m.close()


def main():
    key = tuple(int(x) for x in sys.argv[1:5])
    out_path = sys.argv[5]
    t_start = time.time()
    import vsr_tlaplus_amd as vt
    from oracle import orc
    assert getattr(vt.load(), "vsrmc_test_checker_seed_records", None) is not None, "run me with VSRMC_LIB = libvsrmc_hooks.so"
    sp = cs.Space(orc, key)
    pr = cs.PROGRAMS[key]
    seeds, earlier = sp.seeds(), set(sp.fps)
    out = dict(key=list(key), seeds=len(sp.recs), cases={})
    # (a) the action constraint alone, under invariant mask 3: the violating successors it blocks are counted, the ones it permits reported
    a = cs.step(sp, seeds, earlier, pr["action"], None, 3, seeds=True)
    assert not a.ties
    out["cases"]["a"] = run_case(vt, sp, "(a) %s" % pr["action"]["name"], pr["action"], None, 3, [a], [seeds])
    out["scan"] = run_scan(vt, sp, pr["action"], a)
    # (b) the state constraint alone
    b = cs.step(sp, seeds, earlier, None, pr["state"], 1, seeds=True)
    assert not b.ties
    out["cases"]["b"] = run_case(vt, sp, "(b) %s" % pr["state"]["name"], None, pr["state"], 1, [b], [seeds])
    # (c) both, two steps
    c2, c3, parents3 = cs.two_levels(sp, pr["action"], pr["state"])
    out["cases"]["c"] = run_case(vt, sp, "(c) both", pr["action"], pr["state"], 1, [c2, c3], [seeds, parents3])
    # (d) the second action constraint alone, under invariant mask 3
    d = cs.step(sp, seeds, earlier, pr["second"], None, 3, seeds=True)
    assert not d.ties
    out["cases"]["d"] = run_case(vt, sp, "(d) %s" % pr["second"]["name"], pr["second"], None, 3, [d], [seeds])
    # (e) two clients: violators among the states the state constraint prunes
    if pr["e_state"] is not None:
        e = cs.step(sp, seeds, earlier, pr["action"], pr["e_state"], 3, seeds=True)
        assert not e.ties and any(f in set(e.pruned) for f in e.viol)
        out["cases"]["e"] = run_case(vt, sp, "(e) %s, %s" % (pr["action"]["name"], pr["e_state"]["name"]), pr["action"], pr["e_state"], 3, [e], [seeds])
    # 8. the slice and grid regimes, five replicas: the figures of case (c) again, identical
    if key[0] == 5:
        def comparable(rows):
            return [{k: v for k, v in r.items() if k not in ("relisted", "slices", "traces")} for r in rows]
        out["regimes"] = {}
        for tag, env in (("slice64", dict(VSRMC_ACTION_SLICE="64")), ("listcap64", dict(VSRMC_ACTION_LIST_CAP="64")), ("grid1", dict(VSRMC_CONSTRAIN_GRID="1"))):
            rows = run_case(vt, sp, "(c) both, %s" % tag, pr["action"], pr["state"], 1, [c2, c3], [seeds, parents3], env=env, full=False)
            assert comparable(rows) == comparable(out["cases"]["c"]), tag
            out["regimes"][tag] = dict(slices=[r["slices"] for r in rows], relisted=[r["relisted"] for r in rows])
        assert sum(out["regimes"]["listcap64"]["relisted"]) > 0, "no slice overflowed the list of 64 entries"
        assert out["regimes"]["slice64"]["slices"][0] >= len(sp.recs) // 64 and sum(out["cases"]["c"][k]["relisted"] for k in (0, 1)) == 0
    out["seconds"] = time.time() - t_start
    with open(out_path, "w") as f:
        json.dump(out, f)
    print("ok %.1f s" % out["seconds"], flush=True)


if __name__ == "__main__":
    main()
