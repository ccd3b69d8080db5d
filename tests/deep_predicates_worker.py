"""Child process of tests/test_deep_predicates_gpu.py: the predicate scans of a checker whose level 1 is a set of harvested states (TEST INFRASTRUCTURE).

Runs with VSRMC_LIB = libvsrmc_hooks.so (ModelChecker.seed_records, csrc/host_test_seed.hpp).  The 1500 sampled states are seeded and every state set is scanned
(where_scan, where_states); then the 150 sampled parents are seeded and every step set is scanned (step_scan, step_pairs).  No oracle and no reference
function here: this process only reports — figures to out.json, the parents' level as the checker stores it (the bag order of a stored record names the
ordinals) to frontier.npz.  The parent process compares everything with the reference.

With `deep` (the two-client spaces) a third seed set — a few of the parents — is seeded, the last state set and the last step set are attached (deep_attach) and
two deepen() passes run: the first inserts level 2 into the seen-set only; the second regenerates level 2, inserts level 3 and probes level 4 (k_probe_where).
Every result of deep_results() is reported with its lists (deep_where_states, deep_step_pairs as parent fingerprint and bits).

usage: deep_predicates_worker.py R C n L seeds.npz out.json frontier.npz [assume_commit_number] [deep]
    assume_commit_number    the policy of the two-client spaces, for Model.from_constants"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def sets_of(key):
    """(tag, predicates) of the state sets and of the step sets of a space: the texts are what this process needs of them"""
    import deep_predicates_reference as dp
    return dp.state_sets(key), dp.step_sets(key)


def deep_passes(m, mc, wr, state_set, step_set, words, off):
    mc.seed_records(words, off)
    ws, wp = m.compile_where(wr.text_of(state_set[1])), m.compile_step(wr.text_of(step_set[1]))
    mc.deep_attach(ws, wp)
    out, listed = dict(passes=[], results=[]), set()
    for _ in range(2):
        a, b = mc.deepen()
        out["passes"].append(dict(inserted={k: a[k] for k in ("level", "n_new", "generated", "viol_mask")}, probed=None if b is None else b["level"]))
        for r in mc.deep_results():
            k = (r["level"], r["kind"])
            if k in listed:
                continue
            listed.add(k)
            fps, bits = mc.deep_where_states(r["level"], probed=r["kind"] == "probed")
            r["states"] = [[int(x), int(y)] for x, y in zip(fps, bits)]
            if r["step"] is not None:
                pf, _po, pb = mc.deep_step_pairs(r["level"])
                r["pairs"] = sorted([int(x), int(y)] for x, y in zip(pf, pb))
            out["results"].append(r)
    return out


def main():
    R, C_, n, L = (int(x) for x in sys.argv[1:5])
    flags = set(sys.argv[8:])
    policy = dict(assume_commit_number=True) if "assume_commit_number" in flags else {}
    z = np.load(sys.argv[5])
    import vsr_tlaplus_amd as vt
    import where_reference as wr
    assert getattr(vt.load(), "vsrmc_test_checker_seed_records", None) is not None, "run me with VSRMC_LIB = libvsrmc_hooks.so"
    state_sets, step_sets = sets_of((R, C_, n, L))
    m = vt.Model.from_constants(R=R, C_=C_, n=n, L=L, **policy)
    mc = vt.ModelChecker(m, table_log2=20, frontier_words=1 << 22, frontier_states=1 << 17, pending_entries=1 << 17)
    out = dict(where={}, step={})
    mc.seed_records(z["words"], z["off"])
    for tag, preds in state_sets:
        w = m.compile_where(wr.text_of(preds))
        t = mc.where_scan(w)
        fps, bits = mc.where_states()
        out["where"][tag] = dict(level=t["level"], n_states=t["n_states"], count=t["count"], min_fp=t["min_fp"], min_index=t["min_index"],
                                 found_at=[None if fp is None else mc.find_fp(fp) for fp in t["min_fp"]],
                                 states=[[int(a), int(b)] for a, b in zip(fps, bits)])
    mc.seed_records(z["pwords"], z["poff"])
    fwords, foff = mc.frontier()
    np.savez(sys.argv[7], words=fwords, off=foff)
    for tag, preds in step_sets:
        w = m.compile_step(wr.text_of(preds))
        t = mc.step_scan(w)
        fps, ords, bits = mc.step_pairs()
        out["step"][tag] = dict({k: t[k] for k in ("level", "n_states", "n_pairs", "n_err", "count", "min_fp", "min_index", "min_ordinal", "min_action")},
                                found_at=[None if fp is None else mc.find_fp(fp) for fp in t["min_fp"]],
                                pairs=[[int(a), int(b), int(c)] for a, b, c in zip(fps, ords, bits)])
    if "deep" in flags:
        out["deep"] = deep_passes(m, mc, wr, state_sets[-1], step_sets[-1], z["dwords"], z["doff"])
    mc.close()
    m.close()
    with open(sys.argv[6], "w") as f:
        json.dump(out, f)
    print("ok", flush=True)


if __name__ == "__main__":
    main()
