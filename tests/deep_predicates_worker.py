"""Child process of tests/test_deep_predicates_gpu.py: the predicate scans of a checker whose level 1 is a set of harvested states (TEST INFRASTRUCTURE).

Runs with VSRMC_LIB = libvsrmc_hooks.so (ModelChecker.seed_records, csrc/host_test_seed.hpp).  The 1500 sampled states are seeded and every state set is scanned
(where_scan, where_states); then the 150 sampled parents are seeded and every step set is scanned (step_scan, step_pairs).  No oracle and no reference
function here: this process only reports — figures to out.json, the parents' level as the checker stores it (the bag order of a stored record names the
ordinals) to frontier.npz.  The parent process compares everything with the reference.

usage: deep_predicates_worker.py R C n L seeds.npz out.json frontier.npz"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def sets_of(L):
    """(tag, predicates) of the state sets and of the step sets: the texts are what this process needs of them"""
    import deep_predicates_reference as dp
    import step_reference as sr
    import where_reference as wr
    return ((("A", wr.SET_A), ("B", wr.set_b(L)), ("R4", dp.STATE)), (("A", sr.SET_A), ("B", sr.SET_B), ("C", sr.SET_C), ("R4", dp.STEP)))


def main():
    R, C_, n, L = (int(x) for x in sys.argv[1:5])
    z = np.load(sys.argv[5])
    import vsr_tlaplus_amd as vt
    import where_reference as wr
    assert getattr(vt.load(), "vsrmc_test_checker_seed_records", None) is not None, "run me with VSRMC_LIB = libvsrmc_hooks.so"
    state_sets, step_sets = sets_of(L)
    m = vt.Model.from_constants(R=R, C_=C_, n=n, L=L)
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
    mc.close()
    m.close()
    with open(sys.argv[6], "w") as f:
        json.dump(out, f)
    print("ok", flush=True)


if __name__ == "__main__":
    main()
